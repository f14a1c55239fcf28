#!/usr/bin/env python3
"""GPSR-Basic: the HIP path (csrc/gpsr.hip) against the same op sequence issued through torch on the same GPU
(rocBLAS products + ATen element-wise passes and reductions, one host read per line-search trial and one per stop
test -- how the reference's gpsr.py itself runs on a GPU tensor).

Legs alternate in one process, each run timed with device events around the whole solve; the median of --runs
(>= 5) runs per leg is reported, with ms per iteration and TFLOP/s on (4 + 2 T) n d k flop per iteration (T = trials
as executed).  One JSON line per shape; --out also writes them to a file.

  python tools/bench_gpsr.py [--shapes 4096x256x1024,16384x512x4096] [--maxiter 50] [--runs 5] [--out FILE]
  python tools/bench_gpsr.py --profile-leg hip --shapes 4096x256x1024     # one leg only, for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-lasso_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from recipes import recipe_xw  # noqa: E402


def torch_route(x, W, tau, maxiter, mu=0.1, beta=0.5):
    """GPSR-Basic from a zero start, criterion 3 with tol = 0 (runs maxiter iterations), as torch ops"""
    Ay = x @ W
    z = torch.zeros_like(Ay)
    u, v = torch.relu(z), torch.relu(-z)
    rb = z @ W.T
    r = x - rb
    f = 0.5 * torch.sum(r * r) + tau * (u.sum() + v.sum())
    trials = 0
    for _ in range(maxiter):
        t = rb @ W - Ay
        gu, gv = t + tau, -t + tau
        u_old, v_old = u, v
        cu = gu.masked_fill((u <= 0) & (gu >= 0), 0.)
        cv = gv.masked_fill((v <= 0) & (gv >= 0), 0.)
        q = (cu - cv) @ W.T
        lam = (torch.sum(gu * cu) + torch.sum(gv * cv)) / (torch.sum(q * q) + 1e-7)
        while True:
            trials += 1
            du = torch.relu(u - lam * gu) - u
            dv = torch.relu(v - lam * gv) - v
            u_new, v_new = u + du, v + dv
            rb = (z + (du - dv)) @ W.T
            r = x - rb
            f_new = 0.5 * torch.sum(r * r) + tau * (u_new.sum() + v_new.sum())
            if f_new <= f + mu * (torch.sum(gu * du) + torch.sum(gv * dv)):      # host read
                break
            lam = lam * beta
        f = f_new
        m = torch.min(u_new, v_new)
        u, v = u_new - m, v_new - m
        z = u - v
        numer = torch.max(torch.min(gu, u_old).abs().max(), torch.min(gv, v_old).abs().max())
        crit = numer / torch.max(u_old.abs().max(), v_old.abs().max()).clamp(min=1e-6)
        if crit <= 0.0:                                                           # host read
            break
    return z, float(f), trials


def hip_route(x, W, tau, maxiter):
    from lasso_amd.linear.solvers import gpsr_basic
    z, info = gpsr_basic(x, W, tau, maxiter=maxiter, tol=0.0, return_info=True)
    return z, info["final_objective"], sum(info["trials"])


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x256x1024,16384x512x4096")
    ap.add_argument("--maxiter", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-leg", choices=("hip", "torch"), default=None)
    a = ap.parse_args()
    assert a.runs >= 5 or a.profile_leg
    lines = []
    for shape in a.shapes.split(","):
        n, d, k = map(int, shape.split("x"))
        x, W = recipe_xw(n, d, k, seed=0)
        x, W = x.cuda(), W.cuda()
        legs = {"hip": lambda: hip_route(x, W, a.alpha, a.maxiter), "torch": lambda: torch_route(x, W, a.alpha, a.maxiter)}
        if a.profile_leg:
            legs[a.profile_leg]()
            torch.cuda.synchronize()
            continue
        for fn in legs.values():                       # warm-up: workspaces, rocBLAS kernels
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in legs}
        last = {}
        for _ in range(a.runs):
            for name, fn in legs.items():              # alternate the legs
                t, last[name] = timed(fn)
                ms[name].append(t)
        med = {name: statistics.median(v) for name, v in ms.items()}
        rec = dict(shape=[n, d, k], maxiter=a.maxiter, alpha=a.alpha, runs=a.runs)
        for name in legs:
            z, f, trials = last[name]
            flop = (4.0 * a.maxiter + 2.0 * trials) * n * d * k
            rec[name] = dict(ms_median=med[name], ms_min=min(ms[name]), ms_max=max(ms[name]),
                             ms_per_iteration=med[name] / a.maxiter, tflops=flop / (med[name] * 1e-3) / 1e12,
                             trials=trials, objective=f, nnz=int((z != 0).sum()))
        rec["hip"].update(launches_per_iteration=8, copies_per_iteration=1, host_waits_per_iteration=1)
        rec["speedup_over_torch"] = med["torch"] / med["hip"]
        rec["max_dz_between_legs"] = float((last["hip"][0] - last["torch"][0]).abs().max())
        print(json.dumps(rec))
        lines.append(rec)
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(lines, fh, indent=1)


if __name__ == "__main__":
    main()
