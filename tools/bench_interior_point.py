#!/usr/bin/env python3
"""Interior point: the HIP path (csrc/interior_point.hip) against the reference's formulation issued through torch on the
same GPU -- W_pn = [W, -W], the [n, 2k, d] scaled dictionary, the [n, d, d] batch, torch.linalg.cholesky_ex and
cholesky_solve (written afresh here; no reference text).

Legs alternate in one process, each run timed with device events around the whole solve (the start included on both
sides); the median of --runs (>= 5) runs per leg is reported.  Both legs start from the ridge code, run --maxiter
iterations at tol = 0 and must end at the same lasso objective (--objective-rtol).  The torch leg runs at shapes whose
[n, 2k, d] intermediate stays below TORCH_LEG_MAX_BYTES only: the large shape reports the HIP leg alone (DESIGN.md 3.11
records a launch failure of torch's batched cholesky_solve at large sizes whose cause was never found).  Of the HIP leg
also: the row kernel alone (lasso_interior_point_rows on c = 1, which costs what any c costs) with the TFLOP/s it achieved
on n d^2 k + n d^3 / 3 against the fp32-MFMA peak of DESIGN.md (157.3), its share of the solve, and the bytes of W it
reads (n d k 4).  One JSON line per shape; --out also writes them to a file.

  python tools/bench_interior_point.py [--shapes 8192x64x256,1024x256x1024] [--maxiter 8] [--runs 5] [--out FILE]
  python tools/bench_interior_point.py --profile-leg hip --shapes 8192x64x256      # one leg, for a kernel trace
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

PEAK_TFLOPS = 157.3
ALPHAS = {256: 0.5, 1024: 1.0}
TORCH_LEG_MAX_BYTES = 3 << 29
INF = float("inf")


def lasso_objective(z, x, W, alpha):
    return float(0.5 * (z @ W.T - x).pow(2).sum() + alpha * z.abs().sum())


def torch_route(x, W, z0, alpha, maxiter, barrier_init=0.1, eps=1e-5):
    """the doubled-dictionary formulation on device tensors -> z"""
    n = x.size(0)
    wpn = torch.cat([W, -W], 1)
    zs = torch.cat([torch.relu(z0), torch.relu(-z0)], 1)
    z = zs + 0.1
    y = zs.sign() @ wpn.T
    omega = 1.1 * (y @ W).abs().max(1, keepdim=True)[0]
    lam = alpha * y / omega
    s = alpha - lam @ wpn
    mu = barrier_init * x.new_ones(n, 1)
    for _ in range(maxiter):
        ra = -(lam @ wpn) - s + alpha
        rb = x - z @ wpn.T - lam
        rc = mu - z * s
        s_inv = s.reciprocal().masked_fill(s.abs() < eps, 0)
        dd = s_inv * z
        rhs = rb - (s_inv * rc - dd * ra) @ wpn.T
        m = torch.matmul(wpn, dd.unsqueeze(2) * wpn.T.unsqueeze(0))
        m.diagonal(dim1=1, dim2=2).add_(1)
        chol, info = torch.linalg.cholesky_ex(m)
        d_lam = torch.cholesky_solve(rhs.unsqueeze(2), chol).squeeze(2)
        del m, chol
        d_s = ra - d_lam @ wpn
        d_z = s_inv * (rc - z * d_s)
        beta_z = (-z / d_z).masked_fill(d_z >= 0, INF).min(1, keepdim=True)[0].clamp(None, 1)
        beta_s = (-s / d_s).masked_fill(d_s >= 0, INF).min(1, keepdim=True)[0].clamp(None, 1)
        z = (z + 0.99 * beta_z * d_z).clamp(min=0)
        lam = lam + 0.99 * beta_s * d_lam
        s = (s + 0.99 * beta_s * d_s).clamp(min=0)
        mu = mu * (1 - torch.min(beta_z, beta_s).clamp(None, 0.99))
    zp, zn = z.chunk(2, dim=1)
    return zp - zn


def hip_route(x, W, z0, alpha, maxiter):
    from lasso_amd.linear.solvers import interior_point
    return interior_point(x, W, z0=z0, alpha=alpha, maxiter=maxiter, tol=0.0)[0]


def rows_alone(W, c, b, y):
    """one call of lasso_interior_point_rows on packed device tensors"""
    from lasso_amd import _native as nat
    n, d = b.shape
    k = W.shape[1]
    nat.check(nat.lib().lasso_interior_point_rows(nat.ptr(W), k, nat.ptr(c), k, nat.ptr(b), d, nat.ptr(y), d, n, d, k,
                                                  nat.LASSO_F32, nat.stream_ptr(b.device)))
    return y


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def ridge_start(x, W, alpha):
    m = W.T @ W
    m.diagonal().add_(alpha)
    return torch.linalg.solve(m, (x @ W).T).T.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x64x256,1024x256x1024")
    ap.add_argument("--maxiter", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--objective-rtol", type=float, default=1e-4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-leg", choices=("hip", "torch"), default=None)
    a = ap.parse_args()
    assert a.runs >= 5 or a.profile_leg
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for shape in a.shapes.split(","):
        n, d, k = map(int, shape.split("x"))
        alpha = ALPHAS.get(k, 0.5)
        x, W = recipe_xw(n, d, k, seed=0)
        x, W = x.cuda(), W.cuda()
        z0 = ridge_start(x, W, alpha)
        legs = {"hip": lambda: hip_route(x, W, z0, alpha, a.maxiter)}
        if n * 2 * k * d * 4 <= TORCH_LEG_MAX_BYTES:
            legs["torch"] = lambda: torch_route(x, W, z0, alpha, a.maxiter)
        if a.profile_leg:
            if a.profile_leg in legs:
                legs[a.profile_leg]()
                torch.cuda.synchronize()
            continue
        for fn in legs.values():                       # warm-up: workspaces, rocBLAS / rocSOLVER kernels
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in legs}
        last = {}
        for _ in range(a.runs):
            for name, fn in legs.items():              # alternate the legs
                t, last[name] = timed(fn)
                ms[name].append(t)
        med = {name: statistics.median(v) for name, v in ms.items()}
        rec = dict(shape=[n, d, k], maxiter=a.maxiter, alpha=alpha, runs=a.runs, start="ridge", tol=0.0)
        for name in legs:
            rec[name] = dict(ms_median=med[name], ms_min=min(ms[name]), ms_max=max(ms[name]),
                             ms_per_iteration=med[name] / a.maxiter, lasso_objective=lasso_objective(last[name], x, W, alpha))
        if "torch" in legs:
            rec["speedup_over_torch"] = med["torch"] / med["hip"]
            rec["objective_rel_diff"] = abs(rec["hip"]["lasso_objective"] - rec["torch"]["lasso_objective"]) / \
                abs(rec["torch"]["lasso_objective"])
        else:
            rec["torch"] = "not run: its [n, 2k, d] intermediate is %.1f GB" % (n * 2 * k * d * 4 / 1e9)
        # the row kernel alone, and the solve without iterations (the start pass and the staging)
        c, y = torch.ones(n, k, device="cuda"), torch.empty(n, d, device="cuda")
        rows_alone(W, c, x, y)
        rows_ms = statistics.median(timed(lambda: rows_alone(W, c, x, y))[0] for _ in range(a.runs))
        start_ms = statistics.median(timed(lambda: hip_route(x, W, z0, alpha, 0))[0] for _ in range(a.runs))
        flops = float(n) * d * d * k + float(n) * d ** 3 / 3.0
        rec["hip"].update(start_ms=start_ms, rows_kernel_ms=rows_ms,
                          rows_kernel_share_of_an_iteration=rows_ms / ((med["hip"] - start_ms) / a.maxiter),
                          rows_kernel_tflops=flops / (rows_ms * 1e-3) / 1e12,
                          rows_kernel_fraction_of_fp32_mfma_peak=flops / (rows_ms * 1e-3) / 1e12 / PEAK_TFLOPS,
                          rows_kernel_w_bytes=n * d * k * 4, rows_kernel_w_gbps=n * d * k * 4 / (rows_ms * 1e-3) / 1e9)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
        assert rec.get("objective_rel_diff", 0.0) <= a.objective_rtol, "the legs end at different objectives"


if __name__ == "__main__":
    main()
