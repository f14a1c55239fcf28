#!/usr/bin/env python3
"""Orthant-wise Newton: the HIP path (csrc/own.hip) against the same operation sequence issued through torch on the
same GPU (tests/own_model.py on device tensors: rocBLAS products, ATen element-wise passes and reductions, one host
read per line-search trial -- how the reference's orthant_wise_newton.py itself runs on a GPU tensor; its Brent search
is scipy's).

Legs alternate in one process, each run timed with device events around the whole solve (the Cholesky of the k x k
Hessian included on both sides); the median of --runs (>= 5) runs per leg is reported with ms per iteration and per
line-search evaluation.  Both legs must end at the same objective (--objective-rtol; the codes of two correct
float32 implementations differ after several Brent iterations, their objectives do not).  One JSON line per shape and
line search; --out also writes them to a file.

  python tools/bench_own.py [--shapes 4096x1280x1024,4096x256x1024] [--maxiter 10] [--runs 5] [--out FILE]
  python tools/bench_own.py --profile-leg hip --shapes 4096x1280x1024 --searches brent     # one leg, for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-lasso_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import own_model  # noqa: E402
from recipes import recipe_xw  # noqa: E402


def fixed_step(d, k):
    """the step of line_search='none': a step of 1 diverges on these problems; Brent settles near 0.3 for d > k and,
    where the Hessian is the 1e-4 shift on a (k - d)-dimensional subspace, near 5e-4"""
    return 0.25 if d > k else 5e-4


def torch_route(x, W, z0, alpha, maxiter, search, lr):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z, info = own_model.orthant_wise_newton(W, x, z0, alpha=alpha, lr=lr, maxiter=maxiter, xtol=0.0, line_search=search)
    return z, info["objective"][-1], sum(info["ls_iters"])


def hip_route(x, W, z0, alpha, maxiter, search, lr):
    from lasso_amd.linear.solvers import orthant_wise_newton
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z, info = orthant_wise_newton(W, x, z0, alpha=alpha, lr=lr, maxiter=maxiter, xtol=0.0, line_search=search,
                                      return_info=True)
    return z, info["objective"][-1], sum(info["ls_iters"])


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x1280x1024,4096x256x1024")
    ap.add_argument("--searches", default="brent,backtrack,none")
    ap.add_argument("--maxiter", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--objective-rtol", type=float, default=2e-3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-leg", choices=("hip", "torch"), default=None)
    a = ap.parse_args()
    assert a.runs >= 5 or a.profile_leg
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for shape in a.shapes.split(","):
        n, d, k = map(int, shape.split("x"))
        x, W = recipe_xw(n, d, k, seed=0)
        x, W = x.cuda(), W.cuda()
        z0 = torch.zeros(n, k, device="cuda")
        for search in a.searches.split(","):
            if search == "brent":
                try:
                    import scipy.optimize  # noqa: F401  (the torch leg's Brent search)
                except ImportError:
                    print(json.dumps(dict(shape=[n, d, k], line_search=search, skipped="the torch leg needs scipy")))
                    continue
            lr = fixed_step(d, k) if search == "none" else 1.0
            legs = {"hip": lambda: hip_route(x, W, z0, a.alpha, a.maxiter, search, lr),
                    "torch": lambda: torch_route(x, W, z0, a.alpha, a.maxiter, search, lr)}
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
            rec = dict(shape=[n, d, k], line_search=search, maxiter=a.maxiter, alpha=a.alpha, lr=lr, runs=a.runs)
            for name in legs:
                z, f, evals = last[name]
                rec[name] = dict(ms_median=med[name], ms_min=min(ms[name]), ms_max=max(ms[name]),
                                 ms_per_iteration=med[name] / a.maxiter, evaluations=evals,
                                 ms_per_evaluation=(med[name] / evals) if evals else None, objective=f,
                                 nnz=int((z != 0).sum()))
            rec["hip"].update(launches_per_evaluation=3, host_reads_per_evaluation=1 if search == "brent" else 0.125)
            rec["speedup_over_torch"] = med["torch"] / med["hip"]
            rec["objective_rel_diff"] = abs(rec["hip"]["objective"] - rec["torch"]["objective"]) / abs(rec["torch"]["objective"])
            print(json.dumps(rec), flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(json.dumps(rec) + "\n")
            assert rec["objective_rel_diff"] <= a.objective_rtol, "the legs end at different objectives"


if __name__ == "__main__":
    main()
