#!/usr/bin/env python3
"""BFGS iterated ridge: the HIP path (csrc/irbfgs.hip) against the same operation sequence issued through torch on the
same GPU (tests/irbfgs_model.py on device tensors: rocBLAS products, the reference's bmm / baddbmm / addcdiv / where
update with its [n,k,k] temporaries, torch.linalg.cholesky_ex + cholesky_solve, one host read per line-search
evaluation and per iteration -- how the reference's iterative_ridge_bfgs.py itself runs on a GPU tensor; its Brent
search is scipy's).

Legs alternate in one process, each run timed with device events around the whole solve; the median of --runs (>= 5)
runs per leg is reported with ms per iteration.  The final objective of BOTH legs is reported, computed in double from
the codes each returned (torch's batched float32 solve has been seen wrong at some sizes on this GPU: speed alone is
not a comparison).  The HIP leg is then run once more through the C ABI with bit 1 of options.reserved: the update
launches (row_kernel) and the solves of the systems are timed by events of their own -- ms per iteration in the row
kernel, the bytes per second of its k x k traffic (B read twice and written once, half a matrix written for the
system: 3.5 k^2 floats per valid row) against the 6.3 TB/s a plain copy reaches on this part, and the share of an
iteration spent in the Cholesky solve.  One JSON line per shape and line search; --out also writes them to a file.

k = 1024 is not in the default list: the torch leg's cholesky_solve ended in a launch failure on a batch of 32 such
systems (profiles/irbfgs/README.md).

  python tools/bench_irbfgs.py [--shapes 4096x64x64,...] [--maxiter 10] [--runs 5] [--out FILE]
"""
import argparse
import ctypes as C
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

import irbfgs_model  # noqa: E402
from irbfgs_cases import recipe  # noqa: E402

COPY_RATE = 6.3e12                    # bytes / s of a plain device copy on an MI355X
FIXED_STEP = 0.3


def objective64(W, x, z, alpha):
    r = z.double() @ W.double().T - x.double()
    return 0.5 * float(r.square().sum()) + alpha * float(z.double().abs().sum())


def torch_route(x, W, z0, alpha, maxiter, search):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z, info = irbfgs_model.iterative_ridge_bfgs(W, x, z0, alpha=alpha, lr=FIXED_STEP, xtol=0.0, line_search=search,
                                                    maxiter=maxiter)
    return z, info["iterations"], sum(info["ls_iters"]), sum(info["lu"])


def hip_route(x, W, z0, alpha, maxiter, search):
    from lasso_amd.nonlinear import iterative_ridge_bfgs, rss
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z, info = iterative_ridge_bfgs(rss(x, W), z0, alpha=alpha, lr=FIXED_STEP, xtol=0.0, line_search=search,
                                       maxiter=maxiter, return_info=True)
    return z, info["iterations"], sum(info["ls_iters"]), sum(info["lu"])


def hip_timed_parts(x, W, z0, alpha, maxiter, search):
    """one more solve through the C ABI with the row kernel and the solves timed -> the result struct"""
    from lasso_amd import _native as nat
    n, d = x.shape
    k = W.shape[1]
    opts = nat.IrbfgsOptions(maxiter, 1 if search else 0, FIXED_STEP, 0.0, 1e-4, float(torch.finfo(torch.float32).eps),
                             nat.IRBFGS_TIME_ROWS)
    res = nat.IrbfgsResult()
    L = nat.lib()
    ws = nat.workspace(x.device, L.lasso_irbfgs_workspace_bytes(n, d, k, nat.LASSO_F32), "iterative_ridge_bfgs")
    z = torch.empty(n, k, device=x.device)
    nat.check(L.lasso_irbfgs_solve(nat.ptr(x), d, nat.ptr(W), k, nat.ptr(z0), k, nat.ptr(z), k, n, d, k, nat.LASSO_F32, alpha,
                                   C.byref(opts), C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(x.device)))
    return res


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x64x64,1024x64x128,1024x128x256,128x128x512")
    ap.add_argument("--maxiter", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--searches", default="fixed,brent")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from lasso_amd import _native as nat
    runs = max(args.runs, 5)
    dev = torch.device("cuda", 0)
    lines = []
    for shape in args.shapes.split(","):
        n, d, k = (int(v) for v in shape.split("x"))
        x, W = recipe(n, d, k, seed=0)
        g = torch.Generator().manual_seed(1)
        z0 = 0.3 * torch.randn(n, k, generator=g)
        z0 = torch.where(torch.rand(n, k, generator=g) >= 0.3, z0, torch.zeros(()))
        x, W, z0 = x.to(dev), W.to(dev), z0.to(dev)
        for name in args.searches.split(","):
            search = name == "brent"
            legs = {"hip": hip_route, "torch": torch_route}
            times = {leg: [] for leg in legs}
            last = {}
            for leg, fn in legs.items():                       # warm-up: code objects, rocBLAS / rocSOLVER handles
                fn(x, W, z0, args.alpha, 2, search)
            for _ in range(runs):
                for leg, fn in legs.items():
                    ms, out = timed(lambda: fn(x, W, z0, args.alpha, args.maxiter, search))
                    times[leg].append(ms)
                    last[leg] = out
            res = hip_timed_parts(x, W, z0, args.alpha, args.maxiter, search)
            rec = dict(n=n, d=d, k=k, line_search=name, maxiter=args.maxiter, alpha=args.alpha, runs=runs)
            for leg in legs:
                z, its, evals, lus = last[leg]
                med = statistics.median(times[leg])
                rec[leg] = dict(ms=med, ms_min=min(times[leg]), ms_per_iter=med / max(its, 1), iterations=its, ls_evaluations=evals,
                                lu_iterations=lus, objective=objective64(W, x, z, args.alpha),
                                finite=bool(torch.isfinite(z).all()))
            updates = max(res.n_iter - 1, 1)
            row_ms = res.row_ms / updates
            rate = res.row_bytes / (res.row_ms * 1e-3) if res.row_ms > 0 else 0.0
            rec["hip"].update(row_kernel_ms_per_update=row_ms, row_kernel_bytes_per_s=rate,
                              row_kernel_fraction_of_copy_rate=rate / COPY_RATE,
                              row_kernel_share_of_iteration=row_ms / rec["hip"]["ms_per_iter"],
                              solve_ms_per_iter=res.solve_ms / max(res.n_iter, 1),
                              solve_share_of_iteration=res.solve_ms / max(res.n_iter, 1) / rec["hip"]["ms_per_iter"],
                              workspace_bytes=int(nat.lib().lasso_irbfgs_workspace_bytes(n, d, k, nat.LASSO_F32)))
            rec["speedup_over_torch"] = rec["torch"]["ms"] / rec["hip"]["ms"]
            rec["objective_rel_diff"] = abs(rec["hip"]["objective"] - rec["torch"]["objective"]) / abs(rec["torch"]["objective"])
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
