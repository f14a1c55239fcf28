#!/usr/bin/env python3
"""OWL-QN: the HIP path (csrc/owlqn.hip) against the same operation sequence issued through torch on the same GPU
(tests/owlqn_model.py on device tensors: rocBLAS products, ATen element-wise passes and reductions, the two-loop
recursion as 2m dependent dot / add_ pairs over the flattened [n k] state, one host read per line-search trial and per
memory update -- how the reference's owlqn.py itself runs on a GPU tensor; its Brent search is scipy's).

Legs alternate in one process, each run timed with device events around the whole solve; the median of --runs (>= 5)
runs per leg is reported with ms per iteration.  Both legs must end at the same objective (--objective-rtol; the codes
of two correct float32 implementations differ after several iterations, their objectives do not).  The HIP leg is
then run once more through the C ABI with the direction's three launches (pass A, coefficients, pass B) timed by
events of their own: ms per iteration in the direction, its share of an iteration, and the bytes it moves per second
against the 6.3 TB/s a plain copy reaches on this part.  One JSON line per shape, iteration count and line search;
--out also writes them to a file.

  python tools/bench_owlqn.py [--shapes 4096x256x1024,...] [--maxiters 10,20] [--runs 5] [--out FILE]
  python tools/bench_owlqn.py --profile-leg hip --shapes 4096x256x1024 --searches backtrack     # one leg, for a kernel trace
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

import owlqn_model  # noqa: E402
from owlqn_cases import recipe  # noqa: E402

COPY_RATE = 6.3e12                    # bytes / s of a plain device copy on an MI355X
MODES = {"brent": 0, "backtrack": 1, "none": 2}
FIXED_STEP = 0.05                     # line_search='none': a unit step has no descent guarantee with a young memory


def torch_route(x, W, z0, alpha, max_iter, search, lr):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z, info = owlqn_model.owlqn(W, x, z0, alpha=alpha, lr=lr, max_iter=max_iter, xtol=0.0, line_search=search)
    return z, info["objective"][-1], sum(info["ls_iters"]), info["pairs"][-1]


def hip_route(x, W, z0, alpha, max_iter, search, lr):
    from lasso_amd.nonlinear import owlqn, rss
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z, info = owlqn(rss(x, W), z0, alpha=alpha, lr=lr, max_iter=max_iter, xtol=0.0, line_search=search, return_info=True)
    return z, info["objective"][-1], sum(info["ls_iters"]), info["pairs"][-1]


def hip_direction(x, W, z0, alpha, max_iter, search, lr):
    """one more solve through the C ABI with the direction timed -> (ms in the direction, bytes it moved, iterations)"""
    from lasso_amd import _native as nat
    n, d = x.shape
    k = W.shape[1]
    pairs = max(0, min(100, max_iter - 1))
    opts = nat.OwlqnOptions(max_iter, MODES[search], 500, 100, lr, 0.0, 0.1, 0.95, 2)
    res = nat.OwlqnResult()
    L = nat.lib()
    ws = nat.workspace(x.device, L.lasso_owlqn_workspace_bytes(n, d, k, nat.LASSO_F32, pairs), "owlqn")
    z = torch.empty(n, k, device=x.device)
    nat.check(L.lasso_owlqn_solve(nat.ptr(x), d, nat.ptr(W), k, nat.ptr(z0), k, nat.ptr(z), k, n, d, k, nat.LASSO_F32, alpha,
                                  C.byref(opts), C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(x.device)))
    return res.direction_ms, res.direction_bytes, res.n_iter


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x256x1024,4096x1280x1024,4096x256x8192")
    ap.add_argument("--searches", default="brent,backtrack,none")
    ap.add_argument("--maxiters", default="10,20")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--objective-rtol", type=float, default=2e-3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-leg", choices=("hip", "torch"), default=None)
    a = ap.parse_args()
    assert a.runs >= 5 or a.profile_leg
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    slower = []
    for shape in a.shapes.split(","):
        n, d, k = map(int, shape.split("x"))
        x, W = recipe(n, d, k, 0)
        x, W = x.cuda(), W.cuda()
        z0 = torch.zeros(n, k, device="cuda")
        for max_iter in map(int, a.maxiters.split(",")):
            for search in a.searches.split(","):
                if search == "brent":
                    try:
                        import scipy.optimize  # noqa: F401  (the torch leg's Brent search)
                    except ImportError:
                        print(json.dumps(dict(shape=[n, d, k], line_search=search, skipped="the torch leg needs scipy")))
                        continue
                lr = FIXED_STEP if search == "none" else 1.0
                legs = {"hip": lambda: hip_route(x, W, z0, a.alpha, max_iter, search, lr),
                        "torch": lambda: torch_route(x, W, z0, a.alpha, max_iter, search, lr)}
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
                rec = dict(shape=[n, d, k], line_search=search, max_iter=max_iter, alpha=a.alpha, lr=lr, runs=a.runs)
                for name in legs:
                    z, f, evals, pairs = last[name]
                    rec[name] = dict(ms_median=med[name], ms_min=min(ms[name]), ms_max=max(ms[name]),
                                     ms_per_iteration=med[name] / max_iter, evaluations=evals, objective=f,
                                     pairs_held=pairs, nnz=int((z != 0).sum()))
                dir_ms, dir_bytes, its = hip_direction(x, W, z0, a.alpha, max_iter, search, lr)
                rec["hip"]["direction"] = dict(ms_per_iteration=dir_ms / its, share_of_iteration=dir_ms / med["hip"],
                                               gbytes_per_s=dir_bytes / (dir_ms * 1e-3) / 1e9 if dir_ms > 0 else None,
                                               fraction_of_copy_rate=dir_bytes / (dir_ms * 1e-3) / COPY_RATE if dir_ms > 0 else None,
                                               launches_per_iteration=3)
                rec["speedup_over_torch"] = med["torch"] / med["hip"]
                rec["objective_rel_diff"] = abs(rec["hip"]["objective"] - rec["torch"]["objective"]) / abs(rec["torch"]["objective"])
                print(json.dumps(rec), flush=True)
                if a.out:
                    with open(a.out, "a") as fh:
                        fh.write(json.dumps(rec) + "\n")
                assert rec["objective_rel_diff"] <= a.objective_rtol, "the legs end at different objectives"
                if rec["speedup_over_torch"] < 1.0:
                    slower.append((shape, max_iter, search, rec["speedup_over_torch"]))
    assert not slower, "the HIP leg is slower than the torch leg on: %s" % slower


if __name__ == "__main__":
    main()
