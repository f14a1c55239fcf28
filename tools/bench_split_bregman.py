#!/usr/bin/env python3
"""Split Bregman on the HIP path (csrc/split_bregman.hip): what an inner iteration (one n x k x k product with the
solver's epilogue) and an outer iteration cost, against the library's plain NT GEMM of the same product, and what the
stop rule costs.

Per shape, in one process, legs alternating, every run timed with device events around the whole call and the median
of --runs (>= 5) reported:
  * solves of --short and of --long outer iterations with tol = -1 (never stops: no host read until the end); their
    difference over (long - short) is the time of one outer iteration without the set-up (Gram, Cholesky, Aty), and
    that over niter_inner the time of one inner iteration (the last one's wider epilogue and the fold amortised);
  * the same pair with tol = 1e-10, which reads the update once per outer iteration and never stops either: the
    difference per outer iteration is what the stop rule costs;
  * lasso_init_transpose on an [n,k] operand and the [k,k] matrix: the parent's plain GEMM of the same n x k x k product
    (it transposes the [k,k] operand first, inside the call), the yardstick.
TFLOP/s are as executed, 2 n k^2 per inner iteration, against the fp32-MFMA peak of DESIGN.md (157.3).  One JSON line
per shape; --out also writes them to a file.

  python tools/bench_split_bregman.py [--shapes 4096x256x1024,4096x64x256] [--runs 7] [--out FILE]
  python tools/bench_split_bregman.py --profile --shapes 4096x256x1024        # one solve per shape, for a kernel trace
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x256x1024,4096x64x256")
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--niter-inner", type=int, default=5)
    ap.add_argument("--short", type=int, default=4)
    ap.add_argument("--long", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--gemm-calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    assert a.runs >= 5 or a.profile
    assert a.long > a.short >= 1
    from lasso_amd.engine import HipEngine
    from lasso_amd.linear.solvers import split_bregman
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for shape in a.shapes.split(","):
        n, d, k = map(int, shape.split("x"))
        y, A = recipe_xw(n, d, k, seed=0)
        y, A = y.cuda(), A.cuda()

        def solve(maxiter, tol):
            return split_bregman(A, y, alpha=a.alpha, maxiter=maxiter, niter_inner=a.niter_inner, tol=tol, return_info=True)
        if a.profile:
            solve(a.long, -1.0)
            torch.cuda.synchronize()
            continue
        eng = HipEngine(y.device)
        g = torch.Generator().manual_seed(1)
        T = torch.randn(n, k, generator=g).cuda()
        H = torch.randn(k, k, generator=g).cuda()

        def gemm():
            for _ in range(a.gemm_calls):
                eng.init_transpose(T, H)
        legs = {"never_short": lambda: solve(a.short, -1.0), "never_long": lambda: solve(a.long, -1.0),
                "judged_short": lambda: solve(a.short, 1e-10), "judged_long": lambda: solve(a.long, 1e-10), "gemm": gemm}
        for fn in legs.values():                           # warm-up: workspaces, code objects
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in legs}
        last = {}
        for _ in range(a.runs):
            for name, fn in legs.items():                  # alternate the legs
                t, last[name] = timed(fn)
                ms[name].append(t)
        med = {name: statistics.median(v) for name, v in ms.items()}
        x_never, _, info_never = last["never_long"]
        x_judged, _, info_judged = last["judged_long"]
        assert info_never["iterations"] == info_judged["iterations"] == a.long, "a leg stopped early"
        assert torch.equal(x_never, x_judged) and torch.isfinite(x_never).all()
        span = a.long - a.short
        outer = (med["never_long"] - med["never_short"]) / span
        outer_judged = (med["judged_long"] - med["judged_short"]) / span
        inner = outer / a.niter_inner
        gemm_ms = med["gemm"] / a.gemm_calls
        flops = 2.0 * n * k * k
        rec = dict(shape=[n, d, k], alpha=a.alpha, niter_inner=a.niter_inner, short=a.short, long=a.long, runs=a.runs,
                   ms_median=med, ms_min={name: min(v) for name, v in ms.items()},
                   ms_max={name: max(v) for name, v in ms.items()},
                   ms_per_outer_iteration=outer, ms_per_inner_iteration=inner,
                   ms_setup=med["never_short"] - a.short * outer,
                   inner_tflops=flops / (inner * 1e-3) / 1e12,
                   inner_fraction_of_fp32_mfma_peak=flops / (inner * 1e-3) / 1e12 / PEAK_TFLOPS,
                   plain_gemm_ms=gemm_ms, plain_gemm_tflops=flops / (gemm_ms * 1e-3) / 1e12,
                   inner_over_plain_gemm=inner / gemm_ms,
                   ms_per_outer_iteration_judged=outer_judged, stop_rule_ms_per_outer_iteration=outer_judged - outer,
                   update_last=info_never["update"][-1])
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
