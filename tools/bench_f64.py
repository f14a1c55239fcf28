#!/usr/bin/env python3
"""float64 FISTA on the HIP path (csrc/gemm_f64.hip) against what a user would otherwise run, per shape:
  hip_f64     lasso_amd ista() on float64 device tensors (fp64-MFMA general-GEMM path)
  torch_f64   the oracle's own ops on the same GPU in float64 (oracle.lasso_oracle.fista on .cuda() tensors: torch +
              rocBLAS, the reference's loop)
  hip_f32     lasso_amd ista() on the same problem in fp32 (the fused kernel at config 2, the unfused GEMM path beyond)
Fixed step, no stop rule, --iters iterations per solve; ms per iteration = solve / iters.  Every leg of every shape is
warmed up first; then the legs are ALTERNATED in one process, each timed with device events, until each has at least
--seconds of measured work and --reps solves; median and spread (min .. max) per leg.  FLOPs from shapes: 4 n d k per
iteration (two products).  One JSON line per shape.
  --shape n,d,k   (repeatable) default: config 2 (4096, 256, 1024) and one unfused fp32 shape (16384, 512, 4096)
  --peak TFLOPS   the measured fp64-MFMA rate (tools/ubench/mfma_f64) to quote the achieved share against"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-lasso_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

SHAPES = [(4096, 256, 1024), (16384, 512, 4096)]
ALPHA = 0.3


def _once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ms, iters):
    per = sorted(t / iters for t in ms)
    return dict(ms_per_iteration=statistics.median(per), min=per[0], max=per[-1], solves=len(per))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", action="append", help="n,d,k")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak", type=float, default=None, help="measured fp64-MFMA TFLOP/s of the device")
    args = ap.parse_args()
    from lasso_amd.linear.solvers import ista
    from oracle import lasso_oracle as orc
    from recipes import recipe_xw
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shape] if args.shape else SHAPES
    T = args.iters
    legs = {}
    for n, d, k in shapes:
        X, W = recipe_xw(n, d, k)
        lr = 1.0 / orc.lipschitz_constant(W.double(), "exact")
        x64, w64 = X.double().cuda(), W.double().cuda()
        x32, w32 = X.cuda(), W.cuda()
        z64, z32 = x64.new_zeros(n, k), x32.new_zeros(n, k)
        legs[(n, d, k)] = {
            "hip_f64": lambda x=x64, w=w64, z=z64, lr=lr: ista(x, z, w, ALPHA, lr=lr, maxiter=T, tol=0.0),
            "torch_f64": lambda x=x64, w=w64, z=z64, lr=lr: orc.fista(x, z, w, ALPHA, lr=lr, maxiter=T, tol=0.0),
            "hip_f32": lambda x=x32, w=w32, z=z32, lr=lr: ista(x, z, w, ALPHA, lr=lr, maxiter=T, tol=0.0),
        }
    for shape in shapes:                      # a warm-up of every shape before the first measurement
        for fn in legs[shape].values():
            for _ in range(args.warmup):
                fn()
    torch.cuda.synchronize()
    out = []
    for shape in shapes:
        n, d, k = shape
        times = {name: [] for name in legs[shape]}
        while any(len(t) < args.reps or sum(t) < 1e3 * args.seconds for t in times.values()):
            for name, fn in legs[shape].items():           # alternated: hip_f64, torch_f64, hip_f32, hip_f64, ...
                times[name].append(_once(fn))
        flop = 4.0 * n * d * k
        rec = {"n": n, "d": d, "k": k, "iterations_per_solve": T, "flop_per_iteration": flop}
        for name, t in times.items():
            st = _stats(t, T)
            st["tflops"] = flop / st["ms_per_iteration"] / 1e9
            rec[name] = st
        rec["hip_f64_over_torch_f64"] = rec["hip_f64"]["ms_per_iteration"] / rec["torch_f64"]["ms_per_iteration"]
        if args.peak:
            rec["fp64_mfma_peak_tflops"] = args.peak
            rec["hip_f64_share_of_peak"] = rec["hip_f64"]["tflops"] / args.peak
        # the three legs solve the same problem: the float64 ones agree to summation order
        a, b = legs[shape]["hip_f64"](), legs[shape]["torch_f64"]()
        rec["max_abs_diff_hip_vs_torch_f64"] = (a - b).abs().max().item()
        del a, b
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


if __name__ == "__main__":
    main()
