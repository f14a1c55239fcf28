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
  --peak TFLOPS   the measured fp64-MFMA rate (tools/ubench/mfma_f64) to quote the achieved share against
  --mstep         instead of the solves: the float64 M-step (csrc/mstep_f64.hip) at --mstep-shape (default config 2's,
                  4096,256,1024), ms per call of its three parts -- the Gram products A = Z^T Z, B = Z^T X, the atom
                  sweep, the ridge solve -- each as hip_f64 (this library on float64 tensors), torch_f64 (the same
                  mathematics as torch ops in float64 on the same GPU: Z.T @ Z and Z.T @ X; the oracle's update_dict
                  loop on device tensors; torch.linalg.cholesky + cholesky_solve) and hip_f32 (this library's fp32
                  kernels).  Legs alternated in one process, device events, median [min .. max]; one JSON line."""
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


def _call_stats(ms):
    ms = sorted(ms)
    return dict(ms_per_call=statistics.median(ms), min=ms[0], max=ms[-1], calls=len(ms))


def mstep(args):
    """the M-step leg: see --mstep in the module docstring"""
    from lasso_amd.engine import HipEngine
    from lasso_amd.linear.solvers import ista
    from oracle import lasso_oracle as orc
    from recipes import recipe_xw
    n, d, k = (int(v) for v in args.mstep_shape.split(","))
    X, W = recipe_xw(n, d, k)
    lr = 1.0 / orc.lipschitz_constant(W.double(), "exact")
    eng = HipEngine()
    x32, w32 = X.cuda(), W.cuda()
    z32 = ista(x32, x32.new_zeros(n, k), w32, ALPHA, lr=lr, maxiter=10, tol=0.0)        # a code as an E-step leaves it
    x64, w64, z64 = x32.double(), w32.double(), z32.double()
    lam = 1e-2 * n
    buf64 = torch.empty(k * k + k * d, dtype=torch.float64, device='cuda')
    buf32 = torch.empty(k * k + k * d, dtype=torch.float32, device='cuda')
    A64, B64 = eng.gram(z64, x64, buf64)
    A32, B32 = eng.gram(z32, x32, buf32)
    D64, D32, Zt = w64.clone(), w32.clone(), z64.clone()

    def torch_sweep():
        D64.copy_(w64)
        Zt.copy_(z64)
        orc.update_dict(D64, x64, Zt)

    def torch_ridge():
        M = A64.clone()
        M.diagonal().add_(lam)
        return torch.cholesky_solve(B64, torch.linalg.cholesky(M)).T

    def hip_sweep(A, B, D, w):
        D.copy_(w)
        return eng.sweep(A, B, D, None, 1e-10, False)
    parts = {
        "gram": {"hip_f64": lambda: eng.gram(z64, x64, buf64),
                 "torch_f64": lambda: (z64.T @ z64, z64.T @ x64),
                 "hip_f32": lambda: eng.gram(z32, x32, buf32)},
        "sweep": {"hip_f64": lambda: hip_sweep(A64, B64, D64, w64),
                  "torch_f64": torch_sweep,
                  "hip_f32": lambda: hip_sweep(A32, B32, D32, w32)},
        "ridge": {"hip_f64": lambda: eng.ridge(A64, B64, lam),
                  "torch_f64": torch_ridge,
                  "hip_f32": lambda: eng.ridge(A32, B32, lam)},
    }
    for legs in parts.values():
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
    torch.cuda.synchronize()
    rec = {"mstep": True, "n": n, "d": d, "k": k, "flop_gram": 2.0 * n * k * (k + d)}
    for part, legs in parts.items():
        times = {name: [] for name in legs}
        while any(len(t) < args.reps or sum(t) < 1e3 * args.seconds for t in times.values()):
            for name, fn in legs.items():
                times[name].append(_once(fn))
        rec[part] = {name: _call_stats(t) for name, t in times.items()}
        rec[part]["hip_f64_over_torch_f64"] = rec[part]["hip_f64"]["ms_per_call"] / rec[part]["torch_f64"]["ms_per_call"]
    # the float64 legs compute the same thing
    Ar, Br = z64.T @ z64, z64.T @ x64
    rec["gram_max_rel_diff"] = max(((A64 - Ar).abs().max() / Ar.abs().max()).item(),
                                   ((B64 - Br).abs().max() / Br.abs().max()).item())
    hip_sweep(A64, B64, D64, w64)
    Dh = D64.clone()
    torch_sweep()
    rec["sweep_max_abs_diff"] = (Dh - D64).abs().max().item()
    rec["ridge_max_abs_diff"] = (eng.ridge(A64, B64, lam) - torch_ridge()).abs().max().item()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mstep", action="store_true", help="time the float64 M-step instead of the solves")
    ap.add_argument("--mstep-shape", default="4096,256,1024", help="n,d,k of the M-step leg")
    ap.add_argument("--shape", action="append", help="n,d,k")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peak", type=float, default=None, help="measured fp64-MFMA TFLOP/s of the device")
    args = ap.parse_args()
    if args.mstep:
        return mstep(args)
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
