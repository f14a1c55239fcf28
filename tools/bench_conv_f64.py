#!/usr/bin/env python3
"""float64 ista_conv2d on the HIP path (csrc/conv_f64.hip) against what a user would otherwise
run, on bench.py's three conv cases (gray, rgb, c16), 20 iterations per solve, fixed step, no stop rule:
  hip_f64     lasso_amd ista_conv2d on float64 device tensors
  torch_f64   the same op sequence through torch on float64 tensors of the same GPU: F.conv_transpose2d / F.conv2d plus
              the element-wise passes (oracle.lasso_oracle.conv_fista on .cuda() tensors), torch.autograd for the backward
  hip_f32     lasso_amd ista_conv2d on the same problem in fp32
Two parts per case: the solve (no grad), and the backward with all three gradients (x, z0 and weight require grad; the
timed call is (z * G).sum().backward() on a forward made outside the timed region).  Every leg is warmed up first; then
the legs are ALTERNATED in one process, each call timed with device events around the whole call; median with min ..
max of --reps calls.  FLOPs of the gradient product from shapes: 2 M C kh kw K per iteration.  One JSON line per case.
  --case NAME     (repeatable) gray | rgb | c16; default: all three
  --peak TFLOPS   the measured fp64-MFMA rate (tools/ubench/mfma_f64) to quote the gradient product's share against
  --out PATH      also append the JSON lines to this file"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-lasso_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

# bench.py's CONV_CASES: N, C, K, kernel size, padding, code height = width
CASES = {"gray": (256, 1, 64, 7, 0, 26), "rgb": (64, 3, 128, 5, 2, 64), "c16": (32, 16, 256, 3, 1, 64)}
ITERS = 20
ALPHA = 0.1


def _once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ms):
    ms = sorted(ms)
    return dict(ms_per_call=statistics.median(ms), min=ms[0], max=ms[-1], calls=len(ms))


def _alternate(legs, reps):
    times = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            times[name].append(_once(fn))
    return {name: _stats(t) for name, t in times.items()}


def _backward_leg(fn, x, z0, w, G):
    """-> a callable that times only the backward: the forward graph is rebuilt outside the timed region"""
    leaves = [t.clone().requires_grad_(True) for t in (x, z0, w)]
    state = {}

    def prepare():
        for t in leaves:
            t.grad = None
        state["loss"] = (fn(*leaves) * G).sum()

    def run():
        state.pop("loss").backward()
    return prepare, run, leaves


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--peak", type=float, default=None, help="measured fp64-MFMA TFLOP/s of the device")
    ap.add_argument("--no-backward", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from lasso_amd.conv2d import ista_conv2d
    from oracle import lasso_oracle as orc
    for case in args.case or ["gray", "rgb", "c16"]:
        N, C, K, ks, pd, Hz = CASES[case]
        g = torch.Generator().manual_seed(0)                 # bench.py's run_conv draws
        w = torch.randn(K, C, ks, ks, generator=g) / ks
        H = (Hz - 1) - 2 * pd + ks
        x = torch.randn(N, C, H, H, generator=g)
        G = torch.randn(N, K, Hz, Hz, generator=g)
        lr = 0.5 / w.pow(2).sum().item()
        kw = dict(stride=1, padding=pd, maxiter=ITERS, lr=lr, tol=0.0)
        x32, w32, G32 = x.cuda(), w.cuda(), G.cuda()
        z32 = torch.zeros(N, K, Hz, Hz, device="cuda")
        x64, w64, z64, G64 = x32.double(), w32.double(), z32.double(), G32.double()
        fns = {"hip_f64": (lambda a, b, c: ista_conv2d(a, b, c, ALPHA, **kw), x64, z64, w64, G64),
               "torch_f64": (lambda a, b, c: orc.conv_fista(a, b, c, ALPHA, **kw), x64, z64, w64, G64),
               "hip_f32": (lambda a, b, c: ista_conv2d(a, b, c, ALPHA, **kw), x32, z32, w32, G32)}
        M, ckk = N * Hz * Hz, C * ks * ks
        rec = {"case": case, "N": N, "C": C, "K": K, "kernel": ks, "padding": pd, "Hz": Hz, "M": M,
               "iterations_per_solve": ITERS, "flop_gradient_per_iteration": 2.0 * M * ckk * K}
        with torch.no_grad():
            legs = {name: (lambda f=f, a=a, b=b, c=c: f(a, b, c)) for name, (f, a, b, c, _) in fns.items()}
            for fn in legs.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            rec["solve"] = _alternate(legs, args.reps)
            za, zb = legs["hip_f64"](), legs["torch_f64"]()
            rec["solve"]["max_abs_diff_hip_vs_torch_f64"] = (za - zb).abs().max().item()
            del za, zb
        rec["solve"]["hip_f64_over_torch_f64"] = rec["solve"]["hip_f64"]["ms_per_call"] / rec["solve"]["torch_f64"]["ms_per_call"]
        rec["solve"]["hip_f64_over_hip_f32"] = rec["solve"]["hip_f64"]["ms_per_call"] / rec["solve"]["hip_f32"]["ms_per_call"]
        if not args.no_backward:
            legs = {name: _backward_leg(f, a, b, c, Gd) for name, (f, a, b, c, Gd) in fns.items()}
            times = {name: [] for name in legs}
            for rep in range(args.warmup + args.reps):
                for name, (prepare, run, _) in legs.items():
                    prepare()
                    torch.cuda.synchronize()
                    t = _once(run)
                    if rep >= args.warmup:
                        times[name].append(t)
            rec["backward"] = {name: _stats(t) for name, t in times.items()}
            ga, gb = legs["hip_f64"][2], legs["torch_f64"][2]
            rec["backward"]["max_rel_diff_hip_vs_torch_f64"] = max(
                ((a.grad - b.grad).abs().max() / b.grad.abs().max()).item() for a, b in zip(ga, gb))
            rec["backward"]["hip_f64_over_torch_f64"] = (rec["backward"]["hip_f64"]["ms_per_call"] /
                                                         rec["backward"]["torch_f64"]["ms_per_call"])
            rec["backward"]["hip_f64_over_hip_f32"] = (rec["backward"]["hip_f64"]["ms_per_call"] /
                                                       rec["backward"]["hip_f32"]["ms_per_call"])
            del legs
        if args.peak:
            rec["fp64_mfma_peak_tflops"] = args.peak
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
