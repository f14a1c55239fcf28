#!/usr/bin/env python3
"""Reverse pass of the convolutional solve (SURVEY.md 8f rows f3 + f4) on bench.py's three conv
geometries (CONV_CASES), 20 iterations (CONV_ITERS) with a fixed step and no stop rule, x, weight and z0 requiring grad.
Medians over --reps runs after warm-up, timed with HIP events:
  traced forward      ista_conv2d with grad (lasso_conv_ista_run_traced: the iterates z_0..z_T kept)
  backward            loss.backward() through it (lasso_conv_ista_backward), per iteration, and its TFLOP/s under
                      the 5-product model (5 x 2 M C kh kw K flop per iteration, M = N Hz Wz)
  torch.autograd      the same forward / backward through oracle.conv_fista on device tensors (ATen / MIOpen)
--ab: the backward with the weight gradient from conv_wgrad_kernel against the conv_patches + gram_tn composition
(LASSO_CONV_WGRAD=gram), and without a weight gradient at all (only x, z0 require grad): dW's share of each."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-lasso_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from bench import CONV_CASES, CONV_ITERS  # noqa: E402


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def _fwd_bwd(solve, x, w, z0, G, need, reps, warmup):
    """median ms of the forward, of the backward (a fresh forward before every backward, outside the timing)"""
    leaves = [t.clone().requires_grad_(n) for t, n in zip((x, w, z0), need)]
    fwd = _time(lambda: solve(*leaves), reps, warmup)
    times = []
    for i in range(warmup + reps):
        for t in leaves:
            t.grad = None
        z = solve(*leaves)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        (z * G).sum().backward()
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    return fwd, statistics.median(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=sorted(CONV_CASES), action="append", help="default: all three")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ab", action="store_true", help="weight-gradient kernel against conv_patches + gram_tn")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.autograd / MIOpen baseline")
    args = ap.parse_args()
    from lasso_amd.conv2d import ista_conv2d
    from oracle import lasso_oracle as orc
    T = CONV_ITERS
    out = []
    for case in args.case or ["gray", "rgb", "c16"]:
        N, C, K, ks, pd, Hz = CONV_CASES[case]
        g = torch.Generator().manual_seed(0)
        w = (torch.randn(K, C, ks, ks, generator=g) / ks).cuda()
        H = (Hz - 1) - 2 * pd + ks
        x = torch.randn(N, C, H, H, generator=g).cuda()
        z0 = torch.zeros(N, K, Hz, Hz, device="cuda")
        G = torch.randn(N, K, Hz, Hz, generator=g).cuda()
        lr = 0.5 / w.pow(2).sum().item()
        M, ckk = N * Hz * Hz, C * ks * ks
        flop_bw = 5 * 2.0 * M * ckk * K * T

        def hip(a, b, c):
            return ista_conv2d(a, c, b, 0.1, padding=pd, maxiter=T, lr=lr, tol=0.0)

        def aten(a, b, c):
            return orc.conv_fista(a, c, b, 0.1, padding=pd, maxiter=T, lr=lr, tol=0.0)

        fwd, bwd = _fwd_bwd(hip, x, w, z0, G, (True, True, True), args.reps, args.warmup)
        rec = {"case": case, "N": N, "C": C, "K": K, "ksize": ks, "padding": pd, "code_hw": Hz, "iterations": T,
               "traced_forward_ms": fwd, "traced_forward_ms_per_iteration": fwd / T,
               "backward_ms": bwd, "backward_ms_per_iteration": bwd / T, "backward_tflops": flop_bw / bwd / 1e9}
        if args.ab:
            os.environ["LASSO_CONV_WGRAD"] = "gram"
            try:
                _, bwd_gram = _fwd_bwd(hip, x, w, z0, G, (True, True, True), args.reps, args.warmup)
            finally:
                os.environ.pop("LASSO_CONV_WGRAD", None)
            _, bwd_nodw = _fwd_bwd(hip, x, w, z0, G, (True, False, True), args.reps, args.warmup)
            rec.update(backward_ms_gram=bwd_gram, backward_ms_without_dw=bwd_nodw,
                       dw_ms_per_iteration_wgrad_kernel=(bwd - bwd_nodw) / T,
                       dw_ms_per_iteration_patches_gram=(bwd_gram - bwd_nodw) / T)
        if not args.no_torch:
            afwd, abwd = _fwd_bwd(aten, x, w, z0, G, (True, True, True), args.reps, args.warmup)
            rec.update(torch_forward_ms=afwd, torch_backward_ms=abwd, torch_backward_ms_per_iteration=abwd / T,
                       backward_speedup_vs_torch=abwd / bwd)
        out.append(rec)
        print(json.dumps(rec), flush=True)
        del x, w, z0, G
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
