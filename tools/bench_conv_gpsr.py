#!/usr/bin/env python3
"""Convolutional GPSR-Basic (lasso_amd.conv2d.gpsr_conv2d) on bench.py's three conv geometries
(CONV_CASES: gray, rgb, c16): a fixed count of iterations (CONV_ITERS), tol = 0, zero start, tau = 0.1.
Medians over --reps solves after warm-up, in one process, timed with HIP events around the whole call (the solve
blocks: the host reads the control block once per iteration).  Per geometry one JSON line:
  ms_per_iteration         the HIP solve / iterations, in the form the dispatch chooses
  form                     that form ('implicit' or 'patches')
  patches_ms_per_iteration the same solve with the general form forced (LASSO_CONV_GPSR_FORM=patches), where the dispatch
                           chose the implicit one: the A/B that decides the dispatch
  host_waits_per_iteration DERIVED from the trial counts, not counted: the driver waits once per batch of trials -- 1 for an
                           iteration whose first trial holds, one more per ladder of 4 further step sizes
  torch_ms_per_iteration   tests/gpsr_conv_model.py on the same device tensors (torch through MIOpen): the
                           comparison -- the parent of this feature cannot run it at all
  speedup_vs_torch         their ratio"""
import argparse
import json
import os
import statistics
import sys
import warnings

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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=sorted(CONV_CASES), action="append", help="default: all three")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=CONV_ITERS)
    ap.add_argument("--tau", type=float, default=0.1)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch / MIOpen comparison")
    args = ap.parse_args()
    from lasso_amd.conv2d import gpsr_conv2d
    import gpsr_conv_model
    T = args.iters
    for case in args.case or ["gray", "rgb", "c16"]:
        N, C, K, ks, pd, Hz = CONV_CASES[case]
        g = torch.Generator().manual_seed(0)
        w = (torch.randn(K, C, ks, ks, generator=g) / ks).cuda()
        H = (Hz - 1) - 2 * pd + ks
        x = torch.randn(N, C, H, H, generator=g).cuda()
        kw = dict(padding=pd, maxiter=T, miniter=T, tol=0.0)
        _, info = gpsr_conv2d(x, w, args.tau, return_info=True, **kw)
        its, trials = info["iterations"], info["trials"]
        ms = _time(lambda: gpsr_conv2d(x, w, args.tau, **kw), args.reps, args.warmup)
        waits = sum(1 + (t - 1 + 3) // 4 for t in trials) / max(1, its)
        M, ckk = N * Hz * Hz, C * ks * ks
        pms = None
        if info["form"] != "patches":
            os.environ["LASSO_CONV_GPSR_FORM"] = "patches"
            try:
                _, pinfo = gpsr_conv2d(x, w, args.tau, return_info=True, **kw)
                assert pinfo["form"] == "patches" and pinfo["trials"] == trials
                pms = _time(lambda: gpsr_conv2d(x, w, args.tau, **kw), args.reps, args.warmup)
            finally:
                os.environ.pop("LASSO_CONV_GPSR_FORM", None)
        rec = {"case": case, "N": N, "C": C, "K": K, "ksize": ks, "padding": pd, "code_hw": Hz, "tau": args.tau,
               "iterations": its, "trials": sum(trials), "form": info["form"], "solve_ms": ms,
               "ms_per_iteration": ms / max(1, its), "host_waits_per_iteration_derived": waits,
               "patches_ms_per_iteration": None if pms is None else pms / max(1, its),
               # per iteration with one trial: AT(rb), A(c), A(z+) -- three products of 2 M C kh kw K flop
               "tflops": 3 * 2.0 * M * ckk * K * its / ms / 1e9}
        if not args.no_torch:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                _, im = gpsr_conv_model.gpsr_conv2d(x, w, args.tau, return_info=True, **kw)
                tms = _time(lambda: gpsr_conv_model.gpsr_conv2d(x, w, args.tau, **kw), args.reps, args.warmup)
            rec.update(torch_iterations=im["iterations"], torch_ms_per_iteration=tms / max(1, im["iterations"]),
                       speedup_vs_torch=(tms / max(1, im["iterations"])) / (ms / max(1, its)))
        print(json.dumps(rec), flush=True)
        del x, w
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
