#!/usr/bin/env python3
"""Conjugate gradients on the HIP path (csrc/conjgrad.hip) against the reference's algorithm itself on the same GPU: the
project's torch model of it (tests/conjgrad_model.py: torch.mm / conv2d / conv_transpose2d on device tensors, the
reference's loop with its three host reads per iteration).

Per shape, in one process, legs alternating, every run timed with device events around the whole call and the median
of --runs (>= 5) reported, with the minimum and maximum (the run-to-run spread):
  * hip:    --short and --long iterations (--conv-short and --conv-long for the convolutional shapes) with rtol = 0 and
            tol = 0 (no host read until the end);
            their difference over (long - short) is the time of one iteration without the set-up
  * plain:  the same with bit 0 of the options' reserved word (dense fp32: the product stores Ap and a pass of its own
            takes the per-row curvature; convolutional: conv_transpose2d as GEMM + overlap-add also where an implicit
            kernel covers the geometry) -- what the fused epilogue / the implicit kernel saves
  * model:  the same pair through the model
Shapes: dense NxK (fp32), dense NxK:f64 (float64, recorded without a bar), conv:gray | conv:rgb | conv:c16 (the
geometries of bench.py --workload conv, tik = 0.5).  TFLOP/s of the dense product are as executed, 2 n k^2 per
iteration, against the fp32-MFMA peak of DESIGN.md (157.3).  One JSON line per shape; --out also writes them to a file.

  python tools/bench_conjgrad.py [--shapes 4096x1024,4096x1024:f64,16384x256,conv:gray,conv:rgb,conv:c16] [--out FILE]
  python tools/bench_conjgrad.py --profile --shapes 4096x1024        # one solve per shape, for a kernel trace
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

import conjgrad_model as model  # noqa: E402
from recipes import recipe_xw  # noqa: E402

PEAK_TFLOPS = 157.3
CONV_CASES = {   # bench.py's: N, C, K, kernel size, padding, code height = width
    "gray": (256, 1, 64, 7, 0, 26), "rgb": (64, 3, 128, 5, 2, 64), "c16": (32, 16, 256, 3, 1, 64)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def problem(shape):
    """-> (tag, hip(maxiter, plain), model(maxiter), flops of the product per iteration or None)"""
    import lasso_amd.conjgrad as cgm
    kw = dict(rtol=0.0, tol=0.0)

    def forced(plain, fn):
        cgm._FORCE_PLAIN[0] = plain
        try:
            return fn()
        finally:
            cgm._FORCE_PLAIN[0] = False

    if shape.startswith("conv:"):
        N, C, K, ks, pd, Hz = CONV_CASES[shape[5:]]
        g = torch.Generator().manual_seed(0)
        w = (torch.randn(K, C, ks, ks, generator=g) / (C * ks * ks) ** 0.5).cuda()
        H = (Hz - 1) - 2 * pd + ks
        x = torch.randn(N, C, H, H, generator=g).cuda()
        b = torch.nn.functional.conv2d(x, w, padding=pd)
        hip = lambda it, plain: forced(plain, lambda: cgm.batch_cg_conv2d(w, b, 0.5, maxiter=it, return_info=True, padding=pd, **kw))  # noqa: E731
        mod = lambda it: model.batch_cg_conv2d(w, b, 0.5, maxiter=it, record=False, padding=pd, **kw)  # noqa: E731
        return dict(conv=shape[5:], geometry=[N, C, K, ks, pd, Hz], tik=0.5), hip, mod, None
    dims, _, dt = shape.partition(":")
    n, k = map(int, dims.split("x"))
    dtype = torch.float64 if dt == "f64" else torch.float32
    # W square and a small shift: a full spectrum and a condition number of a few thousand, so that the iterations are
    # still far from converged at --long (a converged run ends in exit 2, curv_sum <= 3 eps, whatever rtol and tol are)
    _, W = recipe_xw(1, k, k, seed=0)
    A = (W.double().T @ W.double() + 1e-3 * torch.eye(k, dtype=torch.float64)).to(dtype).cuda()
    b = torch.randn(n, k, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dtype).cuda()
    hip = lambda it, plain: forced(plain, lambda: cgm.batch_cg(A, b, maxiter=it, return_info=True, **kw))  # noqa: E731
    mod = lambda it: model.batch_cg(A, b, maxiter=it, record=False, **kw)  # noqa: E731
    return dict(dense=[n, k], dtype=str(dtype)), hip, mod, 2.0 * n * k * k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x1024,4096x1024:f64,16384x256,conv:gray,conv:rgb,conv:c16")
    ap.add_argument("--short", type=int, default=10)
    ap.add_argument("--long", type=int, default=50)
    ap.add_argument("--conv-short", type=int, default=5)
    ap.add_argument("--conv-long", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    assert a.runs >= 5 or a.profile
    assert a.long > a.short >= 1
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for shape in a.shapes.split(","):
        tag, hip, mod, flops = problem(shape)
        # (tik = 0.5 makes the convolutional systems converge, and exit 2 fire, within about 30 iterations)
        short, long_ = (a.conv_short, a.conv_long) if shape.startswith("conv:") else (a.short, a.long)
        if a.profile:
            hip(long_, False)
            torch.cuda.synchronize()
            continue
        legs = {"hip_short": lambda: hip(short, False), "hip_long": lambda: hip(long_, False),
                "plain_short": lambda: hip(short, True), "plain_long": lambda: hip(long_, True),
                "model_short": lambda: mod(short), "model_long": lambda: mod(long_)}
        for fn in legs.values():                           # warm-up: workspaces, code objects, the BLAS's plans
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in legs}
        last = {}
        for _ in range(a.runs):
            for name, fn in legs.items():                  # alternate the legs
                t, last[name] = timed(fn)
                ms[name].append(t)
        med = {name: statistics.median(v) for name, v in ms.items()}
        x_hip, info = last["hip_long"]
        x_mod, info_mod = last["model_long"]
        assert info["iterations"] == info_mod["iterations"] == long_ and info["status"] == 4, \
            "a leg stopped early: HIP %d at %d, the model %d at %d" % (info["status"], info["iterations"], info_mod["status"],
                                                                      info_mod["iterations"])
        assert info["host_reads"] <= 1 and torch.isfinite(x_hip).all()
        span = long_ - short
        per = {leg: (med[leg + "_long"] - med[leg + "_short"]) / span for leg in ("hip", "plain", "model")}
        # the spread of a per-iteration figure: the long leg's range over the span
        spread = {leg: (max(ms[leg + "_long"]) - min(ms[leg + "_long"])) / span for leg in ("hip", "plain", "model")}
        rec = dict(tag, short=short, long=long_, runs=a.runs, form=info["form"], form_plain=last["plain_long"][1]["form"],
                   ms_median=med, ms_min={name: min(v) for name, v in ms.items()},
                   ms_max={name: max(v) for name, v in ms.items()}, ms_per_iteration=per, ms_per_iteration_spread=spread,
                   model_over_hip=per["model"] / per["hip"], plain_over_hip=per["plain"] / per["hip"],
                   max_abs_x_difference_from_model=float((x_hip - x_mod).abs().max()))
        if flops:
            rec["product_tflops_if_the_iteration_were_the_product"] = flops / (per["hip"] * 1e-3) / 1e12
            rec["fraction_of_fp32_mfma_peak"] = rec["product_tflops_if_the_iteration_were_the_product"] / PEAK_TFLOPS
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
