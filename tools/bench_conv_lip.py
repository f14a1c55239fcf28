#!/usr/bin/env python3
"""lip_constant on the HIP path (csrc/conv_lanczos.hip) against the reference's algorithm on the same GPU: ARPACK
(scipy.sparse.linalg.eigsh, k = 1, 'LM') on a LinearOperator whose matvec is torch's conv2d / conv_transpose2d on the
device with a numpy round trip per product -- written here from that description.

Shapes: the three of bench.py --workload conv as one image each (gray: 64 atoms 1x7x7 on 32x32, padding 3; rgb: 128 atoms
3x5x5 on 64x64, padding 2; c16: 256 atoms 16x3x3 on 64x64, padding 1), kernels N(0, 1 / (C ks^2)), float32 and float64.
Before anything is timed both legs must agree to the parity bar: tol + 4 x the model's own float32-against-float64 gap
(float64: 1e-9).  Then, in one process, legs alternating after a warm-up, device events around the whole call, medians
of --runs (>= 5) with minimum and maximum:
  * hip:        lip_constant at its default tol
  * model:      the eigsh leg
  * hip_short / hip_long: tol = 0 and maxiter = --short / --long; their difference over (long - short) is the time of one
                Lanczos step without the set-up
--fista also records, as counts, the FISTA iterations ista_conv2d needs to reach tol = 1e-5 (maxiter 2000) on the three
bench.py cases (their batch cut to --fista-images) with lr='auto' and with lr='exact'.
One JSON line per shape and dtype; --out also writes them to a file.

  python tools/bench_conv_lip.py [--shapes gray,rgb,c16] [--dtypes f32,f64] [--fista] [--out FILE]
  python tools/bench_conv_lip.py --profile --shapes rgb --dtypes f32     # one call, for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-lasso_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = {"gray": (64, 1, 7, 32, 3), "rgb": (128, 3, 5, 64, 2), "c16": (256, 16, 3, 64, 1)}     # K, C, ks, H = W, padding
FISTA_CASES = {   # bench.py's: N, C, K, kernel size, padding, code height = width
    "gray": (256, 1, 64, 7, 0, 26), "rgb": (64, 3, 128, 5, 2, 64), "c16": (32, 16, 256, 3, 1, 64)}
DTYPES = {"f32": torch.float32, "f64": torch.float64}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def kernel_of(shape, dtype):
    K, C, ks, H, pd = SHAPES[shape]
    g = torch.Generator().manual_seed(0)
    return (torch.randn(K, C, ks, ks, generator=g, dtype=torch.float64) / (C * ks * ks) ** 0.5).to(dtype).cuda()


def eigsh_leg(w, H, pd):
    """-> (value, operator applications)"""
    from scipy.sparse import linalg
    C = w.shape[1]
    count = [0]

    def matvec(v):
        count[0] += 1
        t = torch.tensor(v, dtype=w.dtype, device=w.device).view(1, C, H, H)
        t = F.conv_transpose2d(F.conv2d(t, w, padding=pd), w, padding=pd)
        return t.view(-1).cpu().numpy()

    op = linalg.LinearOperator((C * H * H, C * H * H), matvec=matvec, dtype=np.float32 if w.dtype == torch.float32 else np.float64)
    return float(linalg.eigsh(op, k=1, which="LM", return_eigenvectors=False).item()), count[0]


def fista_counts(shape, images):
    from lasso_amd.conv2d import ista_conv2d
    N, C, K, ks, pd, Hz = FISTA_CASES[shape]
    N = min(N, images)
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(K, C, ks, ks, generator=g) / ks).cuda()
    H = (Hz - 1) - 2 * pd + ks
    x = torch.randn(N, C, H, H, generator=g).cuda()
    z0 = torch.zeros(N, K, Hz, Hz, device="cuda")
    out = {}
    for lr in ("auto", "exact"):
        _, info = ista_conv2d(x, z0, w, 0.1, stride=1, padding=pd, maxiter=2000, lr=lr, tol=1e-5, return_info=True)
        out[lr] = info["iterations"]
    return dict(fista_case=shape, images=N, tol=1e-5, iterations_to_tol=out, auto_over_exact=out["auto"] / max(out["exact"], 1))


def main():
    from lasso_amd.conv2d import lip_bound_conv2d, lip_constant
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="gray,rgb,c16")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--short", type=int, default=16)
    ap.add_argument("--long", type=int, default=48)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--fista", action="store_true")
    ap.add_argument("--fista-images", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    assert a.runs >= 5 or a.profile
    assert a.long > a.short >= 1
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")

    warnings.simplefilter("ignore", RuntimeWarning)          # the tol = 0 legs end at maxiter by design
    for shape in a.shapes.split(","):
        K, C, ks, H, pd = SHAPES[shape]
        for dt in a.dtypes.split(","):
            dtype = DTYPES[dt]
            w = kernel_of(shape, dtype)
            kw = dict(padding=pd)
            hip = lambda **k: lip_constant(w, (H, H), return_info=True, **kw, **k)  # noqa: E731
            if a.profile:
                hip()
                torch.cuda.synchronize()
                continue
            v_hip, info = hip()
            v_mod, applications = eigsh_leg(w, H, pd)
            v_mod64, _ = eigsh_leg(kernel_of(shape, torch.float64), H, pd)
            tol = 1e-5 if dtype == torch.float32 else 1e-10
            bar = tol + 4 * abs(v_mod - v_mod64) / v_mod64 if dtype == torch.float32 else 1e-9
            dev = abs(v_hip - v_mod64) / v_mod64
            assert dev <= bar, "the legs disagree: hip %r, eigsh %r (float64 %r), bar %g" % (v_hip, v_mod, v_mod64, bar)
            legs = {"hip": hip, "model": lambda: eigsh_leg(w, H, pd),
                    "hip_short": lambda: hip(tol=0.0, maxiter=a.short), "hip_long": lambda: hip(tol=0.0, maxiter=a.long)}
            for fn in legs.values():                           # warm-up: workspaces, code objects, MIOpen's plans
                fn()
            torch.cuda.synchronize()
            ms = {name: [] for name in legs}
            for _ in range(a.runs):
                for name, fn in legs.items():                  # alternate the legs
                    t, _out = timed(fn)
                    ms[name].append(t)
            med = {name: statistics.median(v) for name, v in ms.items()}
            span = a.long - a.short
            bound = float(lip_bound_conv2d(w, pd))
            emit(dict(shape=shape, dtype=dt, geometry=dict(K=K, C=C, ks=ks, H=H, padding=pd), value=v_hip, eigsh_value=v_mod,
                      eigsh_value_f64=v_mod64, deviation_from_eigsh_f64=dev, parity_bar=bar, toeplitz_bound=bound,
                      bound_over_exact=bound / v_hip, steps=info["steps"], matvecs=info["matvecs"],
                      host_reads=info["host_reads"], status=info["status"], space=info["space"], dim=info["dim"],
                      residual=info["residual"], eigsh_operator_applications=applications, runs=a.runs, ms_median=med,
                      ms_min={n: min(v) for n, v in ms.items()}, ms_max={n: max(v) for n, v in ms.items()},
                      model_over_hip=med["model"] / med["hip"],
                      hip_faster_beyond_spread=max(ms["hip"]) < min(ms["model"]),
                      ms_per_lanczos_step=(med["hip_long"] - med["hip_short"]) / span,
                      ms_per_lanczos_step_spread=(max(ms["hip_long"]) - min(ms["hip_long"])) / span,
                      short=a.short, long=a.long))
    if a.fista and not a.profile:
        for shape in a.shapes.split(","):
            emit(fista_counts(shape, a.fista_images))


if __name__ == "__main__":
    main()
