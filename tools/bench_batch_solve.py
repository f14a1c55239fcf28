#!/usr/bin/env python3
"""batch_cholesky_solve on the HIP path (csrc/batch_solve.hip) against two yardsticks on the same GPU.

Per shape B x D, in one process, the legs alternated, every run timed with device events around the whole call
(the call's one host read included) and the median of --runs (>= 5) reported with the minimum and maximum:
  * hip    lasso_amd.linear.utils.batch_cholesky_solve on device tensors (the Cholesky route)
  * rows   8192x256 only: lasso_iter_ridge_rows at full support on 8192 x 64 x 256 -- the in-project yardstick, the
           kernel whose block scheme this one took over (DESIGN.md 3.11 records 5.0 ms); it solves
           (G + diag(alpha / |z|) + tikhonov) with ONE shared G, so it reads 256 KB where the new kernel reads 2.1 GB
  * torch  torch.linalg.cholesky_ex + torch.cholesky_solve, for D <= 256 ONLY: DESIGN.md 3.11 records that torch's
           batched cholesky_solve at 1024 x 1024 ended in a GPU launch failure whose cause was not found
Each line reports, per leg, ms, TFLOP/s on B D^3 / 3 against the MFMA peak of the dtype (157.3 fp32, 77.6 fp64,
DESIGN.md), TB/s on the lower triangles' bytes, B D (D + 1) / 2 elements, against the 8 TB/s HBM peak, and the residual
max|A x - b| / max|b| of the leg's own result over the worst system (the product in double, outside the timing).  The
systems are A_i = G_i G_i^T / D + I (well conditioned; the time does not depend on the values).

  python tools/bench_batch_solve.py [--shapes 65536x32,8192x64,8192x256,256x1024,8192x128:f64,1024x512:f64] [--out FILE]
  python tools/bench_batch_solve.py --profile        # one hip call per shape, for a kernel trace
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-lasso_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PEAK_TFLOPS = {torch.float32: 157.3, torch.float64: 77.6}
PEAK_TBS = 8.0
TORCH_MAX_D = 256
DEFAULT = "65536x32,8192x64,8192x256,256x1024,8192x128:f64,1024x512:f64"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def systems(B, D, dtype):
    g = torch.Generator(device="cuda").manual_seed(B + D)
    A = torch.empty(B, D, D, dtype=dtype, device="cuda")
    eye = torch.eye(D, dtype=dtype, device="cuda")
    step = max(1, (1 << 26) // (D * D))
    for i in range(0, B, step):
        G = torch.randn(min(step, B - i), D, D, generator=g, dtype=dtype, device="cuda")
        A[i:i + step] = torch.bmm(G, G.transpose(1, 2)) / D + eye
    b = torch.randn(B, D, generator=g, dtype=dtype, device="cuda")
    return b, A


def residual(b, A, x):
    """max over the systems of max|A x - b| / max|b|, the product in double (setup arithmetic, not a leg)"""
    worst, step = 0.0, max(1, (1 << 25) // (A.shape[1] ** 2))
    for i in range(0, b.shape[0], step):
        r = torch.bmm(A[i:i + step].double(), x[i:i + step].double().unsqueeze(2)).squeeze(2) - b[i:i + step].double()
        worst = max(worst, float((r.abs().amax(1) / b[i:i + step].double().abs().amax(1)).max()))
    return worst


def rows_leg(b, A):
    """lasso_iter_ridge_rows at full support: one G for every row, z = 1 everywhere (alpha / |z| = alpha)"""
    from lasso_amd import _native as nat
    n, k = b.shape
    gram = A[0].contiguous()
    z = torch.ones_like(b)
    out = torch.empty_like(b)
    L = nat.lib()
    ws = nat.workspace(b.device, L.lasso_iter_ridge_workspace_bytes(n, 1, k, nat.LASSO_F32), "iter_ridge_rows")

    def call():
        row, minor, smax = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        nat.check(L.lasso_iter_ridge_rows(nat.ptr(gram), k, nat.ptr(b), k, nat.ptr(z), k, nat.ptr(out), k, n, k, nat.LASSO_F32,
                                          0.5, 1e-4, 1e-8, C.byref(row), C.byref(minor), C.byref(smax), nat.ptr(ws), ws.numel(),
                                          nat.stream_ptr(b.device)))
        assert smax.value == k and row.value < 0
        return out
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    from lasso_amd.linear.utils import batch_cholesky_solve
    lines = []
    for shape in args.shapes.split(","):
        dims, _, dt = shape.partition(":")
        B, D = map(int, dims.split("x"))
        dtype = torch.float64 if dt == "f64" else torch.float32
        b, A = systems(B, D, dtype)
        esize = 8 if dtype == torch.float64 else 4
        flops, tri_bytes = B * D ** 3 / 3.0, B * D * (D + 1) / 2 * esize
        legs = {"hip": lambda: batch_cholesky_solve(b, A, return_info=True)}
        if args.profile:
            x, info = legs["hip"]()
            torch.cuda.synchronize()
            print(json.dumps(dict(shape=shape, profile=True, tier=info["tier"])))
            continue
        if (B, D, dtype) == (8192, 256, torch.float32):
            legs["rows"] = rows_leg(b, A)
        if D <= TORCH_MAX_D:
            legs["torch"] = lambda: torch.cholesky_solve(b.unsqueeze(2), torch.linalg.cholesky_ex(A)[0]).squeeze(2)
        for fn in legs.values():                          # warm-up: code objects, workspaces, torch's handles
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in legs}
        for _ in range(max(5, args.runs)):
            for name, fn in legs.items():
                times[name].append(timed(fn)[0])
        x, info = legs["hip"]()
        line = dict(shape=shape, B=B, D=D, dtype=str(dtype).replace("torch.", ""), tier=info["tier"], route=info["route"],
                    runs=len(times["hip"]))
        for name, ts in times.items():
            ms = statistics.median(ts)
            line[name] = dict(ms=round(ms, 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                              tflops=round(flops / ms / 1e9, 3), of_mfma_peak=round(flops / ms / 1e9 / PEAK_TFLOPS[dtype], 4))
            if name != "rows":
                line[name].update(tri_tbs=round(tri_bytes / ms / 1e9, 3), of_hbm_peak=round(tri_bytes / ms / 1e9 / PEAK_TBS, 4))
        line["hip"]["residual"] = residual(b, A, x)
        if "torch" in legs:
            ref = legs["torch"]()
            line["torch"]["residual"] = residual(b, A, ref)
            line["max_rel_diff_to_torch"] = float(((x - ref).abs().amax(1) / ref.abs().amax(1)).max())
        else:
            line["torch"] = "not run above D = %d (DESIGN.md 3.11)" % TORCH_MAX_D
        lines.append(line)
        print(json.dumps(line), flush=True)
        del b, A, legs
        torch.cuda.empty_cache()
    if args.out and lines:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
