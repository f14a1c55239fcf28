#!/usr/bin/env python
"""Prints one JSON line per call of every size query of the C ABI (``*_workspace_bytes``, ``*_trace_bytes``,
``lasso_mstep_pipe_stages`` / ``_stage_rows``) over a fixed grid of shapes.  Host only: no tensor, no launch.  Two
builds of the library carve the same workspaces exactly when their outputs are equal:

    python tools/abi_sizes.py > head.jsonl
    python tools/abi_sizes.py --lib /path/to/other/liblasso_hip.so > other.jsonl
    diff head.jsonl other.jsonl
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-lasso_amd"))
sys.path.insert(0, ROOT)

NS = (0, 1, 37, 4096, 70000)
DKS = ((8, 12), (64, 256), (64, 300), (128, 384), (128, 512), (256, 768), (256, 1024), (300, 520), (256, 4096),
       (2100, 2100))
DTYPES = (0, 1, 2)                   # LASSO_F32, LASSO_BF16, LASSO_F64
MAXITERS = (0, 10, 100)
TOLS = (0.0, 1e-5)
STOPS = (0, 1, 2)
BACKTRACK = (0, 1)


def conv_geometries():
    """bench.py's three convolution cases and a 1 x 1 image: (N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw)"""
    from bench import CONV_CASES
    out = []
    for name in sorted(CONV_CASES):
        N, Cc, K, ks, pd, Hz = CONV_CASES[name]
        H = (Hz - 1) - 2 * pd + ks
        out.append((N, Cc, H, H, K, Hz, Hz, ks, ks, 1, 1, pd, pd))
    out.append((1, 1, 1, 1, 2, 1, 1, 3, 3, 1, 1, 1, 1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", help="another build of liblasso_hip.so (default: the one in the tree)")
    args = ap.parse_args()
    from lasso_amd import _native as nat
    if args.lib:
        nat.use_library(os.path.abspath(args.lib))
    L = nat.lib()

    def emit(fn, *a):
        print(json.dumps({"fn": fn, "args": list(a), "value": int(getattr(L, fn)(*a))}))

    for n, (d, k), dt, mi, tol, stop, bt in itertools.product(NS, DKS, DTYPES, MAXITERS, TOLS, STOPS, BACKTRACK):
        emit("lasso_fista_workspace_bytes", n, d, k, dt, mi, tol, stop, bt)
    for n, (d, k) in itertools.product(NS, DKS):
        for fn in ("lasso_objective_workspace_bytes", "lasso_objective_f64_workspace_bytes", "lasso_gram_workspace_bytes",
                   "lasso_gram_f64_workspace_bytes", "lasso_mstep_pipe_workspace_bytes", "lasso_mstep_pipe_stages",
                   "lasso_fista_backward_workspace_bytes"):
            emit(fn, n, d, k)
        for dt in DTYPES:
            emit("lasso_cd_workspace_bytes", n, d, k, dt)
            emit("lasso_gpsr_workspace_bytes", n, d, k, dt)
        for s in range(int(L.lasso_mstep_pipe_stages(n, d, k))):
            lo, hi = C.c_int64(0), C.c_int64(0)
            st = L.lasso_mstep_pipe_stage_rows(n, d, k, s, C.byref(lo), C.byref(hi))
            print(json.dumps({"fn": "lasso_mstep_pipe_stage_rows", "args": [n, d, k, s],
                              "value": [int(st), lo.value, hi.value]}))
    for d, k in DKS:
        for fn in ("lasso_lipschitz_workspace_bytes", "lasso_dict_sweep_workspace_bytes",
                   "lasso_dict_sweep_f64_workspace_bytes", "lasso_init_transpose_workspace_bytes",
                   "lasso_ridge_workspace_bytes", "lasso_ridge_f64_workspace_bytes"):
            emit(fn, d, k)
    for g in conv_geometries():
        emit("lasso_conv_ista_workspace_bytes", *g)
        emit("lasso_conv_ista_backward_workspace_bytes", *g)
        for iters in (0, 1, 20):
            emit("lasso_conv_ista_trace_bytes", *g, iters)
        for sample in (0, 16):
            emit("lasso_conv_lip_workspace_bytes", g[4], g[1], g[7], sample)


if __name__ == "__main__":
    main()
