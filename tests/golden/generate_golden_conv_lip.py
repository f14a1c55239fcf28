#!/usr/bin/env python3
"""Generate tests/golden/conv_lip_cases.npz by running the REAL reference's lip_constant (rfeinman/pytorch-lasso,
lasso/conv2d/lip_const.py:8-31: ARPACK through scipy.sparse.linalg.eigsh) on the CPU, in float32 AND float64, with
transpose False AND True, on every case of tests/conv_lip_cases.py.

Runs only where the reference is mounted (/root/reference); the .npz it writes is data: the kernels are re-creatable from
the seeded recipes, the values are stored.  lip_const.py imports only torch and scipy, so it is loaded by path; no
reference file is edited or copied.

Per finite case it stores ref64 and ref32 (each for transpose False, True), gap32 = the reference's own
float32-against-float64 gap (relative, the larger of the two transposes), lip_bound_conv2d (NaN where the reference
refuses: stride != 1 or a non-square kernel), spread32 / spread64 = the largest relative distance from ref64-certified
model runs of the model's variants (tests/conv_lip_model.py: permuted summation orders of the dots, float32 with the
dots folded in double, other start vectors) to the model's plain run, and the model's step counts.  For the special
cases it records what the reference does (ARPACK raises on a zero and on a NaN kernel).

Every finite case is CERTIFIED (the script exits non-zero otherwise):
  (a) the reference's two transpose runs in float64 agree to 1e-10 relative;
  (b) the model in float64 with tol = 1e-10 (the case's own tol where it has one) is within 1e-9 of ref64, in the space
      it picks and in the other one.
The lr='exact' case is certified too: bound / exact >= 1.5, and the model's FISTA reaches a lower conv_loss after 20
iterations with the step 1 / exact than with 1 / bound.

Usage:  python tests/golden/generate_golden_conv_lip.py
"""
import importlib.util
import inspect
import json
import os
import sys
import time

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conv_lip_model as model  # noqa: E402
from conv_lip_cases import (CASES, EXACT_LR_ALPHA, EXACT_LR_CASE, EXACT_LR_ITERS, FINITE, ORDER_SEEDS, conv_kwargs,  # noqa: E402
                            exact_lr_image, imsize_of, kernel_of, tol_of)

_spec = importlib.util.spec_from_file_location("reference_lip_const", "/root/reference/lasso/conv2d/lip_const.py")
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a - b)


REFUSALS = {}


def dense_value(w, imsize, transpose, ck):
    """the largest eigenvalue of the operator's dense matrix (LAPACK): where ARPACK cannot run (k >= N at dim = 1)"""
    K, C = w.shape[:2]
    ch = K if transpose else C
    eye = torch.eye(ch * imsize[0] * imsize[1], dtype=w.dtype).view(-1, ch, *imsize)
    if transpose:
        A = torch.nn.functional.conv2d(torch.nn.functional.conv_transpose2d(eye, w, **ck), w, **ck)
    else:
        A = torch.nn.functional.conv_transpose2d(torch.nn.functional.conv2d(eye, w, **ck), w, **ck)
    A = A.reshape(eye.shape[0], -1)
    return float(torch.linalg.eigvalsh((A + A.T) / 2)[-1])


def ref_runs(name, spec, dtype):
    w = kernel_of(spec, dtype)
    out = []
    for t in (False, True):
        try:
            out.append(float(ref.lip_constant(w, imsize_of(spec, t), transpose=t, **conv_kwargs(spec))))
        except TypeError as exc:
            REFUSALS[name] = "%s: %s" % (type(exc).__name__, exc)
            out.append(dense_value(w, imsize_of(spec, t), t, conv_kwargs(spec)))
    return out


def finite_case(name, spec):
    t0 = time.time()
    r64, r32 = ref_runs(name, spec, torch.float64), ref_runs(name, spec, torch.float32)
    if rel(r64[0], r64[1]) > 1e-10:                                                            # (a)
        raise SystemExit("case %s refused: the float64 runs differ, %r" % (name, r64))
    ref64 = r64[0]
    gap32 = max(rel(v, ref64) for v in r32)
    rec = {"ref64": np.array(r64), "ref32": np.array(r32), "gap32": np.float64(gap32)}
    if name in REFUSALS:                      # the values above are LAPACK's on the dense matrix
        rec["reference_refusal"] = np.array(REFUSALS[name])
    w64, w32 = kernel_of(spec, torch.float64), kernel_of(spec, torch.float32)
    ck = conv_kwargs(spec)
    for space in (None, "image", "code"):                                                      # (b)
        v, info = model.lip_constant(w64, spec["imsize"], tol=tol_of(spec, torch.float64), return_info=True, space=space, **ck)
        if rel(v, ref64) > 1e-9:
            raise SystemExit("case %s refused: the float64 model (%s) gives %r, the reference %r" % (name, space, v, ref64))
        if space is None:
            rec["model64"], rec["steps64"], rec["status64"] = np.float64(v), np.int64(info["steps"]), np.array(info["status"])
    for tag, w in (("32", w32), ("64", w64)):
        tol = tol_of(spec, w.dtype)
        base, info = model.lip_constant(w, spec["imsize"], tol=tol, return_info=True, **ck)
        spread = 0.0
        for knobs in model.variants(ORDER_SEEDS):
            if knobs.get("fold64") and tag == "64":
                continue
            v = model.lip_constant(w, spec["imsize"], tol=tol, **knobs, **ck)
            spread = max(spread, rel(v, base))
        rec["spread" + tag] = np.float64(spread)
        if tag == "32":
            rec["model32"], rec["steps32"], rec["status32"] = np.float64(base), np.int64(info["steps"]), np.array(info["status"])
    try:
        bound = float(ref.lip_bound_conv2d(w32, spec["padding"], stride=spec["stride"]))
    except Exception as exc:                                                                   # stride != 1, 3 x 5 kernels
        bound = float("nan")
        rec["bound_refusal"] = np.array("%s: %s" % (type(exc).__name__, exc))
    rec["bound"] = np.float64(bound)
    print("%-10s ref64=%.10g gap32=%.2e spread32=%.2e spread64=%.2e model32-ref=%.2e steps32=%d steps64=%d bound/exact=%.2f  %.1fs"
          % (name, ref64, gap32, rec["spread32"], rec["spread64"], rel(float(rec["model32"]), ref64), rec["steps32"],
             rec["steps64"], bound / ref64, time.time() - t0))
    return rec


def special_case(name, spec):
    """what the reference does with a zero and with a NaN kernel"""
    out = {}
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        try:
            v = ref.lip_constant(kernel_of(spec, dtype), spec["imsize"], **conv_kwargs(spec))
            out["reference" + tag] = np.array("returns %r" % (v,))
        except Exception as exc:
            out["reference" + tag] = np.array("%s: %s" % (type(exc).__name__, str(exc).splitlines()[0][:200]))
        print("%-10s reference %s: %s" % (name, tag, out["reference" + tag]))
    return out


def exact_lr(spec, rec):
    ratio = float(rec["bound"]) / float(rec["ref64"][0])
    if not ratio >= 1.5:
        raise SystemExit("lr='exact' case refused: bound / exact = %.3f" % ratio)
    w, x = kernel_of(spec), exact_lr_image(spec)
    ck = conv_kwargs(spec)
    loss_auto = model.fista_loss(x, w, EXACT_LR_ALPHA, float(np.float32(1.0) / np.float32(rec["bound"])), EXACT_LR_ITERS, **ck)
    loss_exact = model.fista_loss(x, w, EXACT_LR_ALPHA, 1.0 / (float(rec["ref64"][0]) * (1 + 1e-5)), EXACT_LR_ITERS, **ck)
    if not loss_exact < loss_auto * (1 - 1e-3):
        raise SystemExit("lr='exact' case refused: loss %r with the exact step, %r with the bound" % (loss_exact, loss_auto))
    print("lr='exact': bound / exact = %.3f, conv_loss after %d iterations %.6f (exact) < %.6f (auto)"
          % (ratio, EXACT_LR_ITERS, loss_exact, loss_auto))
    return {"exact_lr/ratio": np.float64(ratio), "exact_lr/loss_auto": np.float64(loss_auto),
            "exact_lr/loss_exact": np.float64(loss_exact)}


def signature():
    sig = inspect.signature(ref.lip_constant)
    return [[p.name, p.default is not inspect.Parameter.empty, None if p.default is inspect.Parameter.empty else p.default,
             p.kind.name] for p in sig.parameters.values()]


def main():
    arrays = {}
    for name, spec in CASES.items():
        rec = finite_case(name, spec) if name in FINITE else special_case(name, spec)
        for key, val in rec.items():
            arrays["%s/%s" % (name, key)] = val
        if name == EXACT_LR_CASE:
            arrays.update(exact_lr(spec, rec))
    arrays["signature_json"] = np.array(json.dumps(signature()))
    path = os.path.join(HERE, "conv_lip_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
