#!/usr/bin/env python3
"""Generate tests/golden/interior_point_cases.npz by running the REAL reference's interior-point solver
(rfeinman/pytorch-lasso, lasso/linear/solvers/interior_point.py), in float32 AND in float64.

Runs only where the reference is mounted (/root/reference); the .npz it writes is data: the inputs are re-creatable
from the seeded recipes of tests/recipes.py, the expected outputs are stored.  Same scipy shim as
generate_golden_own.py; no reference file is edited or copied.

Each run is observed with sys.settrace at the line that tests convergence: per iteration the objective
alpha sum z + 0.5 sum lambda^2 (in double from the run's z and lambda) and the three ratio means prim_feas, dual_feas,
gap.  The float32 run's verbose output is stored as well.

Every case is CERTIFIED before it is written (the script exits non-zero otherwise -- choose another seed):
  (a) at every iteration of both runs the stop decision is robust: some mean is > 1.01 tol, or all three are < 0.99 tol;
  (b) the model (tests/interior_point_model.py) in index order is within 64 float32 ulp of max |z| of the float32 run
      wherever codes are compared, and the float64 model within 1e-7 of the float64 run; what was measured is stored
      (model_gap32 / 64).  "Index order" is the reference's order of summation (order_seed=None of the model): one
      rounding of difference anywhere grows to hundreds of ulp in four Newton steps.  The HIP path's order, which
      merges the halves first, is held to the float64 run as well, within 1e-7 (model_gap64_path);
  (c) spread_z = the maximum over 8 order_seeds of max|z_model - z_ref32| ("another correct float32 implementation"),
      spread_f likewise for the relative lasso objective of the codes, and the same for the per-iteration records;
  (d) a case compared by its codes needs spread_z <= 2.5e-3, one compared by its objective spread_f <= 1e-4.

Usage:  python tests/golden/generate_golden_interior_point.py
"""
import contextlib
import inspect
import io
import os
import sys
import time

sys.dont_write_bytecode = True
import numpy as np
import scipy.optimize.optimize as _so
from scipy.optimize import _optimize as _o

_so._status_message = _o._status_message          # shim
sys.path.insert(0, "/root/reference")
import torch  # noqa: E402
import lasso  # noqa: E402,F401
import lasso.linear.solvers  # noqa: E402,F401

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import interior_point_model  # noqa: E402
from interior_point_cases import (CASES, ORDER_SEEDS, RECORDS, SPREAD_F_CAP, SPREAD_Z_CAP, case_inputs,  # noqa: E402
                                  lasso_objective)

ref_mod = sys.modules["lasso.linear.solvers.interior_point"]
ref_solve = ref_mod.interior_point
_MAIN = inspect.unwrap(ref_solve)
ULP32 = float(np.finfo(np.float32).eps)


def _line_of(fn, fragment):
    src, first = inspect.getsourcelines(fn)
    hits = [first + i for i, s in enumerate(src) if fragment in s]
    assert len(hits) == 1, (fragment, hits)
    return hits[0]


L_STOP = _line_of(_MAIN, "if ((prim_feas < tol)")


class Observer:
    def __init__(self):
        self.obj, self.prim, self.dual, self.gap = [], [], [], []

    def _local(self, frame, event, arg):
        if event == "line" and frame.f_lineno == L_STOP:
            loc = frame.f_locals
            self.obj.append(float(loc["alpha"] * loc["z"].double().sum() + 0.5 * loc["lmbda"].double().pow(2).sum()))
            self.prim.append(float(loc["prim_feas"].double()))
            self.dual.append(float(loc["dual_feas"].double()))
            self.gap.append(float(loc["gap"].double()))
        return self._local

    def __call__(self, frame, event, arg):
        return self._local if frame.f_code is _MAIN.__code__ else None


def run_reference(spec, dtype):
    x, w, z0 = (t.to(dtype) for t in case_inputs(spec))
    obs, out = Observer(), io.StringIO()
    with contextlib.redirect_stdout(out):
        sys.settrace(obs)
        try:
            z, success = ref_solve(x, w, z0=z0, alpha=spec["alpha"], verbose=True, **spec["kwargs"])
        finally:
            sys.settrace(None)
    return z, bool(success), obs, out.getvalue()


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return float("inf")
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def run_case(name, spec):
    t0 = time.time()
    x, w, z0 = case_inputs(spec)
    kw = dict(spec["kwargs"])
    tol = kw.get("tol", 1e-2)
    z32, ok32, o32, text = run_reference(spec, torch.float32)
    z64, ok64, o64, _ = run_reference(spec, torch.float64)
    # (a) no stop decision that rounding could flip
    for obs in (o32, o64):
        for i in range(len(obs.obj)):
            trio = (obs.prim[i], obs.dual[i], obs.gap[i])
            if tol > 0 and not (max(trio) > 1.01 * tol or max(trio) < 0.99 * tol):
                raise SystemExit("case %s refused: ratio means %r within 1%% of tol %r at iteration %d" % (name, trio, tol, i + 1))
    if len(o32.obj) != len(o64.obj) or ok32 != ok64 or ok32 != bool(spec.get("stops")):
        raise SystemExit("case %s refused: the stop did not fire as expected in both runs (%d %s, %d %s)" %
                         (name, len(o32.obj), ok32, len(o64.obj), ok64))
    # (b) the restatement against the reference
    m32, s32, i32 = interior_point_model.interior_point(x, w, z0, alpha=spec["alpha"], **kw)
    m64, s64, i64 = interior_point_model.interior_point(x, w, z0, alpha=spec["alpha"], dtype=torch.float64, **kw)
    gap32 = float((m32 - z32).abs().max())
    gap64 = float((m64 - z64).abs().max())
    compare = spec["compare"]
    bar32 = 64 * ULP32 * max(1.0, float(z32.abs().max()))
    if i32["iterations"] != len(o32.obj) or s32 != ok32 or i64["iterations"] != len(o64.obj) or s64 != ok64:
        raise SystemExit("case %s: the model stops elsewhere than the reference" % name)
    if compare == "z":
        if gap32 > bar32:
            raise SystemExit("case %s: the float32 model is %g from the reference (bar %g)" % (name, gap32, bar32))
        if gap64 > 1e-7:
            raise SystemExit("case %s: the float64 model is %g from the reference" % (name, gap64))
    # ... and the HIP path's order (halves merged first) in double: the formulation itself, free of float32 rounding
    p64, sp64, ip64 = interior_point_model.interior_point(x, w, z0, alpha=spec["alpha"], dtype=torch.float64,
                                                          order_seed=ORDER_SEEDS[0], **kw)
    gap64_path = float((p64 - z64).abs().max())
    if ip64["iterations"] != len(o64.obj) or sp64 != ok64 or (compare == "z" and gap64_path > 1e-7):
        raise SystemExit("case %s: the float64 model in the path's order is %g from the reference" % (name, gap64_path))
    # (c) how far another correct float32 implementation moves the result
    f_ref = lasso_objective(z32, x, w, spec["alpha"])
    spread = dict(z=0.0, f=0.0, obj=0.0, prim=0.0, dual=0.0, gap=0.0)
    want = dict(obj=o32.obj, prim=o32.prim, dual=o32.dual, gap=o32.gap)
    for seed in ORDER_SEEDS:
        zm, sm, im = interior_point_model.interior_point(x, w, z0, alpha=spec["alpha"], order_seed=seed, **kw)
        same = im["iterations"] == len(o32.obj) and sm == ok32
        spread["z"] = max(spread["z"], float((zm - z32).abs().max()) if same else float("inf"))
        spread["f"] = max(spread["f"], abs(lasso_objective(zm, x, w, spec["alpha"]) - f_ref) / abs(f_ref))
        got = dict(obj=im["obj"], prim=im["prim_feas"], dual=im["dual_feas"], gap=im["gap"])
        for key in RECORDS:
            spread[key] = max(spread[key], rel(got[key], want[key]))
    if compare == "z" and not spread["z"] <= SPREAD_Z_CAP:
        raise SystemExit("case %s refused for code comparison: spread_z = %.3g" % (name, spread["z"]))
    if compare == "f" and not spread["f"] <= SPREAD_F_CAP:
        raise SystemExit("case %s refused for objective comparison: spread_f = %.3g" % (name, spread["f"]))
    gap = float((z32.double() - z64).abs().max())
    rec = {"z32": z32.numpy(), "z64": z64.numpy(), "success": np.bool_(ok32), "tol": np.float64(tol),
           "lasso32": np.float64(f_ref), "lasso64": np.float64(lasso_objective(z64, x, w, spec["alpha"])),
           "stdout": np.array(text), "gap_z": np.float64(gap),
           "spread_z": np.float64(spread["z"]), "spread_f": np.float64(spread["f"]),
           "model_gap32": np.float64(gap32), "model_gap64": np.float64(gap64), "model_bar32": np.float64(bar32),
           "model_gap64_path": np.float64(gap64_path)}
    for key in RECORDS:
        rec[key + "32"] = np.array(getattr(o32, key))
        rec[key + "64"] = np.array(getattr(o64, key))
        rec["spread_" + key] = np.float64(spread[key])
    print("%-10s iters=%d ok=%s F=%.6e spread_z=%.2e spread_f=%.2e gap=%.2e model32=%.2e model64=%.2e path64=%.2e  %.1fs" %
          (name, len(o32.obj), ok32, f_ref, spread["z"], spread["f"], gap, gap32, gap64, gap64_path, time.time() - t0))
    print("           spreads " + " ".join("%s=%.2e" % (key, spread[key]) for key in RECORDS))
    return rec


def main():
    arrays = {}
    for name, spec in CASES.items():
        for key, val in run_case(name, spec).items():
            arrays["%s/%s" % (name, key)] = val
    path = os.path.join(HERE, "interior_point_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
