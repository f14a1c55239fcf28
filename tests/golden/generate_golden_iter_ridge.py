#!/usr/bin/env python3
"""Generate tests/golden/iter_ridge_cases.npz by running the REAL reference's iterated-ridge solver
(rfeinman/pytorch-lasso, lasso/linear/solvers/iterative_ridge.py, cg=False), in float32 AND in float64.

Runs only where the reference is mounted (/root/reference); the .npz it writes is data: the inputs are re-creatable
from the seeded recipes of tests/recipes.py, the expected outputs are stored.  Same scipy shim as
generate_golden_own.py; no reference file is edited or copied.

Each run is observed with sys.settrace at the line that tests convergence: per iteration fval, sum |update|, t, and the
support counts of the new z.  The float32 run's verbose output and warnings are stored as well.

Every case is CERTIFIED before it is written (the script exits non-zero otherwise -- choose another seed):
  (a) no sum |update| is within 1 % of the scaled tol at any iteration, in either run;
  (b) the compacted model (tests/iter_ridge_model.py) in the reference's order is within 64 float32 ulp of max |z| of
      the float32 run wherever codes are compared (bitwise is not attainable: the compacted system sums in another
      order), and the float64 model within 1e-7 of the float64 run; what was measured is stored (model_gap32 / 64);
  (c) spread_z = the maximum over 8 order_seeds of max|z_model - z_ref32| ("another correct float32 implementation"),
      spread_f likewise for the relative final objective, and the same for the per-iteration fval, update and t;
  (d) a case compared by its codes needs spread_z <= 2.5e-3, one compared by its objective spread_f <= 1e-4.

Usage:  python tests/golden/generate_golden_iter_ridge.py
"""
import contextlib
import inspect
import io
import os
import sys
import time
import warnings

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
import iter_ridge_model  # noqa: E402
from iter_ridge_cases import CASES, ORDER_SEEDS, SPREAD_F_CAP, SPREAD_Z_CAP, case_inputs  # noqa: E402

ref_mod = sys.modules["lasso.linear.solvers.iterative_ridge"]
ref_solve = ref_mod.iterative_ridge
_MAIN = inspect.unwrap(ref_solve)
ULP32 = float(np.finfo(np.float32).eps)


def _line_of(fn, fragment):
    src, first = inspect.getsourcelines(fn)
    hits = [first + i for i, s in enumerate(src) if fragment in s]
    assert len(hits) == 1, (fragment, hits)
    return hits[0]


L_STOP = _line_of(_MAIN, "if update.abs().sum() <= tol")


class Observer:
    def __init__(self):
        self.f, self.update, self.t, self.smax, self.smean, self.tol = [], [], [], [], [], None

    def _local(self, frame, event, arg):
        if event == "line" and frame.f_lineno == L_STOP:
            loc = frame.f_locals
            self.tol = float(loc["tol"])
            self.f.append(float(loc["fval"].double()))
            self.update.append(float(loc["update"].abs().sum().double()))
            self.t.append(float(loc["t"]) if loc["line_search"] else 1.0)
            counts = (~(loc["z"].abs() < loc["eps"])).sum(1)
            self.smax.append(int(counts.max()))
            self.smean.append(float(counts.double().mean()))
        return self._local

    def __call__(self, frame, event, arg):
        return self._local if frame.f_code is _MAIN.__code__ else None


def run_reference(spec, dtype):
    x, w, z0 = (t.to(dtype) for t in case_inputs(spec))
    obs, out = Observer(), io.StringIO()
    with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(out):
        warnings.simplefilter("always")
        sys.settrace(obs)
        try:
            z = ref_solve(z0, x, w, alpha=spec["alpha"], verbose=True, **spec["kwargs"])
        finally:
            sys.settrace(None)
    return z, obs, out.getvalue(), [str(c.message) for c in caught]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return float("inf")
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def run_case(name, spec):
    t0 = time.time()
    x, w, z0 = case_inputs(spec)
    kw = dict(spec["kwargs"])
    z32, o32, text, msgs = run_reference(spec, torch.float32)
    z64, o64, _, _ = run_reference(spec, torch.float64)
    # (a) no stop decision that rounding could flip
    for obs in (o32, o64):
        for i, u in enumerate(obs.update):
            if abs(u - obs.tol) < 0.01 * obs.tol:
                raise SystemExit("case %s refused: sum |update| %r within 1%% of tol %r at iteration %d" % (name, u, obs.tol, i + 1))
    if spec.get("stops") and not (len(o32.f) < kw["maxiter"] and len(o32.f) == len(o64.f)):
        raise SystemExit("case %s refused: the stop did not fire alike in both runs (%d, %d)" % (name, len(o32.f), len(o64.f)))
    # (b) the compacted restatement against the reference
    m32, i32 = iter_ridge_model.iterative_ridge(z0, x, w, alpha=spec["alpha"], **kw)
    m64, i64 = iter_ridge_model.iterative_ridge(z0, x, w, alpha=spec["alpha"], dtype=torch.float64, **kw)
    gap32 = float((m32 - z32).abs().max())
    gap64 = float((m64 - z64).abs().max())
    compare = spec["compare"]
    if compare == "z" and (gap32 > 64 * ULP32 * max(1.0, float(z32.abs().max())) or i32["iterations"] != len(o32.f)):
        raise SystemExit("case %s: the float32 model is %g from the reference" % (name, gap32))
    if gap64 > 1e-7 and compare == "z":
        raise SystemExit("case %s: the float64 model is %g from the reference" % (name, gap64))
    # (c) how far another correct float32 implementation moves the result
    f_ref = o32.f[-1]
    spread = dict(z=0.0, f=0.0, fval=0.0, update=0.0, t=0.0)
    for seed in ORDER_SEEDS:
        zm, im = iter_ridge_model.iterative_ridge(z0, x, w, alpha=spec["alpha"], order_seed=seed, **kw)
        same = im["iterations"] == len(o32.f)
        spread["z"] = max(spread["z"], float((zm - z32).abs().max()) if same else float("inf"))
        spread["f"] = max(spread["f"], abs(im["fval"][-1] - f_ref) / abs(f_ref))
        spread["fval"] = max(spread["fval"], rel(im["fval"], o32.f))
        spread["update"] = max(spread["update"], rel(im["update"], o32.update))
        spread["t"] = max(spread["t"], rel(im["t"], o32.t))
    if compare == "z" and not spread["z"] <= SPREAD_Z_CAP:
        raise SystemExit("case %s refused for code comparison: spread_z = %.3g" % (name, spread["z"]))
    if compare == "f" and not spread["f"] <= SPREAD_F_CAP:
        raise SystemExit("case %s refused for objective comparison: spread_f = %.3g" % (name, spread["f"]))
    gap = float((z32.double() - z64).abs().max())
    rec = {"z32": z32.numpy(), "z64": z64.numpy(),
           "f32": np.array(o32.f), "update32": np.array(o32.update), "t32": np.array(o32.t),
           "smax32": np.array(o32.smax, dtype=np.int64), "smean32": np.array(o32.smean),
           "f64": np.array(o64.f), "update64": np.array(o64.update), "t64": np.array(o64.t),
           "tol": np.float64(o32.tol), "warnings": np.array("\n".join(msgs)), "stdout": np.array(text),
           "spread_z": np.float64(spread["z"]), "spread_f": np.float64(spread["f"]),
           "spread_fval": np.float64(spread["fval"]), "spread_update": np.float64(spread["update"]),
           "spread_t": np.float64(spread["t"]), "gap_z": np.float64(gap),
           "model_gap32": np.float64(gap32), "model_gap64": np.float64(gap64)}
    print("%-9s iters=%d f=%.6e spread_z=%.2e spread_f=%.2e gap=%.2e model32=%.2e model64=%.2e smax=%s  %.1fs" %
          (name, len(o32.f), f_ref, spread["z"], spread["f"], gap, gap32, gap64, o32.smax[-1], time.time() - t0))
    return rec


def main():
    arrays = {}
    for name, spec in CASES.items():
        for key, val in run_case(name, spec).items():
            arrays["%s/%s" % (name, key)] = val
    path = os.path.join(HERE, "iter_ridge_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
