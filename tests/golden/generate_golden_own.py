#!/usr/bin/env python3
"""Generate tests/golden/own_cases.npz by running the REAL reference's orthant-wise Newton solver
(rfeinman/pytorch-lasso, lasso/linear/solvers/orthant_wise_newton.py), in float32 AND in float64.

Runs only where the reference is mounted (/root/reference); the .npz it writes is data: the inputs are re-creatable
from the seeded recipes of tests/recipes.py, the expected outputs are stored.  Same scipy shim as
generate_golden_gpsr.py; no reference file is edited or copied.

Each run is observed with sys.settrace: per iteration the unrounded t, ls_iters, f and |dz| at the line that tests
convergence, and (f_new, bound, f) at every backtracking decision.  The float32 run's verbose=2 output and warnings
are stored as well.

Every case is CERTIFIED before it is written (the script exits non-zero otherwise -- choose another seed):
  (a) every backtracking decision is at least 1e-4 |f| from its bound and every |dz| at least 1 % from xtol, in both
      runs;
  (b) spread_z = the maximum over 8 order_seeds x accurate_f in {0, 1} of max|z_model - z_ref32| (tests/own_model.py:
      "another correct float32 implementation"), spread_f likewise for the relative final objective, and the same for
      the per-iteration t, objective and |dz|; all are stored;
  (c) a case compared by its codes needs spread_z <= 2.5e-3;
  (d) a case compared by its objective needs spread_f <= 1e-4.
The model in the reference's order must equal the float32 run bit for bit and the float64 run to 1e-7.

Usage:  python tests/golden/generate_golden_own.py
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
import own_model  # noqa: E402
from own_cases import CASES, ORDER_SEEDS, SPREAD_F_CAP, SPREAD_Z_CAP, case_inputs  # noqa: E402

ref_mod = sys.modules["lasso.linear.solvers.orthant_wise_newton"]
ref_solve = ref_mod.orthant_wise_newton
_MAIN = inspect.unwrap(ref_solve)
_BT = ref_mod.backtracking


def _line_of(fn, fragment):
    src, first = inspect.getsourcelines(fn)
    hits = [first + i for i, s in enumerate(src) if fragment in s]
    assert len(hits) == 1, (fragment, hits)
    return hits[0]


L_STOP = _line_of(_MAIN, "if delta_z <= xtol")
L_DECIDE = _line_of(_BT, "if f_new <= f - tol")


class Observer:
    def __init__(self):
        self.t, self.ls, self.f, self.dz, self.decisions = [], [], [], [], []

    def _local(self, frame, event, arg):
        if event != "line":
            return self._local
        loc = frame.f_locals
        if frame.f_code is _MAIN.__code__ and frame.f_lineno == L_STOP:
            self.t.append(float(loc["t"]))
            self.ls.append(int(loc["ls_iters"]))
            self.f.append(float(loc["f"].double()))
            self.dz.append(float(loc["delta_z"].double()))
        elif frame.f_code is _BT.__code__ and frame.f_lineno == L_DECIDE:
            bound = loc["f"] - loc["tol"] * loc["v"].mul(loc["z_new"] - loc["z"]).sum()
            self.decisions.append((float(loc["f_new"].double()), float(bound.double()), float(loc["f"].double())))
        return self._local

    def __call__(self, frame, event, arg):
        return self._local if frame.f_code in (_MAIN.__code__, _BT.__code__) else None


def run_reference(spec, dtype):
    x, w, z0 = (t.to(dtype) for t in case_inputs(spec))
    obs, out = Observer(), io.StringIO()
    with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(out):
        warnings.simplefilter("always")
        sys.settrace(obs)
        try:
            z = ref_solve(w, x, z0, alpha=spec["alpha"], verbose=2, **spec["kwargs"])
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
    xtol = kw.get("xtol", 1e-5)
    z32, o32, text, msgs = run_reference(spec, torch.float32)
    z64, o64, _, msgs64 = run_reference(spec, torch.float64)
    # (a) no decision that rounding could flip
    for obs in (o32, o64):
        for fn, bound, f in obs.decisions:
            if not abs(fn - bound) >= 1e-4 * abs(f):
                raise SystemExit("case %s refused: backtracking decision too close (%r, %r, %r)" % (name, fn, bound, f))
        for i, dz in enumerate(obs.dz):
            if abs(dz - xtol) < 0.01 * xtol:
                raise SystemExit("case %s refused: |dz| %r within 1%% of xtol at iteration %d" % (name, dz, i + 1))
    # the restatement is the reference
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m32, i32 = own_model.orthant_wise_newton(w, x, z0, alpha=spec["alpha"], **kw)
        m64, i64 = own_model.orthant_wise_newton(w, x, z0, alpha=spec["alpha"], dtype=torch.float64, **kw)
    if not torch.equal(m32, z32) or i32["ls_iters"] != o32.ls:
        raise SystemExit("case %s: the float32 model is not the reference bit for bit (max|dz| = %g)"
                         % (name, float((m32 - z32).abs().max())))
    if float((m64 - z64).abs().max()) > 1e-7:
        raise SystemExit("case %s: the float64 model is %g from the reference" % (name, float((m64 - z64).abs().max())))
    # (b) how far another correct float32 implementation moves the result
    f_ref = o32.f[-1]
    spread = dict(z=0.0, f=0.0, t=0.0, objective=0.0, delta=0.0)
    for seed in ORDER_SEEDS:
        for acc in (False, True):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                zm, im = own_model.orthant_wise_newton(w, x, z0, alpha=spec["alpha"], accurate_f=acc, order_seed=seed, **kw)
            same = im["ls_iters"] == o32.ls or kw["line_search"] == "brent"
            spread["z"] = max(spread["z"], float((zm - z32).abs().max()) if same else float("inf"))
            spread["f"] = max(spread["f"], abs(im["objective"][-1] - f_ref) / abs(f_ref))
            spread["t"] = max(spread["t"], rel(im["t"], o32.t))
            spread["objective"] = max(spread["objective"], rel(im["objective"], o32.f))
            spread["delta"] = max(spread["delta"], rel(im["delta_z"], o32.dz))
    compare = spec["compare"]
    if compare == "z" and not spread["z"] <= SPREAD_Z_CAP:
        raise SystemExit("case %s refused for code comparison: spread_z = %.3g" % (name, spread["z"]))
    if compare == "f" and not spread["f"] <= SPREAD_F_CAP:
        raise SystemExit("case %s refused for objective comparison: spread_f = %.3g" % (name, spread["f"]))
    gap = float((z32.double() - z64).abs().max())
    rec = {"z32": z32.numpy(), "z64": z64.numpy(),
           "t32": np.array(o32.t), "ls32": np.array(o32.ls, dtype=np.int64), "f32": np.array(o32.f), "dz32": np.array(o32.dz),
           "t64": np.array(o64.t), "ls64": np.array(o64.ls, dtype=np.int64), "f64": np.array(o64.f), "dz64": np.array(o64.dz),
           "decisions32": np.array(o32.decisions, dtype=np.float64).reshape(-1, 3),
           "warnings": np.array("\n".join(msgs)), "stdout": np.array(text),
           "spread_z": np.float64(spread["z"]), "spread_f": np.float64(spread["f"]), "spread_t": np.float64(spread["t"]),
           "spread_objective": np.float64(spread["objective"]), "spread_delta": np.float64(spread["delta"]),
           "gap_z": np.float64(gap)}
    print("%-10s iters=%d ls=%s f=%.6e spread_z=%.2e spread_f=%.2e gap=%.2e  %.1fs  warnings=%d" %
          (name, len(o32.f), o32.ls, f_ref, spread["z"], spread["f"], gap, time.time() - t0, len(msgs)))
    return rec


def main():
    arrays = {}
    for name, spec in CASES.items():
        for key, val in run_case(name, spec).items():
            arrays["%s/%s" % (name, key)] = val
    path = os.path.join(HERE, "own_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
