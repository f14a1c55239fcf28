#!/usr/bin/env python3
"""Generate tests/golden/irbfgs_cases.npz by running the REAL reference's BFGS iterated-ridge solver
(rfeinman/pytorch-lasso, lasso/nonlinear/iterative_ridge_bfgs.py) on f(z) = 0.5 * (z @ W.T - x).pow(2).sum(), in
float32 AND in float64.

Runs only where the reference is mounted (/root/reference); the .npz it writes is data: the inputs are re-creatable
from the seeded recipe of tests/irbfgs_cases.py, the expected outputs are stored.  Same scipy shim as
generate_golden_gpsr.py; no reference file is edited or copied.

Each run is observed with sys.settrace: per iteration the unrounded t, the objective and |dx| at the line that tests
convergence, and every row's y.s at every BFGS update.  The float32 run's verbose=2 output and warnings are stored as
well (maxiter = 0 runs silently: the reference's closing print needs an iteration).

Every case is CERTIFIED before it is written (the script exits non-zero otherwise -- choose another seed):
  (a) every |y.s| is a factor 10 from 1e-10 and every |dx| at least 1 % from xtol, in both runs, and both runs take
      the same verdicts;
  (b) spread_z = the maximum over 8 order_seeds of max|z_model - z_ref32| (tests/irbfgs_model.py: "another correct
      float32 implementation"), spread_f likewise for the relative final objective, and the same for the per-iteration
      t, objective and |dx|; all are stored;
  (c) a case compared by its codes needs spread_z <= 2.5e-3;
  (d) a case compared by its objective needs spread_f <= 1e-4.
The model in the reference's order must equal the float32 run bit for bit and the float64 run to 1e-7.
The NONFINITE cases (one NaN or Inf operand) are recorded as they come: the float32 result, its warnings and the
iteration count.

Usage:  python tests/golden/generate_golden_irbfgs.py
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
import lasso.nonlinear  # noqa: E402,F401

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import irbfgs_model  # noqa: E402
from irbfgs_cases import (CASES, NONFINITE, ORDER_SEEDS, SPREAD_F_CAP, SPREAD_Z_CAP, case_inputs,  # noqa: E402
                          poisoned_inputs)

ref_mod = sys.modules["lasso.nonlinear.iterative_ridge_bfgs"]
ref_solve = ref_mod.iterative_ridge_bfgs
_MAIN = inspect.unwrap(ref_solve)
_UPD = ref_mod.BFGS.update


def _line_of(fn, fragment):
    src, first = inspect.getsourcelines(fn)
    hits = [first + i for i, s in enumerate(src) if fragment in s]
    assert len(hits) == 1, (fragment, hits)
    return hits[0]


L_STOP = _line_of(_MAIN, "if (delta_x <= xtol)")
L_CURV = _line_of(_UPD, "valid = rho_inv.abs()")


class Observer:
    def __init__(self):
        self.t, self.f, self.dx, self.curv = [], [], [], []

    def _local(self, frame, event, arg):
        if event != "line":
            return self._local
        loc = frame.f_locals
        if frame.f_code is _MAIN.__code__ and frame.f_lineno == L_STOP:
            self.t.append(float(loc["t"]))
            self.f.append(float(loc["fval"].double()))
            self.dx.append(float(loc["delta_x"].double()))
        elif frame.f_code is _UPD.__code__ and frame.f_lineno == L_CURV:
            self.curv.append((len(self.f), loc["rho_inv"].double().reshape(-1).tolist()))
        return self._local

    def __call__(self, frame, event, arg):
        return self._local if frame.f_code in (_MAIN.__code__, _UPD.__code__) else None


def run_reference(inputs, spec, dtype):
    x, w, z0 = (t.to(dtype) for t in inputs)
    obs, out = Observer(), io.StringIO()
    verbose = 2 if spec["kwargs"]["maxiter"] > 0 else 0
    with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(out):
        warnings.simplefilter("always")
        sys.settrace(obs)
        try:
            z = ref_solve(lambda z: 0.5 * (z @ w.T - x).pow(2).sum(), z0, alpha=spec["alpha"], verbose=verbose,
                          **spec["kwargs"])
        finally:
            sys.settrace(None)
    return z, obs, out.getvalue(), [str(c.message) for c in caught]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return float("inf")
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def verdicts(curv):
    return [[abs(v) > irbfgs_model.CURV_MIN for v in row] for _, row in curv]


def run_case(name, spec):
    t0 = time.time()
    x, w, z0 = case_inputs(spec)
    kw = dict(spec["kwargs"])
    xtol = kw.get("xtol", 1e-5)
    z32, o32, text, msgs = run_reference((x, w, z0), spec, torch.float32)
    z64, o64, _, msgs64 = run_reference((x, w, z0), spec, torch.float64)
    if msgs or msgs64:
        raise SystemExit("case %s refused: the reference warned %r" % (name, msgs + msgs64))
    # (a) no decision that rounding could flip
    for obs in (o32, o64):
        for it, row in obs.curv:
            for ys in row:
                if not (abs(ys) >= 10 * irbfgs_model.CURV_MIN or abs(ys) <= irbfgs_model.CURV_MIN / 10):
                    raise SystemExit("case %s refused: |y.s| = %r at iteration %d is within 10x of 1e-10" % (name, ys, it))
        for i, dx in enumerate(obs.dx):
            if xtol > 0 and abs(dx - xtol) < 0.01 * xtol:
                raise SystemExit("case %s refused: |dx| %r within 1%% of xtol at iteration %d" % (name, dx, i + 1))
    if verdicts(o32.curv) != verdicts(o64.curv) or len(o32.f) != len(o64.f):
        raise SystemExit("case %s refused: the float32 and float64 runs take different verdicts" % name)
    # the restatement is the reference
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m32, i32 = irbfgs_model.iterative_ridge_bfgs(w, x, z0, alpha=spec["alpha"], **kw)
        m64, i64 = irbfgs_model.iterative_ridge_bfgs(w, x, z0, alpha=spec["alpha"], dtype=torch.float64, **kw)
    if not torch.equal(m32, z32) or i32["curvature"] != o32.curv or i32["t"] != o32.t:
        raise SystemExit("case %s: the float32 model is not the reference bit for bit (max|dz| = %g)"
                         % (name, float((m32 - z32).abs().max())))
    if float((m64 - z64).abs().max()) > 1e-7:
        raise SystemExit("case %s: the float64 model is %g from the reference" % (name, float((m64 - z64).abs().max())))
    irbfgs_model.assert_robust(i32)
    irbfgs_model.assert_robust(i64)
    # (b) how far another correct float32 implementation moves the result
    f_ref = o32.f[-1] if o32.f else i32["f0"]
    spread = dict(z=0.0, f=0.0, t=0.0, objective=0.0, delta=0.0)
    for seed in ORDER_SEEDS:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            zm, im = irbfgs_model.iterative_ridge_bfgs(w, x, z0, alpha=spec["alpha"], order_seed=seed, **kw)
        same = im["invalid_rows"] == i32["invalid_rows"] and im["lu"] == i32["lu"]
        f_m = im["objective"][-1] if im["objective"] else im["f0"]
        spread["z"] = max(spread["z"], float((zm - z32).abs().max()) if same else float("inf"))
        spread["f"] = max(spread["f"], abs(f_m - f_ref) / abs(f_ref))
        spread["t"] = max(spread["t"], rel(im["t"], o32.t))
        spread["objective"] = max(spread["objective"], rel(im["objective"], o32.f))
        spread["delta"] = max(spread["delta"], rel(im["delta_x"], o32.dx))
    compare = spec["compare"]
    if compare == "z" and not spread["z"] <= SPREAD_Z_CAP:
        raise SystemExit("case %s refused for code comparison: spread_z = %.3g" % (name, spread["z"]))
    if compare == "f" and not spread["f"] <= SPREAD_F_CAP:
        raise SystemExit("case %s refused for objective comparison: spread_f = %.3g" % (name, spread["f"]))
    gap = float((z32.double() - z64).abs().max())
    rec = {"z32": z32.numpy(), "z64": z64.numpy(), "f0": np.float64(i64["f0"]),
           "t32": np.array(o32.t), "f32": np.array(o32.f), "dx32": np.array(o32.dx),
           "t64": np.array(o64.t), "f64": np.array(o64.f), "dx64": np.array(o64.dx),
           "ls32": np.array(i32["ls_iters"], dtype=np.int64),
           "invalid_rows": np.array(i32["invalid_rows"], dtype=np.int64),
           "curv32": np.array([v for _, row in o32.curv for v in row], dtype=np.float64),
           "warnings": np.array("\n".join(msgs)), "stdout": np.array(text),
           "spread_z": np.float64(spread["z"]), "spread_f": np.float64(spread["f"]), "spread_t": np.float64(spread["t"]),
           "spread_objective": np.float64(spread["objective"]), "spread_delta": np.float64(spread["delta"]),
           "gap_z": np.float64(gap)}
    print("%-16s iters=%d invalid=%s f=%.6e spread_z=%.2e spread_f=%.2e spread_t=%.2e gap=%.2e  %.1fs" %
          (name, len(o32.f), i32["invalid_rows"], f_ref, spread["z"], spread["f"], spread["t"], gap, time.time() - t0))
    return rec


def run_nonfinite(name, entry):
    spec = entry["case"]
    z32, o32, _, msgs = run_reference(poisoned_inputs(entry), spec, torch.float32)
    print("%-16s iters=%d warnings=%r nan=%d inf=%d" % (name, len(o32.f), msgs, int(torch.isnan(z32).sum()),
                                                         int(torch.isinf(z32).sum())))
    return {"z32": z32.numpy(), "iterations": np.int64(len(o32.f)), "warnings": np.array("\n".join(msgs))}


def main():
    arrays = {}
    only = sys.argv[1:]
    for name, spec in CASES.items():
        if only and name not in only:
            continue
        for key, val in run_case(name, spec).items():
            arrays["%s/%s" % (name, key)] = val
    for name, entry in NONFINITE.items():
        if only and name not in only:
            continue
        for key, val in run_nonfinite(name, entry).items():
            arrays["%s/%s" % (name, key)] = val
    if only:
        return
    path = os.path.join(HERE, "irbfgs_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
