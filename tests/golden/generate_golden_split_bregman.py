#!/usr/bin/env python3
"""Generate tests/golden/split_bregman_cases.npz by running the REAL reference's Split Bregman solver
(rfeinman/pytorch-lasso, lasso/linear/solvers/split_bregman.py), in float32 AND in float64.

Runs only where the reference is mounted (/root/reference); the .npz it writes is data: the inputs are re-creatable
from the seeded recipes of tests/recipes.py, the expected outputs are stored.  Same scipy shim as
generate_golden_own.py; no reference file is edited or copied.

Each run is observed with sys.settrace: the value of ``update`` after every outer iteration (at the line that tests
``verbose``, the first one behind the norm).

Every case is CERTIFIED before it is written (the script exits non-zero otherwise -- choose another seed or tol):
  (a) every recorded update of both runs is at least 1 % away from tol;
  (b) the model in the reference's order (tests/split_bregman_model.py, every knob off) equals the float32 run bit for
      bit -- or else the difference is reported and stored (model_gap) -- and the float64 run to 1e-9;
  (c) spread_z = the maximum over the model's variants ("another correct float32 implementation": row-major state, a
      double Hinv rounded once, permuted summation orders) of max|x_model - x_ref32|, spread_update likewise for the
      relative update sequence (infinite if a variant runs another number of iterations); both are stored;
  (d) a case needs spread_z <= 2.5e-3 and a finite spread_update.

Usage:  python tests/golden/generate_golden_split_bregman.py
"""
import inspect
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
import split_bregman_model as model  # noqa: E402
from split_bregman_cases import CASES, ORDER_SEEDS, SPREAD_Z_CAP, case_inputs  # noqa: E402

ref_mod = sys.modules["lasso.linear.solvers.split_bregman"]
ref_solve = ref_mod.split_bregman
_MAIN = inspect.unwrap(ref_solve)


def _line_of(fn, fragment):
    src, first = inspect.getsourcelines(fn)
    hits = [first + i for i, s in enumerate(src) if fragment in s]
    assert len(hits) == 1, (fragment, hits)
    return hits[0]


L_AFTER_NORM = _line_of(_MAIN, "if verbose:")


class Observer:
    def __init__(self):
        self.update = []

    def _local(self, frame, event, arg):
        if event == "line" and frame.f_code is _MAIN.__code__ and frame.f_lineno == L_AFTER_NORM:
            self.update.append(float(frame.f_locals["update"].double()))
        return self._local

    def __call__(self, frame, event, arg):
        return self._local if frame.f_code is _MAIN.__code__ else None


def run_reference(spec, dtype):
    A, y, x0 = (None if t is None else t.to(dtype) for t in case_inputs(spec))
    obs = Observer()
    sys.settrace(obs)
    try:
        x, itn = ref_solve(A, y, x0, alpha=spec["alpha"], **spec["kwargs"])
    finally:
        sys.settrace(None)
    return x, int(itn), obs.update


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return float("inf")
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def run_case(name, spec):
    t0 = time.time()
    A, y, x0 = case_inputs(spec)
    kw = dict(spec["kwargs"])
    tol = kw.get("tol", 1e-10)
    maxiter = kw.get("maxiter", 20)
    x32, itn32, u32 = run_reference(spec, torch.float32)
    x64, itn64, u64 = run_reference(spec, torch.float64)
    for u in u32 + u64:                                                         # (a)
        if abs(u - tol) < 0.01 * tol:
            raise SystemExit("case %s refused: update %r within 1%% of tol" % (name, u))
    if itn32 != itn64 or len(u32) != len(u64):
        raise SystemExit("case %s refused: the float32 and float64 runs stop at %d and %d" % (name, itn32, itn64))
    m32, mi32, minfo32 = model.split_bregman(A, y, x0, alpha=spec["alpha"], **kw)        # (b)
    m64, mi64, minfo64 = model.split_bregman(A, y, x0, alpha=spec["alpha"], dtype=torch.float64, **kw)
    model_gap = float((m32 - x32).abs().max())
    if not torch.equal(m32, x32) or minfo32["update"] != u32:
        print("case %s: the float32 model is NOT the reference bit for bit (max|dx| = %g)" % (name, model_gap))
    if mi32 != itn32 or mi64 != itn64 or float((m64 - x64).abs().max()) > 1e-9:
        raise SystemExit("case %s: the model disagrees with the reference (itn %d / %d, float64 gap %g)"
                         % (name, mi32, itn32, float((m64 - x64).abs().max())))
    spread_z, spread_u = 0.0, 0.0                                               # (c)
    for knobs in model.variants(ORDER_SEEDS):
        xm, im, infom = model.split_bregman(A, y, x0, alpha=spec["alpha"], **knobs, **kw)
        spread_z = max(spread_z, float((xm - x32).abs().max()))
        spread_u = max(spread_u, rel(infom["update"], u32) if im == itn32 else float("inf"))
    if not (spread_z <= SPREAD_Z_CAP and np.isfinite(spread_u)):                # (d)
        raise SystemExit("case %s refused: spread_z = %.3g, spread_update = %.3g" % (name, spread_z, spread_u))
    gap = float((x32.double() - x64).abs().max())
    stopped = len(u32) < maxiter
    rec = {"x32": x32.numpy(), "x64": x64.numpy(), "itn": np.int64(itn32), "iterations": np.int64(len(u32)),
           "stopped": np.bool_(stopped), "update32": np.array(u32), "update64": np.array(u64),
           "spread_z": np.float64(spread_z), "spread_update": np.float64(spread_u), "gap_z": np.float64(gap),
           "model_gap": np.float64(model_gap)}
    print("%-16s itn=%d iterations=%d stopped=%d max|x|=%.3g update[-1]=%.3e spread_z=%.2e spread_update=%.2e gap=%.2e "
          "model_gap=%.1e  %.1fs" % (name, itn32, len(u32), stopped, float(x32.abs().max()), u32[-1], spread_z, spread_u, gap,
                                     model_gap, time.time() - t0))
    return rec


def main():
    arrays = {}
    for name, spec in CASES.items():
        for key, val in run_case(name, spec).items():
            arrays["%s/%s" % (name, key)] = val
    path = os.path.join(HERE, "split_bregman_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
