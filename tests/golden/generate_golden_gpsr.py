#!/usr/bin/env python3
"""Generate tests/golden/gpsr_cases.npz by running the REAL reference's GPSR-Basic
(rfeinman/pytorch-lasso, lasso/linear/solvers/gpsr.py) through lasso.linear.sparse_encode.

Runs only where the reference is mounted (/root/reference); the .npz it writes is data: the inputs are
re-creatable from the seeded recipes of tests/recipes.py, the expected outputs are stored.  Same scipy shim as
generate_golden.py; no reference file is edited or copied.

Per case the reference runs with verbose=2 and its stdout is captured and parsed (objective, lambda, criterion per
iteration, the trial count from the 'line-search reducing' lines, the debias steps from their ' Iter =' lines).
The prints carry 6 and 3 significant digits, so the same run is also observed with sys.settrace: the unrounded float32 values of f, lambd and criterion at the
lines that print them, and (f_new, f + mu * g, f) at every line-search decision.  Those are what the fixture
stores; the parsed values are cross-checked against them.

Every case is CERTIFIED before it is written: at each line-search decision |f_new - bound| >= 1e-4 |f|, and at
each iteration the criterion is at least 1 % away from tol (criterion 0: the integer count differs from tol), so
no rounding difference between two correct implementations can flip a branch; and the accepted steps of the host
model (tests/gpsr_model.py) run in float32 and in float64 agree to 2.5e-6, a quarter of the 1e-5 the tests compare
lambda at -- the trace is then not more sensitive to summation order than the bar allows.  A case that fails is refused
(the script exits non-zero) -- choose other arguments.  Every case has an explicit, modest maxiter: the reference
is slow beyond a few dozen iterations on a CPU.

Usage:  python tests/golden/generate_golden_gpsr.py
"""
import contextlib
import inspect
import io
import os
import re
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
from lasso.linear import sparse_encode  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from recipes import recipe_xw  # noqa: E402
from gpsr_cases import CASES, case_inputs  # noqa: E402

ref_mod = sys.modules["lasso.linear.solvers.gpsr"]
_CODE = ref_mod._gpsr_basic.__code__
_SRC, _FIRST = inspect.getsourcelines(ref_mod._gpsr_basic)


def _line_of(fragment):
    hits = [_FIRST + i for i, s in enumerate(_SRC) if fragment in s]
    assert len(hits) == 1, (fragment, hits)
    return hits[0]


L_DECIDE = _line_of("if f_new <= f + mu")
L_COUNT = _line_of("n_iter += 1")
L_STOP = _line_of("if n_iter > miniter and criterion <= tol")


class Observer:
    def __init__(self):
        self.decisions, self.f, self.lam, self.crit, self.tol, self.trials = [], [], [], [], [], []
        self._t = 0

    def _local(self, frame, event, arg):
        if event != "line":
            return self._local
        loc = frame.f_locals
        if frame.f_lineno == L_DECIDE:
            dot = loc["dot"]
            bound = loc["f"] + loc["mu"] * (dot(loc["gradu"], loc["du"]) + dot(loc["gradv"], loc["dv"]))
            self.decisions.append((float(loc["f_new"]), float(bound), float(loc["f"])))
            self._t += 1
        elif frame.f_lineno == L_COUNT:
            self.f.append(float(loc["f"]))
            self.lam.append(float(loc["lambd"]))
            self.trials.append(self._t)
            self._t = 0
        elif frame.f_lineno == L_STOP:
            self.crit.append(float(loc["criterion"]))
            self.tol.append(float(loc["tol"]))
        return self._local

    def __call__(self, frame, event, arg):
        return self._local if frame.f_code is _CODE else None


IT_RE = re.compile(r"It =\s*(\d+), obj = ([-+.\deEna]+), lambda = ([-+.\deEna]+), nz = (\d+)")
CRIT_RE = re.compile(r"^    \S.* = ([-+.\deEinfa]+) \(target = ([-+.\deE]+)\)", re.M)


def run_case(name, spec):
    x, w, z0 = case_inputs(spec)
    kw = dict(spec["kwargs"])
    obs = Observer()
    out = io.StringIO()
    t0 = time.time()
    with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(out):
        warnings.simplefilter("always")
        sys.settrace(obs)
        try:
            z = sparse_encode(x, w, alpha=spec["alpha"], z0=z0, algorithm="gpsr", verbose=2, **kw)
        finally:
            sys.settrace(None)
    text = out.getvalue()
    msgs = [str(c.message) for c in caught]
    n_iter = len(obs.f)
    # the prints agree with the observed values to their printed precision
    its = IT_RE.findall(text)
    assert len(its) == n_iter, (name, len(its), n_iter)
    for (i, fo, lo, _), f, lam in zip(its, obs.f, obs.lam):
        assert abs(float(fo) - f) <= 6e-6 * abs(f) and abs(float(lo) - lam) <= 6e-3 * abs(lam), (name, i, fo, f, lo, lam)
    assert text.count("line-search reducing") == sum(obs.trials) - n_iter, name
    crits = CRIT_RE.findall(text)
    assert len(crits) == n_iter, (name, len(crits), n_iter)
    # certification
    for fn, bound, f in obs.decisions:
        if not abs(fn - bound) >= 1e-4 * abs(f):
            raise SystemExit("case %s refused: line-search decision too close (%r, %r, %r)" % (name, fn, bound, f))
    main_crit = spec["kwargs"].get("stop_criterion", 3)
    for i, (c, tol) in enumerate(zip(obs.crit, obs.tol)):
        crit_id = main_crit if tol == spec["kwargs"].get("tol", 1e-2) else 3
        near = (c == tol) if (crit_id == 0 and np.isfinite(c)) else (np.isfinite(c) and abs(c - tol) < 0.01 * abs(tol))
        if near:
            raise SystemExit("case %s refused: criterion %r within 1%% of tol %r at iteration %d" % (name, c, tol, i + 1))
    import gpsr_model
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m32 = gpsr_model.gpsr_basic(x, w, spec["alpha"], x0=z0, return_info=True, **kw)[1]["accepted_lambda"]
        m64 = gpsr_model.gpsr_basic(x.double(), w.double(), spec["alpha"], x0=None if z0 is None else z0.double(),
                                    return_info=True, **kw)[1]["accepted_lambda"]
    if len(m32) != n_iter or len(m64) != n_iter:
        raise SystemExit("case %s refused: the model takes %d / %d iterations, the reference %d" % (name, len(m32), len(m64), n_iter))
    sens = max([abs(a - b) / abs(b) for a, b in zip(m32, m64)] or [0.0])
    if sens > 2.5e-6:
        raise SystemExit("case %s refused: lambda moves by %.2e between float32 and float64" % (name, sens))
    zn = z.numpy()
    rec = {"n_iter": np.int64(n_iter), "db_iters": np.int64(len(re.findall(r"^ Iter = ", text, re.M))),
           "objective": np.array(obs.f), "lam": np.array(obs.lam),
           "trials": np.array(obs.trials, dtype=np.int64), "criterion": np.array(obs.crit),
           "warnings": np.array("\n".join(msgs)), "stdout": np.array(text if spec.get("keep_stdout") else ""),
           "z_sum": np.float64(z.double().sum().item()), "z_abssum": np.float64(z.double().abs().sum().item()),
           "z_nnz": np.int64((z != 0).sum().item())}
    if zn.nbytes > (256 << 10):                  # the large case: slices plus sums (as G2 does)
        rows = np.unique(np.concatenate([np.arange(0, zn.shape[0], max(1, zn.shape[0] // 24)), [zn.shape[0] - 1]]))
        rec["z_rows"], rec["z"] = rows, zn[rows]
    else:
        rec["z_rows"], rec["z"] = np.arange(zn.shape[0]), zn
    print("%-10s n_iter=%3d trials=%s f=%.6e nnz=%d  %.1fs  warnings=%r" %
          (name, n_iter, obs.trials, obs.f[-1] if obs.f else float("nan"), rec["z_nnz"], time.time() - t0, msgs))
    return rec


def main():
    arrays = {}
    for name, spec in CASES.items():
        for key, val in run_case(name, spec).items():
            arrays["%s/%s" % (name, key)] = val
    path = os.path.join(HERE, "gpsr_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
