#!/usr/bin/env python3
"""Generate tests/golden/gpsr_conv_cases.npz by running the REAL reference's GPSR-Basic
(rfeinman/pytorch-lasso, lasso/linear/solvers/gpsr.py: gpsr_basic(y, A, tau, AT, x0, ...)) in float32 with the two
closures of a convolutional dictionary,

    A  = lambda v: F.conv_transpose2d(v, W, stride=s, padding=p)
    AT = lambda v: F.conv2d(v, W, stride=s, padding=p)

Runs only where the reference is mounted (/root/reference); the .npz it writes is data: the inputs are re-creatable
from the seeded recipe of tests/gpsr_conv_cases.py, the expected outputs are stored.  Same scipy shim as the other
generators; no reference file is edited or copied.

As in generate_golden_gpsr.py the run is observed with sys.settrace (the unrounded float32 f, lambd, criterion and
(f_new, f + mu g, f) of every line-search decision) and its verbose=2 prints are parsed and cross-checked.

The host model (tests/gpsr_conv_model.py) must REPRODUCE the reference: equal iteration and trial counts, and z
torch.equal -- or, where this CPU's convolutions do not allow that, within the model's own float32-float64 gap.

Every case is CERTIFIED before it is written: at each line-search decision |f_new - bound| >= 1e-4 |f|; at each
iteration the criterion is at least 1 % away from tol (criterion 0: the integer count differs from tol); and the
model's float32 and float64 runs have identical trial lists.  A case that fails is refused (non-zero exit): choose
another seed, never a looser rule.

Usage:  python tests/golden/generate_golden_gpsr_conv.py
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
from lasso.linear.solvers.gpsr import gpsr_basic  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gpsr_conv_model  # noqa: E402
from gpsr_conv_cases import CASES, case_inputs, rows_of  # noqa: E402

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


def refuse(name, why):
    raise SystemExit("case %s refused: %s" % (name, why))


def run_case(name, spec):
    x, w, z0 = case_inputs(spec)
    kw = dict(spec["kwargs"])
    s, p, tau = spec["stride"], spec["padding"], spec["tau"]
    A, AT = gpsr_conv_model.closures(w, s, p)
    obs = Observer()
    out = io.StringIO()
    t0 = time.time()
    with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(out):
        warnings.simplefilter("always")
        sys.settrace(obs)
        try:
            z = gpsr_basic(x, A, tau, AT, x0=z0, verbose=2, **kw)
        finally:
            sys.settrace(None)
    text = out.getvalue()
    msgs = [str(c.message) for c in caught]
    n_iter = len(obs.f)
    db_iters = len(re.findall(r"^ Iter = ", text, re.M))
    its = IT_RE.findall(text)
    assert len(its) == n_iter, (name, len(its), n_iter)
    for (i, fo, lo, _), f, lam in zip(its, obs.f, obs.lam):
        assert abs(float(fo) - f) <= 6e-6 * abs(f) and abs(float(lo) - lam) <= 6e-3 * abs(lam), (name, i, fo, f, lo, lam)
    assert text.count("line-search reducing") == sum(obs.trials) - n_iter, name
    # ---- certification ----
    margin = min([abs(fn - bound) / abs(f) for fn, bound, f in obs.decisions] or [float("inf")])
    if not margin >= 1e-4:
        refuse(name, "a line-search decision is within %.2e |f| of flipping" % margin)
    main_crit = kw.get("stop_criterion", 3)
    for i, (c, tol) in enumerate(zip(obs.crit, obs.tol)):
        crit_id = main_crit if tol == kw.get("tol", 1e-2) else 3
        near = (c == tol) if (crit_id == 0 and np.isfinite(c)) else (np.isfinite(c) and abs(c - tol) < 0.01 * abs(tol))
        if near:
            refuse(name, "criterion %r within 1%% of tol %r at iteration %d" % (c, tol, i + 1))
    # ---- the model reproduces the reference; its float32 and float64 runs take the same trials ----
    with warnings.catch_warnings(record=True) as caught_m:
        warnings.simplefilter("always")
        z32, i32 = gpsr_conv_model.gpsr_conv2d(x, w, tau, z0=z0, stride=s, padding=p, return_info=True, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z64, i64 = gpsr_conv_model.gpsr_conv2d(x.double(), w.double(), tau, z0=None if z0 is None else z0.double(),
                                               stride=s, padding=p, return_info=True, **kw)
    if i32["iterations"] != n_iter + db_iters or i32["trials"] != obs.trials:
        refuse(name, "the model takes %d iterations / trials %s, the reference %d / %s"
               % (i32["iterations"], i32["trials"], n_iter + db_iters, obs.trials))
    if i64["trials"] != obs.trials or i64["iterations"] != i32["iterations"]:
        refuse(name, "the float64 run takes trials %s, the float32 run %s" % (i64["trials"], obs.trials))
    if sorted(str(c.message) for c in caught_m) != sorted(msgs):
        refuse(name, "the model warns %r, the reference %r" % ([str(c.message) for c in caught_m], msgs))
    gap = float((z32.double() - z64).abs().max())
    exact = torch.equal(z32, z)
    dev = float((z32 - z).abs().max())
    if not exact and dev > gap:
        refuse(name, "the model is %.3g from the reference, its own float32-float64 gap is %.3g" % (dev, gap))
    zr = rows_of(z).numpy()
    rec = {"n_iter": np.int64(n_iter), "db_iters": np.int64(db_iters),
           "objective": np.array(obs.f), "lam": np.array(obs.lam),
           "trials": np.array(obs.trials, dtype=np.int64), "criterion": np.array(obs.crit),
           "warnings": np.array("\n".join(msgs)), "stdout": np.array(text if spec.get("keep_stdout") else ""),
           "model_gap": np.float64(gap), "decision_margin": np.float64(margin),
           "z_sum": np.float64(z.double().sum().item()), "z_abssum": np.float64(z.double().abs().sum().item()),
           "z_nnz": np.int64((z != 0).sum().item())}
    if zr.nbytes > (32 << 10):                   # a sample of rows plus sums
        rows = np.unique(np.concatenate([np.arange(0, zr.shape[0], max(1, zr.shape[0] // 24)), [zr.shape[0] - 1]]))
    else:
        rows = np.arange(zr.shape[0])
    rec["z_rows"], rec["z"] = rows, zr[rows]
    print("%-8s n_iter=%3d+%d trials=%s f=%.6e nnz=%d model %s (dev %.2g, f32-f64 gap %.2g) margin %.2g  %.1fs  warnings=%r" %
          (name, n_iter, db_iters, obs.trials, obs.f[-1] if obs.f else float("nan"), rec["z_nnz"],
           "equal" if exact else "within gap", dev, gap, margin, time.time() - t0, msgs))
    if main_crit != 3:
        print("         criterion:", ["%.4g" % c for c in obs.crit])
    return rec


def main():
    arrays = {}
    for name, spec in CASES.items():
        for key, val in run_case(name, spec).items():
            arrays["%s/%s" % (name, key)] = val
    path = os.path.join(HERE, "gpsr_conv_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
