#!/usr/bin/env python3
"""Generate tests/golden/ista_nl_cases.npz by running the REAL reference's ``ista_nl`` (rfeinman/pytorch-lasso,
lasso/nonlinear/ista.py) on decoders nn.Sequential(nn.Linear(k, d), activation), in float32 AND in float64, with
``torch.randn_like`` patched to return the case's ``power_init`` (the reference draws the power iteration's start at
every step; the HIP path and tests/ista_nl_model.py use one start per solve).

Runs only where the reference is mounted (/root/reference); the .npz it writes is data: the inputs are re-creatable
from the seeded recipe of tests/ista_nl_cases.py, the expected outputs are stored.  Same scipy shim as
generate_golden_owlqn.py (the package imports scipy at import time); no reference file is edited or copied.

Each run is observed with sys.settrace: per iteration the sum |z - z_next| at the line that tests it, and what
hessian_2norm returned last.  The float32 run's verbose=2 output is stored as well.  The float64 codes are stored for
shapes of at most 1000 codes only (the fixture's size); the float64 sums and L of every case are.

Every case is CERTIFIED before it is written (the script exits non-zero otherwise -- choose another seed or iteration
count, never another cap):
  (a) every code is finite and some code is non-zero, in both runs;
  (b) no sum |z - z_next| lies within 1 % of the stop budget, and both runs make the same number of iterations;
  (c) spread_z = the maximum over the order_seeds x link64 in {0, 1} of max|z_model - z_ref32| (tests/ista_nl_model.py:
      "another correct float32 implementation") is at most 2.5e-3; spread_L likewise for the relative L of the last step.
The model in the reference's order must equal the float32 run bit for bit for the identity and to 4 x spread_z
otherwise, and the float64 run to 1e-12.

Usage:  python tests/golden/generate_golden_ista_nl.py [case ...]
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
import lasso.nonlinear  # noqa: E402,F401

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ista_nl_model as model  # noqa: E402
from ista_nl_cases import CASES, ORDER_SEEDS, SPREAD_Z_CAP, case_inputs  # noqa: E402

ref_mod = sys.modules["lasso.nonlinear.ista"]
_MAIN = ref_mod.ista_nl
_POWER = ref_mod.hessian_2norm
Z64_CAP = 1000                        # the float64 codes are stored for shapes of at most this many (the fixture's size)
_MODULES = dict(identity=torch.nn.Identity, sigmoid=torch.nn.Sigmoid, tanh=torch.nn.Tanh, relu=torch.nn.ReLU)


def _line_of(fn, fragment):
    src, first = inspect.getsourcelines(fn)
    hits = [first + i for i, s in enumerate(src) if fragment in s]
    assert len(hits) == 1, (fragment, hits)
    return hits[0]


L_STOP = _line_of(_MAIN, "if (z - z_next).abs().sum() <= tol")


class Observer:
    def __init__(self):
        self.deltas, self.L = [], None

    def _local(self, frame, event, arg):
        if event == "line" and frame.f_code is _MAIN.__code__ and frame.f_lineno == L_STOP:
            loc = frame.f_locals
            self.deltas.append(float((loc["z"] - loc["z_next"]).abs().sum()))
        elif event == "return" and frame.f_code is _POWER.__code__ and arg is not None:
            self.L = arg.detach().clone()
        return self._local

    def __call__(self, frame, event, arg):
        return self._local if frame.f_code in (_MAIN.__code__, _POWER.__code__) else None


def run_reference(spec, dtype):
    x, w, b, z0, u0 = case_inputs(spec)
    n, d, k = spec["n"], spec["d"], spec["k"]
    lin = torch.nn.Linear(k, d, bias=b is not None)
    with torch.no_grad():
        lin.weight.copy_(w)
        if b is not None:
            lin.bias.copy_(b)
    decoder = torch.nn.Sequential(lin, _MODULES[spec["activation"]]()).to(dtype)
    obs, out = Observer(), io.StringIO()
    drawn = torch.randn_like
    torch.randn_like = lambda t, **kw: u0.to(t.dtype)
    try:
        with contextlib.redirect_stdout(out):
            sys.settrace(obs)
            try:
                z = _MAIN(x.to(dtype), z0.to(dtype), decoder, alpha=spec["alpha"], verbose=2, **spec["kwargs"])
            finally:
                sys.settrace(None)
    finally:
        torch.randn_like = drawn
    return z, obs, out.getvalue()


def run_case(name, spec):
    t0 = time.time()
    x, w, b, z0, u0 = case_inputs(spec)
    kw = spec["kwargs"]
    budget = z0.numel() * kw["tol"]
    z32, o32, text = run_reference(spec, torch.float32)
    z64, o64, _ = run_reference(spec, torch.float64)
    # (a), (b)
    for z, obs in ((z32, o32), (z64, o64)):
        if not torch.isfinite(z).all() or not (z != 0).any():
            raise SystemExit("case %s refused: a code is not finite, or every code is zero" % name)
        for i, dl in enumerate(obs.deltas):
            if budget > 0 and abs(dl - budget) < 0.01 * budget:
                raise SystemExit("case %s refused: sum |dz| %r within 1%% of the budget at iteration %d" % (name, dl, i + 1))
    if len(o32.deltas) != len(o64.deltas):
        raise SystemExit("case %s refused: the float32 and float64 runs stop at %d and %d" % (name, len(o32.deltas), len(o64.deltas)))
    stopped = budget > 0 and o32.deltas[-1] <= budget
    if kw["tol"] > 0 and not (stopped and len(o32.deltas) < kw["maxiter"]):
        raise SystemExit("case %s refused: a stop case whose rule does not fire mid-run" % name)
    run = lambda **more: model.ista_nl(x, z0, w, b, spec["activation"], alpha=spec["alpha"], power_init=u0, **dict(kw, **more))
    # (c) how far another correct float32 implementation moves the result
    spread_z, spread_l = 0.0, 0.0
    for seed in ORDER_SEEDS:
        for link64 in (False, True):
            zm, im = run(order_seed=seed, link64=link64)
            same = im["iterations"] == len(o32.deltas)
            spread_z = max(spread_z, float((zm - z32).abs().max()) if same else float("inf"))
            if o32.L is not None:
                spread_l = max(spread_l, float(((im["L"] - o32.L).abs() / o32.L.abs()).max()))
    if not spread_z <= SPREAD_Z_CAP:
        raise SystemExit("case %s refused for code comparison: spread_z = %.3g" % (name, spread_z))
    # the restatement is the reference
    m32, i32 = run()
    m64, i64 = run(dtype=torch.float64)
    err32, err64 = float((m32 - z32).abs().max()), float((m64 - z64).abs().max())
    if i32["iterations"] != len(o32.deltas) or i64["iterations"] != len(o64.deltas):
        raise SystemExit("case %s: the model makes another number of iterations" % name)
    if (spec["activation"] == "identity" and not torch.equal(m32, z32)) or err32 > 4.0 * spread_z:
        raise SystemExit("case %s: the float32 model is %g from the reference (spread_z %g)" % (name, err32, spread_z))
    if err64 > 1e-12:
        raise SystemExit("case %s: the float64 model is %g from the reference" % (name, err64))
    gap = float((z32.double() - z64).abs().max())
    rec = {"z32": z32.numpy(), "deltas32": np.array(o32.deltas), "deltas64": np.array(o64.deltas),
           "stopped": np.int64(stopped), "stdout": np.array(text), "spread_z": np.float64(spread_z),
           "spread_L": np.float64(spread_l), "gap_z": np.float64(gap)}
    if z64.numel() <= Z64_CAP:
        rec["z64"] = z64.numpy()
    if o32.L is not None:
        rec["L32"], rec["L64"] = o32.L.numpy(), o64.L.numpy()
    print("%-24s iters=%3d stopped=%d nnz=%5d spread_z=%.2e spread_L=%.2e model32=%.2e model64=%.2e gap=%.2e  %.1fs" %
          (name, len(o32.deltas), stopped, int((z32 != 0).sum()), spread_z, spread_l, err32, err64, gap, time.time() - t0),
          flush=True)
    return rec


def main():
    arrays = {}
    only = sys.argv[1:]
    for name, spec in CASES.items():
        if only and name not in only:
            continue
        for key, val in run_case(name, spec).items():
            arrays["%s/%s" % (name, key)] = val
    if only:
        return
    path = os.path.join(HERE, "ista_nl_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
