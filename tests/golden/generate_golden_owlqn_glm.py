#!/usr/bin/env python3
"""Generate tests/golden/owlqn_glm_cases.npz by running the REAL reference's OWL-QN solver (rfeinman/pytorch-lasso,
lasso/nonlinear/owlqn.py) on fun(z) = F.binary_cross_entropy_with_logits(z @ W.T, x, reduction='sum'), in float32 AND in
float64.

Everything that observes and certifies a run is generate_golden_owlqn.py's, imported: the scipy shim, the sys.settrace
Observer (per iteration the unrounded t, ls_iters, f and |dx|; (f_new, bound, f) at every backtracking decision; y.s at
every memory update) and rule (a).  Runs only where the reference is mounted; the .npz it writes is data: the inputs
are re-creatable from the seeded recipe of tests/owlqn_glm_cases.py, the expected outputs are stored.

Every case is CERTIFIED before it is written (the script exits non-zero otherwise -- choose another seed or iteration
count, never another cap):
  (a) every backtracking decision is at least 1e-4 |f| from its bound, every y.s a factor 10 from 1e-10 and every |dx|
      at least 1 % from xtol, in both runs;
  (b) spread_z = the maximum over 8 order_seeds x accurate_f in {0, 1} x link64 in {0, 1} of max|z_model - z_ref32|
      (tests/owlqn_glm_model.py: "another correct float32 implementation" -- link64 evaluates the link in float64 and
      rounds once, standing in for a device whose expf / log1pf differ from torch's by ulps), spread_f likewise for the
      relative final objective, and the same for the per-iteration t, objective and |dx|; all are stored;
  (c) a case compared by its codes needs spread_z <= 2.5e-3;
  (d) a case compared by its objective needs spread_f <= 1e-4.
The model in the reference's order must equal the float32 run bit for bit and the float64 run to 1e-7.

Usage:  python tests/golden/generate_golden_owlqn_glm.py [case ...]
"""
import contextlib
import io
import os
import sys
import time
import warnings

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate_golden_owlqn as base  # noqa: E402  (mounts the reference, installs the shim)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import owlqn_glm_model as model  # noqa: E402
from owlqn_glm_cases import CASES, ORDER_SEEDS, SPREAD_F_CAP, SPREAD_Z_CAP, case_inputs  # noqa: E402


def run_reference(spec, dtype):
    x, w, z0 = (t.to(dtype) for t in case_inputs(spec))
    obs, out = base.Observer(), io.StringIO()
    verbose = 2 if spec["kwargs"]["max_iter"] > 0 else 0
    with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(out):
        warnings.simplefilter("always")
        sys.settrace(obs)
        try:
            z = base.ref_solve(lambda z: F.binary_cross_entropy_with_logits(z @ w.T, x, reduction='sum'), z0,
                               alpha=spec["alpha"], verbose=verbose, **spec["kwargs"])
        finally:
            sys.settrace(None)
    return z, obs, out.getvalue(), [str(c.message) for c in caught]


def run_case(name, spec):
    t0 = time.time()
    x, w, z0 = case_inputs(spec)
    kw = dict(spec["kwargs"])
    xtol = kw.get("xtol", 1e-5)
    z32, o32, text, msgs = run_reference(spec, torch.float32)
    z64, o64, _, _ = run_reference(spec, torch.float64)
    # (a) no decision that rounding could flip
    for obs in (o32, o64):
        for fn, bound, f in obs.decisions:
            if not abs(fn - bound) >= 1e-4 * abs(f):
                raise SystemExit("case %s refused: backtracking decision too close (%r, %r, %r)" % (name, fn, bound, f))
        for it, ys in obs.curv:
            if not (ys >= 10 * model.CURV_MIN or ys <= model.CURV_MIN / 10):
                raise SystemExit("case %s refused: y.s = %r at iteration %d is within 10x of 1e-10" % (name, ys, it))
        for i, dx in enumerate(obs.dx):
            if xtol > 0 and abs(dx - xtol) < 0.01 * xtol:
                raise SystemExit("case %s refused: |dx| %r within 1%% of xtol at iteration %d" % (name, dx, i + 1))
    if [ys > model.CURV_MIN for _, ys in o32.curv] != [ys > model.CURV_MIN for _, ys in o64.curv]:
        raise SystemExit("case %s refused: the float32 and float64 runs keep different pairs" % name)
    # the restatement is the reference
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m32, i32 = model.owlqn(w, x, z0, alpha=spec["alpha"], **kw)
        m64, i64 = model.owlqn(w, x, z0, alpha=spec["alpha"], dtype=torch.float64, **kw)
    if not torch.equal(m32, z32) or i32["ls_iters"] != o32.ls or i32["curvature"] != o32.curv:
        raise SystemExit("case %s: the float32 model is not the reference bit for bit (max|dz| = %g)"
                         % (name, float((m32 - z32).abs().max())))
    if float((m64 - z64).abs().max()) > 1e-7:
        raise SystemExit("case %s: the float64 model is %g from the reference" % (name, float((m64 - z64).abs().max())))
    model.assert_robust(i32)
    model.assert_robust(i64)
    # (b) how far another correct float32 implementation moves the result
    f_ref = o32.f[-1] if o32.f else i32["f0"]
    spread = dict(z=0.0, f=0.0, t=0.0, objective=0.0, delta=0.0)
    for seed in ORDER_SEEDS:
        for acc in (False, True):
            for link64 in (False, True):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    zm, im = model.owlqn(w, x, z0, alpha=spec["alpha"], accurate_f=acc, order_seed=seed, link64=link64, **kw)
                same = (im["ls_iters"] == o32.ls or kw["line_search"] == "brent") and im["skipped"] == i32["skipped"]
                f_m = im["objective"][-1] if im["objective"] else im["f0"]
                spread["z"] = max(spread["z"], float((zm - z32).abs().max()) if same else float("inf"))
                spread["f"] = max(spread["f"], abs(f_m - f_ref) / abs(f_ref))
                spread["t"] = max(spread["t"], base.rel(im["t"], o32.t))
                spread["objective"] = max(spread["objective"], base.rel(im["objective"], o32.f))
                spread["delta"] = max(spread["delta"], base.rel(im["delta_x"], o32.dx))
    compare = spec["compare"]
    if compare == "z" and not spread["z"] <= SPREAD_Z_CAP:
        raise SystemExit("case %s refused for code comparison: spread_z = %.3g" % (name, spread["z"]))
    if compare == "f" and not spread["f"] <= SPREAD_F_CAP:
        raise SystemExit("case %s refused for objective comparison: spread_f = %.3g" % (name, spread["f"]))
    gap = float((z32.double() - z64).abs().max())
    rec = {"z32": z32.numpy(), "z64": z64.numpy(), "f0": np.float64(i64["f0"]),
           "t32": np.array(o32.t), "ls32": np.array(o32.ls, dtype=np.int64), "f32": np.array(o32.f), "dx32": np.array(o32.dx),
           "t64": np.array(o64.t), "ls64": np.array(o64.ls, dtype=np.int64), "f64": np.array(o64.f), "dx64": np.array(o64.dx),
           "decisions32": np.array(o32.decisions, dtype=np.float64).reshape(-1, 3),
           "curvature32": np.array(o32.curv, dtype=np.float64).reshape(-1, 2),
           "pairs": np.array(i32["pairs"], dtype=np.int64), "skipped": np.array(i32["skipped"], dtype=np.int64),
           "hdiag32": np.array(i32["H_diag"]),
           "warnings": np.array("\n".join(msgs)), "stdout": np.array(text),
           "spread_z": np.float64(spread["z"]), "spread_f": np.float64(spread["f"]), "spread_t": np.float64(spread["t"]),
           "spread_objective": np.float64(spread["objective"]), "spread_delta": np.float64(spread["delta"]),
           "gap_z": np.float64(gap)}
    print("%-14s iters=%d ls=%s pairs=%s skipped=%s f=%.6e spread_z=%.2e spread_f=%.2e gap=%.2e  %.1fs  warnings=%d" %
          (name, len(o32.f), o32.ls, i32["pairs"], [int(s) for s in i32["skipped"]], f_ref, spread["z"], spread["f"], gap,
           time.time() - t0, len(msgs)), flush=True)
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
    path = os.path.join(HERE, "owlqn_glm_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
