#!/usr/bin/env python3
"""Generate tests/golden/cd_mod_cases.npz: the reference's coord_descent_mod
(rfeinman/pytorch-lasso, lasso/linear/solvers/coordinate_descent.py:57-139) and the host model of it.

Runs only where the reference is mounted (/root/reference); the .npz it writes is data: the inputs are re-creatable
from the seeded recipe of tests/cd_mod_cases.py, the expected outputs are stored.  Same scipy shim as
generate_golden.py; no reference file is edited or copied.

The reference allocates the code as [n_features, n_components] (:73), so it runs only when n == d.  On those cases
the REAL reference runs in float32 and the host model (tests/cd_mod_model.py, code shaped [n, k]) must equal its z
and gap with torch.equal; the reference's outputs are stored.  On every case -- n != d included -- the model runs in
float32 and in float64 and the fixture stores both results, the per-row sweeps of both, the per-row spread
max|z32 - z64| and a per-row `certified` flag: same sweeps in both, converged in both, and no evaluated gap within
5 % of tol * ||x_row||^2 in either.  On such rows no rounding difference between two correct implementations can flip
the gap's stop decision.  The solver has a second decision per sweep, the check rule of :132 (max|change| / max|z| < tol),
which decides whether the gap is looked at at all; the change is a difference of two float32 values of size <= max|z|,
each good to a few ulp (4 ulp = 5e-7 max|z|), so at tol = 1e-4 the ratio carries a relative error of up to 5e-3 -- runs
of the host model in float32 on two CPUs, and the covariance form of the kernel, do differ by that much and have been
seen to stop a sweep apart on certified rows.  The fixture therefore also stores `decisive`: certified AND, in both
precisions, no sweep at which the ratio was within RULE_NEAR = 5e-3 of tol while the other outcome would have changed
the sweep count (cd_mod_model.py, rule_margin).  The tests compare sweeps and codes on the decisive rows.  A multi-row
case in which fewer than 3/4 of the rows are certified AND decisive is refused (the script exits non-zero): choose
another seed, never a lower share.

Usage:  python tests/golden/generate_golden_cd_mod.py
"""
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
from lasso.linear.solvers import coord_descent_mod as reference_solver  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cd_mod_model  # noqa: E402
from cd_mod_cases import CASES, MAX_ITER, REFERENCE_CASES, TOL, case_inputs  # noqa: E402

NEAR = 0.05            # an evaluated gap this close to the threshold (relative) leaves the row uncertified
RULE_NEAR = 5e-3       # relative distance of the check rule's ratio from tol below which rounding may flip it
SHARE = 0.75           # least share of certified rows in a multi-row case


def run_case(name, spec):
    x, w = case_inputs(spec)
    alpha = spec["alpha"]
    t0 = time.time()
    z32, g32, i32 = cd_mod_model.coord_descent_mod(x, w, alpha=alpha, max_iter=MAX_ITER, tol=TOL)
    z64, g64, i64 = cd_mod_model.coord_descent_mod(x.double(), w.double(), alpha=alpha, max_iter=MAX_ITER, tol=TOL)
    rec = {}
    if name in REFERENCE_CASES:
        zr, gr = reference_solver(x.clone(), w.clone(), alpha=alpha, max_iter=MAX_ITER, tol=TOL)
        if not (torch.equal(zr, z32) and torch.equal(gr, g32)):
            raise SystemExit("case %s: the host model differs from the reference (max|dz| = %g, max|dgap| = %g)"
                             % (name, (zr - z32).abs().max(), (gr - g32).abs().max()))
        rec["z_ref"], rec["gap_ref"] = zr.numpy(), gr.numpy()
    certified = ((i32["sweeps"] == i64["sweeps"]) & i32["converged"] & i64["converged"]
                 & (i32["closest"] >= NEAR) & (i64["closest"] >= NEAR))
    decisive = certified & (i32["rule_margin"] >= RULE_NEAR) & (i64["rule_margin"] >= RULE_NEAR)
    share = float(decisive.float().mean())
    if spec["n"] > 1 and share < SHARE:
        raise SystemExit("case %s refused: %d of %d rows certified, %d decisive"
                         % (name, int(certified.sum()), spec["n"], int(decisive.sum())))
    spread = (z32.double() - z64).abs().max(1)[0]
    rec.update({
        "z32": z32.numpy(), "gap32": g32.numpy(), "sweeps32": i32["sweeps"].numpy(),
        "converged32": i32["converged"].numpy(), "committed32": np.int64(i32["committed"]),
        "z64": z64.numpy(), "gap64": g64.numpy(), "sweeps64": i64["sweeps"].numpy(),
        "converged64": i64["converged"].numpy(),
        "certified": certified.numpy(), "decisive": decisive.numpy(), "spread": spread.numpy(),
        "rule_margin32": i32["rule_margin"].numpy(), "rule_margin64": i64["rule_margin"].numpy(),
    })
    print("%-15s certified %3d/%3d decisive %3d  sweeps %d..%d  nnz %d  spread %.2e  reference %s  %.1fs" %
          (name, int(certified.sum()), spec["n"], int(decisive.sum()), int(i32["sweeps"].min()), int(i32["sweeps"].max()),
           int((z32 != 0).sum()), float(spread.max()), "equal" if name in REFERENCE_CASES else "-", time.time() - t0))
    return rec


def main():
    arrays = {}
    for name, spec in CASES.items():
        for key, val in run_case(name, spec).items():
            arrays["%s/%s" % (name, key)] = val
    assert not arrays["sq24_all_zero/z32"].any(), "the all-zero case has a nonzero code: raise its alpha"
    path = os.path.join(HERE, "cd_mod_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
