#!/usr/bin/env python3
"""Write tests/golden/f64_cases.npz: float64 codes of the REAL reference (rfeinman/pytorch-lasso) for the cases of
tests/golden_f64.py -- FISTA and ISTA, 25 iterations at a fixed step, and one line-search case.

Run once where a checkout of the reference is available (never on the GPU machine); the reference is imported the way
generate_golden.py imports it, from the directory named by LASSO_REFERENCE_DIR or the first argument.  Inputs are
re-drawn from the seeded recipe; only the resulting codes and each case's step size are stored.

Usage:  LASSO_REFERENCE_DIR=<checkout> python tests/golden/generate_golden_f64.py [--run NAME]

The reference's float64 GEMMs sum in another order on other kinds of CPU, so the bitwise fixture holds on the kind of
CPU it was recorded on, like the fp32 ones.  --run NAME records the reference on this CPU as a further run, as
generate_golden.py does: tests/golden/NAME/f64_cases.npz keeps the arrays that differ from the primary fixture, and the
test takes the run tests/golden_runs.py picks for the CPU it runs on.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import scipy.optimize.optimize as _so
from scipy.optimize import _optimize as _o

_so._status_message = _o._status_message          # the shim of generate_golden.py
ARGS = sys.argv[1:]
RUN = None            # --run NAME: record this CPU as a further run, tests/golden/NAME/f64_cases.npz
if "--run" in ARGS:
    RUN = ARGS[ARGS.index("--run") + 1]
    del ARGS[ARGS.index("--run"):ARGS.index("--run") + 2]
REFERENCE = ARGS[0] if ARGS else os.environ.get("LASSO_REFERENCE_DIR")
if not REFERENCE or not os.path.isdir(REFERENCE):
    sys.exit("usage: generate_golden_f64.py [--run NAME] <checkout of the reference>   (or LASSO_REFERENCE_DIR)")
sys.path.insert(0, REFERENCE)
import torch  # noqa: E402
import lasso  # noqa: E402,F401
import lasso.linear  # noqa: E402,F401

ref_ista = sys.modules["lasso.linear.solvers.ista"].ista

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from golden_f64 import CASES, case_inputs  # noqa: E402


def main():
    arrays = {}
    for tag, case in CASES.items():
        X, W, z0, kw = case_inputs(case)
        z = ref_ista(X, z0, W, alpha=case["alpha"], **kw)
        assert z.dtype == torch.float64
        arrays[tag + "_z"] = z.numpy()
        arrays[tag + "_lr"] = np.float64(kw["lr"])
        print(tag, "nnz", int((z != 0).sum()), "max|z|", z.abs().max().item())
    path = os.path.join(HERE, "f64_cases.npz")
    if RUN:       # a further run: only the arrays that differ from the primary fixture (tests/golden_runs.py)
        primary = np.load(path)
        arrays = {k: v for k, v in arrays.items() if k not in primary.files or not np.array_equal(primary[k], v)}
        os.makedirs(os.path.join(HERE, RUN), exist_ok=True)
        path = os.path.join(HERE, RUN, "f64_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
