#!/usr/bin/env python3
"""Generate tests/golden/batch_solve_cases.npz by running the REAL reference's batch_cholesky_solve
(rfeinman/pytorch-lasso, lasso/linear/utils.py:43-58) on the CPU, in float32 AND in float64.

Runs only where the reference is mounted (/root/reference); the .npz it writes is data: the inputs are re-creatable
from the seeded recipes of tests/batch_solve_cases.py, the expected outputs are stored.  utils.py imports only torch
and warnings, so it is loaded by path; no reference file is edited or copied.

Per case and dtype: x (the reference's result), warned (whether it gave its LU warning), info (cholesky_ex's info per
system: the order of the first leading minor that is not positive definite) and spread -- the largest, over the
systems and the variants, of max|x_variant - x| / max|x|, where a variant is a seeded symmetric permutation P A P^T,
P b solved with torch on the route the case takes and un-permuted ("another correct implementation"); the float32
spread includes the distance to the float64 result.  A case with spread > SPREAD_CAP is refused (exit status 1).
The names and defaults of the reference's four functions are recorded, and for the non-finite cases the results as
they are (NaN and Inf included; where the case takes the LU route, also the spread of the rows that stay finite).

Usage:  python tests/golden/generate_golden_batch_solve.py
"""
import importlib.util
import inspect
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from batch_solve_cases import CASES, DTYPES, NONFINITE, PERM_SEEDS, SPREAD_CAP, dtypes_of, inputs, nonfinite_inputs, rel_rows  # noqa: E402

_spec = importlib.util.spec_from_file_location("reference_linear_utils", "/root/reference/lasso/linear/utils.py")
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
WARNING = "Cholesky factorization failed. Reverting to LU decomposition..."


def run_reference(b, A):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        x = ref.batch_cholesky_solve(b.clone(), A.clone())
    texts = [str(c.message) for c in caught]
    assert all(t == WARNING for t in texts) and len(texts) <= 1, texts
    return x, bool(texts)


def solve_like(b, A, lu):
    if lu:
        return torch.linalg.solve(A, b.unsqueeze(2)).squeeze(2)
    return torch.cholesky_solve(b.unsqueeze(2), torch.linalg.cholesky_ex(A)[0]).squeeze(2)


def main():
    out, report, failed = {}, [], False
    for name, spec in CASES.items():
        x64 = None
        for key in reversed(dtypes_of(spec)):            # float64 first: the float32 spread looks at it
            dtype = DTYPES[key]
            b, A = inputs(spec, dtype)
            x, warned = run_reference(b, A)
            info = torch.linalg.cholesky_ex(A)[1]
            assert warned == bool((info != 0).any())
            assert bool(torch.isfinite(x).all()), name
            spread = 0.0
            for seed in PERM_SEEDS:
                perm = torch.randperm(spec["D"], generator=torch.Generator().manual_seed(seed))
                xp = solve_like(b[:, perm], A[:, perm][:, :, perm], warned)
                back = torch.empty_like(xp)
                back[:, perm] = xp
                spread = max(spread, float(rel_rows(back.numpy(), x.numpy()).max()))
            if key == "64":
                x64 = x
            elif x64 is not None:
                spread = max(spread, float(rel_rows(x.numpy(), x64.numpy()).max()))
            out["%s/x%s" % (name, key)] = x.numpy()
            out["%s/warned%s" % (name, key)] = np.array(warned)
            out["%s/info%s" % (name, key)] = info.numpy().astype(np.int32)
            out["%s/spread%s" % (name, key)] = np.array(spread)
            ok = spread <= SPREAD_CAP
            failed |= not ok
            report.append("%-22s f%s  warned %d  spread %.3g%s" % (name, key, warned, spread, "" if ok else "   REFUSED"))
    for name in NONFINITE:
        for key, dtype in DTYPES.items():
            b, A = nonfinite_inputs(name, dtype)
            x, warned = run_reference(b, A)
            out["nonfinite_%s/x%s" % (name, key)] = x.numpy()
            out["nonfinite_%s/warned%s" % (name, key)] = np.array(warned)
            if warned:                                   # the rows that stay finite are judged like any LU result
                keep = [i for i in range(x.shape[0]) if i != NONFINITE[name][2]]
                bk, Ak, xk = b[keep], A[keep], x[keep]
                spread = 0.0
                for seed in PERM_SEEDS:
                    perm = torch.randperm(bk.shape[1], generator=torch.Generator().manual_seed(seed))
                    back = torch.empty_like(xk)
                    back[:, perm] = solve_like(bk[:, perm], Ak[:, perm][:, :, perm], True)
                    spread = max(spread, float(rel_rows(back.numpy(), xk.numpy()).max()))
                if key == "32":
                    b64, A64 = nonfinite_inputs(name, torch.float64)
                    spread = max(spread, float(rel_rows(xk.numpy(), solve_like(b64[keep], A64[keep], True).numpy()).max()))
                assert spread <= SPREAD_CAP
                out["nonfinite_%s/spread%s" % (name, key)] = np.array(spread)
            report.append("nonfinite_%-12s f%s  warned %d  non-finite rows %s" % (
                name, key, warned, sorted(set(np.nonzero(~np.isfinite(x.numpy()))[0].tolist()))))
    sigs = {}
    for fn in ("qr", "lstsq", "ridge", "batch_cholesky_solve"):
        params = inspect.signature(getattr(ref, fn)).parameters
        sigs[fn] = [[p, None if v.default is inspect.Parameter.empty else v.default] for p, v in params.items()]
    out["signatures"] = np.array(json.dumps(sigs))
    out["warning"] = np.array(WARNING)
    print("\n".join(report))
    if failed:
        sys.exit(1)
    path = os.path.join(HERE, "batch_solve_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
