"""NaN and Inf operand values through iterative_ridge_bfgs, against the class pattern the reference produced
(tests/golden/irbfgs_cases.npz, the NONFINITE cases of tests/irbfgs_cases.py).  The curvature is per row, but the
objective, the step and the stop test are batch-wide: one poisoned row makes the objective non-finite, the solve stops
after its first iteration, that row comes back NaN except for its frozen zeros and the other rows are finite.  A NaN
in z0 puts a NaN on a system's diagonal: its Cholesky fails, the reference's warning is raised and the whole batch goes
through the LU route; a NaN in x leaves the systems finite and the Cholesky route is kept.

The poisons are VALUES inside valid buffers; nothing here is meant to fault or hang.  Read for bounds before the first
run: no index or trip count of csrc/irbfgs.hip derives from a floating value (grids and strides come from n and k), the
Brent search is capped at 500 evaluations and ends at the first non-finite objective, a NaN y.s fails ``|y.s| > 1e-10``,
and batch_solve's kernels replace a bad pivot and never search past their matrix (tests/test_batch_solve_gpu.py)."""
import warnings

import pytest
import torch

from irbfgs_cases import NONFINITE, classes, load_case, poisoned_inputs
from irbfgs_model import LU_WARNING

pytestmark = pytest.mark.gpu
NONFINITE_WARNING = 'iterative_ridge_bfgs: the objective is not finite; the solve ends with this iterate'


@pytest.fixture(scope="module")
def cases(golden):
    return golden("irbfgs_cases")


@pytest.mark.parametrize("name", sorted(NONFINITE))
def test_class_pattern_of_the_reference(cases, name):
    from lasso_amd.nonlinear import iterative_ridge_bfgs, rss
    entry, g = NONFINITE[name], load_case(cases, name)
    spec = entry["case"]
    x, w, z0 = poisoned_inputs(entry)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        z, info = iterative_ridge_bfgs(rss(x.cuda(), w.cuda()), z0.cuda(), alpha=spec["alpha"], return_info=True,
                                       **spec["kwargs"])
    z, said = z.cpu(), [str(c.message) for c in caught]
    want_said = [m for m in str(g["warnings"]).split("\n") if m]
    assert [m for m in said if m != NONFINITE_WARNING] == want_said
    assert said.count(NONFINITE_WARNING) == 1
    assert info["lu"] == [LU_WARNING in want_said]
    assert info["iterations"] == int(g["iterations"]) == 1 and info["invalid_rows"] == [-1]
    want = torch.from_numpy(g["z32"])
    assert torch.equal(classes(z), classes(want))
    row = entry["poison"][1]
    frozen = z0[row] == 0
    assert torch.equal(z[row][frozen], z0[row][frozen])
    others = [r for r in range(z.shape[0]) if r != row]
    assert torch.isfinite(z[others]).all()
    if name == "nan_z0":
        assert torch.isnan(z[row][~frozen]).all()


def test_the_clean_batch_is_untouched_by_the_checks_above():
    from lasso_amd.nonlinear import iterative_ridge_bfgs, rss
    entry = NONFINITE["nan_z0"]
    spec = entry["case"]
    from irbfgs_cases import case_inputs
    x, w, z0 = case_inputs(spec)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        z, info = iterative_ridge_bfgs(rss(x.cuda(), w.cuda()), z0.cuda(), alpha=spec["alpha"], return_info=True,
                                       **spec["kwargs"])
    assert not caught and info["iterations"] == 5 and info["lu"] == [False] * 5 and torch.isfinite(z).all()
