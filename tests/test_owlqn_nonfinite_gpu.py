"""NaN and Inf operand values through owlqn.  Every decision of the solver is batch-wide: one poisoned row of x reaches
the one objective, so the solve ends with the last accepted iterate and a warning (as orthant_wise_newton does) -- for a
poison present from the start that iterate is z0, bit for bit.

The poisons are VALUES inside valid buffers; nothing here is meant to fault or hang.  Read for bounds before the first
run: no index or trip count of csrc/owlqn.hip derives from a floating value (segments, ring slots and grids come from
n, k and the integer ring state); the Brent search is capped at 500 evaluations and the ladder at ls_maxiter trials, and
both end at the first non-finite objective; a NaN y.s fails ``> 1e-10`` and the pair is dropped."""
import warnings

import pytest
import torch

from owlqn_cases import recipe

pytestmark = pytest.mark.gpu
WARNING = "owlqn: the objective is not finite; returning the last accepted iterate"


def solve(x, w, z0, **kw):
    from lasso_amd.nonlinear import owlqn, rss
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        z, info = owlqn(rss(x.cuda(), w.cuda()), z0.cuda(), alpha=0.1, return_info=True, **kw)
    return z.cpu(), info, [str(c.message) for c in caught]


@pytest.mark.parametrize("line_search", ["brent", "backtrack", "none"])
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("where", ["x", "w", "z0"])
def test_a_poison_from_the_start_returns_z0(where, poison, line_search):
    n, d, k = 33, 48, 130
    x, w = recipe(n, d, k, seed=2)
    z0 = 0.1 * torch.randn(n, k, generator=torch.Generator().manual_seed(3)) * (torch.arange(k) % 3 == 0)
    {"x": x, "w": w, "z0": z0}[where][7, 5] = poison                     # one element of one row
    z, info, said = solve(x, w, z0, line_search=line_search, max_iter=4, history_size=2, lr=0.05)
    assert said == [WARNING]
    assert info["iterations"] == 0 and info["objective"] == [] and info["evaluations"] == []
    assert torch.equal(z.view(torch.int32), z0.view(torch.int32))          # z0 as it came, its poison included


def test_an_overflow_ends_the_solve_with_the_last_accepted_iterate():
    """finite inputs and a step of about 1e27 (lr = 1e30 over |pg|_1): the objective of the step overflows float32"""
    n, d, k = 33, 48, 130
    x, w = recipe(n, d, k, seed=2)
    z0 = torch.zeros(n, k)
    # a fixed step is taken unexamined: it is the last accepted iterate, and its objective is what ended the solve
    z, info, said = solve(x, w, z0, line_search="none", max_iter=6, history_size=2, lr=1e30)
    assert said == [WARNING]
    assert info["iterations"] == 1 and info["objective"] == [float("inf")]
    assert info["pairs"] == [0] and info["skipped"] == [False]                 # no update after the iteration that stops
    assert torch.isfinite(z).all() and float(z.abs().max()) > 1e20
    # a search that evaluates before it accepts never takes the overflowing step: z0 comes back
    zb, infob, saidb = solve(x, w, z0, line_search="backtrack", max_iter=6, history_size=2, lr=1e30,
                             ls_options=dict(maxiter=4))
    assert saidb == [WARNING] and infob["iterations"] == 0 and torch.equal(zb, z0)
    assert 1 <= len(infob["evaluations"]) <= 4 and infob["evaluations"][0][2] == float("inf")   # (one ladder of rungs)


def test_the_clean_batch_is_untouched_by_the_checks_above():
    """the same call without a poison runs its iterations and warns of nothing"""
    x, w = recipe(33, 48, 130, seed=2)
    z, info, said = solve(x, w, torch.zeros(33, 130), line_search="none", max_iter=4, history_size=2, lr=0.05)
    assert said == [] and info["iterations"] == 4 and torch.isfinite(z).all()
