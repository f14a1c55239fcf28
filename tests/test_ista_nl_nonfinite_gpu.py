"""NaN and Inf operand values through ``ista_nl``.  Rows are independent, under lr='auto' too (L is per row): a poison in
one row of x or z0 stays in that row, which matches the host model class for class (finite, NaN, +Inf, -Inf); every other
row is bit for bit what it is without the bad row.  The batch-wide stop rule sees a NaN sum and never fires: ``maxiter``
iterations run, with no warning.

The poisons are VALUES inside valid buffers; nothing here is meant to fault or hang.  Read for bounds before the first
run: no index or trip count of csrc/ista_nl.hip derives from a floating value (grids, block counts and the chunk sizes
come from n, d, k, maxiter and power_iters; a NaN sum fails ``<= budget`` and the chunk sizer of csrc/stoprule_host.hpp
answers a NaN with the largest chunk)."""
import warnings

import pytest
import torch

import ista_nl_model as model
from ista_nl_cases import recipe

pytestmark = pytest.mark.gpu
N, D, K, ROW = 33, 48, 130, 7


def classes(t):
    return torch.where(torch.isnan(t), 1, 0) + torch.where(t == float("inf"), 2, 0) + torch.where(t == float("-inf"), 3, 0)


def problem(activation):
    x, w, b = recipe(N, D, K, 2, activation)
    g = torch.Generator().manual_seed(3)
    z0 = 0.1 * torch.randn(N, K, generator=g) * (torch.arange(K) % 3 == 0)
    return x, w, b, z0, torch.randn(N, K, generator=g)


def solve(x, w, b, z0, u0, activation, lr):
    from lasso_amd.nonlinear import affine, ista_nl
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        z, info = ista_nl(x.cuda(), z0.cuda(), affine(w.cuda(), b.cuda(), activation), alpha=0.05, lr=lr, maxiter=6, tol=1e-3,
                          power_iters=4, power_init=u0.cuda(), return_info=True)
    assert [str(c.message) for c in caught] == []
    return z.cpu(), info


_CLEAN = {}


def clean(activation, lr):
    if (activation, lr) not in _CLEAN:
        _CLEAN[activation, lr] = solve(*problem(activation), activation, lr)
    return _CLEAN[activation, lr]


@pytest.mark.parametrize("lr", [0.1, "auto"])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["x", "z0"])
@pytest.mark.parametrize("activation", ["sigmoid", "relu"])
def test_a_poisoned_row_stays_in_its_row(activation, where, poison, lr):
    x, w, b, z0, u0 = problem(activation)
    {"x": x, "z0": z0}[where][ROW, 5] = poison
    z, info = solve(x, w, b, z0, u0, activation, lr)
    zc, ic = clean(activation, lr)
    assert ic["iterations"] == 6 and not ic["stopped"] and torch.isfinite(zc).all()
    zm, im = model.ista_nl(x, z0, w, b, activation, alpha=0.05, lr=lr, maxiter=6, tol=1e-3, power_iters=4, power_init=u0)
    assert im["iterations"] == 6 and not torch.isfinite(zm[ROW]).all()
    # the stop never fires: maxiter iterations; no sum the rule saw is finite (an Inf at first from an Inf in x, then NaN)
    assert info["iterations"] == 6 and not info["stopped"] and all(not abs(dl) < float("inf") for dl in info["deltas"])
    others = torch.arange(N) != ROW
    assert torch.equal(z[others].view(torch.int32), zc[others].view(torch.int32))
    assert torch.equal(classes(z[ROW]), classes(zm[ROW])), (classes(z[ROW]), classes(zm[ROW]))
    if lr == "auto":
        assert torch.equal(info["L"].cpu()[others].view(torch.int32), ic["L"].cpu()[others].view(torch.int32))


@pytest.mark.parametrize("where", ["w", "b"])
def test_a_nan_in_the_weight_or_bias_reaches_every_row(where):
    x, w, b, z0, u0 = problem("tanh")
    if where == "w":
        w[5, 9] = float("nan")
    else:
        b[5] = float("nan")
    z, info = solve(x, w, b, z0, u0, "tanh", 0.1)
    assert info["iterations"] == 6 and torch.isnan(z).any(dim=1).all()
