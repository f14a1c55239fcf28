"""float64 M-step on the HIP path (update_dict, update_dict_ridge, dict_learning in double: fp64-MFMA Gram product,
atom sweep, Cholesky solve) against the oracle run in float64 on the CPU on the same seeded inputs.

Bars: the project's fp32 bars scaled by the ratio of the unit round-offs, 2^-29 (the rule of tests/test_f64_gpu.py):
unit-norm atoms after update_dict 1e-4 * 2^-29 = 1.9e-13, re-drawn atoms and dictionaries of an EM run 5e-5 * 2^-29 =
9.3e-14 (a wrong RNG stream shows as O(1)), update_dict_ridge 3.7e-13 * max(1, max|V|) (2e-4 * 2^-29), losses 1e-13
relative.  The reference side alone (the oracle against itself in Gram form, or with its rows permuted) stays below
7.8e-15 on these shapes, so every bar has more than 20x headroom over summation-order effects, while anything with a
single-precision step inside is 1e-7 or worse.  The Gram product's bound is the worst case of a length-n dot product
in any order, 2 n 2^-53 |Z|^T |Z| element-wise.  Every test prints the deviation it measured."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from recipes import recipe_xw

pytestmark = pytest.mark.gpu

S = 2.0 ** -29
ATOM_BAR = 1e-4 * S          # 1.9e-13
DRAW_BAR = 5e-5 * S          # 9.3e-14
RIDGE_BAR = 2e-4 * S         # 3.7e-13
LOSS_RTOL = 1e-13

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _orc():
    from oracle import lasso_oracle as orc
    return orc


@functools.lru_cache(maxsize=None)
def problem(n, d, k):
    """(X, W, Z) in double, computed once per shape and never modified: Z = 8 FISTA iterations of the oracle with
    columns 0 and 7 zeroed (two atoms degenerate in the sweep)"""
    orc = _orc()
    X, W = recipe_xw(n, d, k, 0)
    X, W = X.double(), W.double()
    lr = 1.0 / orc.lipschitz_constant(W, "exact")
    Z = orc.fista(X, X.new_zeros(n, k), W, 0.3, lr=lr, maxiter=8, tol=0.0).clone()
    Z[:, [0, 7]] = 0.0
    return X, W, Z


# 1 -- Gram product -----------------------------------------------------------------------------------------------
def _check_gram(tag, Zc, Xc, Zg, Xg):
    from lasso_amd.engine import HipEngine
    n, k = Zc.shape
    d = Xc.shape[1]
    eng = HipEngine()
    buf = torch.full((k * k + k * d,), float('nan'), dtype=torch.float64, device='cuda')
    A, B = eng.gram(Zg, Xg, buf)
    A, B = A.cpu(), B.cpu()
    Ar, Br = Zc.T @ Zc, Zc.T @ Xc
    tolA = 2.0 * n * 2.0 ** -53 * (Zc.abs().T @ Zc.abs())
    tolB = 2.0 * n * 2.0 ** -53 * (Zc.abs().T @ Xc.abs())
    ea, eb = (A - Ar).abs(), (B - Br).abs()
    print("%s: max|dA| = %.3g, max|dB| = %.3g; worst ratio to the bound %.3g / %.3g"
          % (tag, ea.max().item(), eb.max().item(), (ea / tolA.clamp_min(1e-300)).max().item(),
             (eb / tolB.clamp_min(1e-300)).max().item()))
    assert A.dtype is torch.float64 and B.dtype is torch.float64
    assert bool((ea <= tolA).all()) and bool((eb <= tolB).all()), tag
    assert torch.equal(A, A.T), tag                                  # exactly symmetric
    buf2 = torch.full_like(buf, float('nan'))
    A2, B2 = eng.gram(Zg, Xg, buf2)
    assert torch.equal(A2.cpu(), A) and torch.equal(B2.cpu(), B), tag     # two calls: the same bits


def _gram_inputs(n, d, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(n, k, generator=g, dtype=torch.float64)
    Z = Z * (torch.rand(n, k, generator=g) < 0.4)                    # a code: mostly zeros
    X = torch.randn(n, d, generator=g, dtype=torch.float64)
    return Z, X


@pytest.mark.parametrize("n,d,k", [(37, 10, 50), (257, 70, 33), (500, 130, 96), (1030, 48, 200), (1, 3, 2)])
def test_gram_product(n, d, k):
    Z, X = _gram_inputs(n, d, k)
    _check_gram("gram_%dx%dx%d" % (n, d, k), Z, X, Z.cuda(), X.cuda())


def test_gram_product_strided_x_and_row_split():
    """X a column slice of a wider matrix (and Z one too); n = 2500 rows: the product splits its rows into partial
    slabs from n = 2048 on (kGramSplitMinRows in csrc/mstep_f64.hip; two slabs of 1264 and 1236 rows here) and
    folds them in slab order"""
    Z, X = _gram_inputs(300, 70, 96, seed=1)
    g = torch.Generator().manual_seed(2)
    wide = torch.randn(300, 130, generator=g, dtype=torch.float64)
    wide[:, 25:95] = X
    zwide = torch.zeros(300, 100, dtype=torch.float64)
    zwide[:, 3:99] = Z
    Xg, Zg = wide.cuda()[:, 25:95], zwide.cuda()[:, 3:99]
    assert not Xg.is_contiguous() and not Zg.is_contiguous()
    _check_gram("gram_strided", Z, X, Zg, Xg)
    for n, d, k in [(2500, 10, 50), (4100, 70, 130)]:
        Z, X = _gram_inputs(n, d, k, seed=3)
        _check_gram("gram_split_%dx%dx%d" % (n, d, k), Z, X, Z.cuda(), X.cuda())


# 2 -- update_dict ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def update_dict_reference(n, d, k, positive):
    orc = _orc()
    X, W, Z = problem(n, d, k)
    D, Zr = W.clone(), Z.clone()
    torch.manual_seed(3)
    out = orc.update_dict(D, X, Zr, positive=positive)
    assert out is D
    return D, Zr


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("n,d,k", [(37, 10, 50), (100, 48, 200), (257, 70, 33), (200, 130, 96), (300, 300, 520),
                                   (60, 520, 40)])          # (the last: d > 512, the widest form of the block kernel)
def test_update_dict(n, d, k, positive):
    from lasso_amd.linear.dict_learning import update_dict
    X, W, Z = problem(n, d, k)
    Dr, Zr = update_dict_reference(n, d, k, positive)
    redrawn = (Zr == 0).all(0)
    assert redrawn[0] and redrawn[7]
    Dg, Zg = W.cuda(), Z.cuda()
    torch.manual_seed(3)
    out = update_dict(Dg, X.cuda(), Zg, positive=positive)
    assert out is Dg and Dg.dtype is torch.float64
    D, Zn = Dg.cpu(), Zg.cpu()
    err = (D - Dr).abs().max(0).values
    used = err[~redrawn].max().item() if (~redrawn).any() else 0.0
    drawn = err[redrawn].max().item()
    norms = (D.norm(dim=0) - 1).abs().max().item()
    print("update_dict %dx%dx%d positive=%s: used atoms %.3g (bar %.3g), %d re-drawn atoms %.3g (bar %.3g), "
          "|norm - 1| %.3g" % (n, d, k, positive, used, ATOM_BAR, int(redrawn.sum()), drawn, DRAW_BAR, norms))
    assert used <= ATOM_BAR
    assert drawn <= DRAW_BAR
    assert torch.equal(Zn == 0, Zr == 0)
    assert norms <= 1e-14
    if (n, d, k) == (37, 10, 50):        # CPU tensors are staged through the device and updated in place
        Dc, Zc = W.clone(), Z.clone()
        torch.manual_seed(3)
        out = update_dict(Dc, X, Zc, positive=positive)
        assert out is Dc and not Dc.is_cuda
        assert torch.equal(Dc, D) and torch.equal(Zc, Zn)


# 3 -- update_dict_ridge ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k", [(37, 10, 50), (100, 48, 200), (257, 70, 33), (200, 130, 96), (300, 300, 520),
                                   (150, 20, 130)])         # (the last: two 64-blocks and a ragged edge)
def test_update_dict_ridge(n, d, k):
    """lambd = 1e-2, the value dict_learning calls update_dict_ridge with.  The bar needs a system the reference itself
    solves well below it: with the two dead atoms (and k > n in two shapes) Z^T Z is singular and lambd n I is all
    that conditions it.  At lambd = 1e-2 the oracle against itself with permuted rows deviates by at most 1.4e-14 on
    these shapes (27x under the bar); at 1e-4 the condition number is 2e3 .. 1.5e4 and the oracle is already 1.3e-12
    from its permuted self and 8e-13 from a long-double solve of its own matrix -- above the bar before any kernel of
    this library has run."""
    from lasso_amd.linear.dict_learning import update_dict_ridge
    orc = _orc()
    X, _, Z = problem(n, d, k)
    ref = orc.update_dict_ridge(X, Z, lambd=1e-2)
    got = update_dict_ridge(X.cuda(), Z.cuda(), lambd=1e-2)
    assert got.is_cuda and got.dtype is torch.float64 and tuple(got.shape) == (d, k)
    err = (got.cpu() - ref).abs().max().item()
    bar = RIDGE_BAR * max(1.0, ref.abs().max().item())
    print("update_dict_ridge %dx%dx%d: max|dV| = %.3g (bar %.3g, max|V| = %.3g)" % (n, d, k, err, bar, ref.abs().max().item()))
    assert err <= bar
    if (n, d, k) == (37, 10, 50):
        got_cpu = update_dict_ridge(X, Z, lambd=1e-2)                # CPU tensors: the result comes back to the CPU
        assert not got_cpu.is_cuda and torch.equal(got_cpu, got.cpu())


def test_update_dict_ridge_reports_a_non_positive_pivot():
    from lasso_amd.linear.dict_learning import update_dict_ridge
    X, _, Z = problem(37, 10, 50)
    with pytest.raises(torch.linalg.LinAlgError):
        update_dict_ridge(X.cuda(), torch.zeros_like(Z).cuda(), lambd=0.0)


# 4 -- dict_learning ----------------------------------------------------------------------------------------------
def _em_data(n, d, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g, dtype=torch.float64)


def _check_em(tag, got, ref):
    (W, losses), (Wr, lr_) = got, ref
    assert W.dtype is torch.float64 and losses.dtype is torch.float64 and Wr.dtype is torch.float64
    ew = (W.cpu() - Wr).abs().max().item()
    el = ((losses.cpu() - lr_).abs() / lr_.abs()).max().item()
    print("%s: max|dW| = %.3g (bar %.3g), losses rel %.3g (bar %.3g)" % (tag, ew, DRAW_BAR, el, LOSS_RTOL))
    assert ew <= DRAW_BAR
    assert el <= LOSS_RTOL


@pytest.mark.parametrize("kw", [dict(), dict(constrained=False), dict(persist=True)],
                         ids=["constrained", "ridge", "persist"])
def test_dict_learning_matches_the_oracle_in_double(kw):
    from lasso_amd.linear import dict_learning
    orc = _orc()
    X = _em_data(300, 32)
    args = dict(alpha=0.3, lr=0.05, maxiter=20, steps=5, **kw)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(1)
        ref = orc.dict_learning(X, 64, **args)
        torch.manual_seed(1)
        got = dict_learning(X, 64, progbar=False, **args)
    finally:
        torch.set_default_dtype(old)
    assert got[0].device.type == "cpu" and tuple(got[0].shape) == (32, 64) and tuple(got[1].shape) == (5,)
    _check_em("dict_learning_f64_%s" % (",".join(kw) or "constrained"), got, ref)


def test_dict_learning_lr_auto(monkeypatch):
    """lr='auto': the oracle runs with the device's own float64 lipschitz_constant as its step (its ARPACK value differs
    in the last digits, as test_lr_auto_matches_reference_within_arpack_jitter notes)"""
    from lasso_amd.linear import dict_learning
    from lasso_amd.linear.lipschitz import lipschitz_constant
    orc = _orc()
    monkeypatch.setattr(orc, "lipschitz_constant", lambda w, method="arpack": float(lipschitz_constant(w.cuda())))
    X = _em_data(257, 48, seed=6)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(4)
        ref = orc.dict_learning(X, 100, alpha=0.3, steps=4)
        torch.manual_seed(4)
        got = dict_learning(X, 100, alpha=0.3, steps=4, progbar=False)
    finally:
        torch.set_default_dtype(old)
    _check_em("dict_learning_f64_lr_auto", got, ref)


def test_dict_learning_redraws_degenerate_atoms(monkeypatch):
    """alpha = 2 leaves atoms without any code: the oracle re-draws atoms in its steps ([3, 1, 1, 1] of them); the
    float64 column-view draw has to consume the generator exactly as the reference's dictionary[:, k].normal_() does"""
    from lasso_amd.linear import dict_learning
    orc = _orc()
    g = torch.Generator().manual_seed(11)
    X = torch.randn(60, 16, generator=g, dtype=torch.float64)
    W0 = torch.nn.functional.normalize(torch.randn(16, 48, generator=g, dtype=torch.float64), dim=0)
    steps_with_draws = []
    plain = orc.update_dict

    def counting(dictionary, X_, Z_, *a, **kw):
        before = torch.get_rng_state()
        out = plain(dictionary, X_, Z_, *a, **kw)
        steps_with_draws.append(not torch.equal(before, torch.get_rng_state()))
        return out
    monkeypatch.setattr(orc, "update_dict", counting)
    args = dict(alpha=2.0, lr=0.1, maxiter=30, steps=4)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)                  # the oracle's losses take the default dtype
    try:
        torch.manual_seed(2)
        ref = orc.dict_learning(X, 48, init_weight=W0, **args)
        assert any(steps_with_draws), "the oracle re-drew no atom: the case does not test the draws"
        monkeypatch.setattr(orc, "update_dict", plain)
        torch.manual_seed(2)
        got = dict_learning(X.cuda(), 48, init_weight=W0, device='cuda', progbar=False, **args)
    finally:
        torch.set_default_dtype(old)
    assert ref[1].dtype is torch.float64
    assert got[0].is_cuda and got[1].is_cuda
    print("steps in which the oracle re-drew atoms: %s" % steps_with_draws)
    _check_em("dict_learning_f64_degenerate", got, ref)


# 5 -- refusals; the fp32 path beside the float64 one -------------------------------------------------------------
_FP32_SCRIPT = r"""
import sys, torch
sys.path[:0] = [%(pkg)r, %(tests)r]
from recipes import recipe_xw
from lasso_amd.linear.dict_learning import update_dict
X, W = recipe_xw(200, 64, 96, 0)
g = torch.Generator().manual_seed(9)
Z = torch.randn(200, 96, generator=g) * (torch.rand(200, 96, generator=g) < 0.3)
Z[:, 5] = 0
D = W.cuda()
torch.manual_seed(7)
update_dict(D, X.cuda(), Z.cuda())
torch.save(D.cpu(), %(out)r)
"""


def test_refusals_and_fp32_update_dict_is_untouched(tmp_path):
    from lasso_amd import _native as nat
    from lasso_amd.linear.dict_learning import update_dict, update_dict_ridge, dict_learning
    from lasso_amd.parallel import dict_learning_sharded
    X, W, Z = problem(100, 48, 200)
    Xg, Wg, Zg = X.cuda(), W.cuda(), Z.cuda()
    # mixed float32 / float64 among the tensors of one call: RuntimeError, nothing written
    for args in [(Wg.float(), Xg, Zg), (Wg, Xg.float(), Zg), (Wg, Xg, Zg.float())]:
        before = [t.clone() for t in args]
        with pytest.raises(RuntimeError):
            update_dict(*args)
        assert all(torch.equal(a, b) for a, b in zip(args, before))
    with pytest.raises(RuntimeError):
        update_dict_ridge(Xg, Zg.float())
    with pytest.raises(RuntimeError):
        dict_learning(Xg, 200, init_weight=Wg.float(), steps=1, lr=0.05, progbar=False)
    # the multi-GPU driver and the other E-step algorithms name float64 as the cause
    with pytest.raises(NotImplementedError, match="float64"):
        dict_learning_sharded(Xg, 200, steps=1, lr=0.05)
    for algorithm in ("cd", "gpsr"):
        with pytest.raises(NotImplementedError, match="float64"):
            dict_learning(Xg, 200, init_weight=Wg, steps=1, algorithm=algorithm, progbar=False)
    # float64 M-steps, then an fp32 update_dict on the same engine (same process, same stream, same workspace cache):
    # bitwise what a fresh process gives
    D64 = Wg.clone()
    update_dict(D64, Xg, Zg.clone())
    update_dict_ridge(Xg, Zg)
    X32, W32 = recipe_xw(200, 64, 96, 0)
    g = torch.Generator().manual_seed(9)
    Z32 = torch.randn(200, 96, generator=g) * (torch.rand(200, 96, generator=g) < 0.3)
    Z32[:, 5] = 0
    D32 = W32.cuda()
    torch.manual_seed(7)
    update_dict(D32, X32.cuda(), Z32.cuda())
    tags = {key[-1] for key in nat._WS}
    assert {"gram", "sweep", "gram_f64", "sweep_f64", "ridge_f64"} <= tags, tags      # the float64 tags are their own
    out = str(tmp_path / "fp32_fresh.pt")
    code = _FP32_SCRIPT % dict(pkg=os.path.join(ROOT, "pytorch-lasso_amd"), tests=os.path.join(ROOT, "tests"), out=out)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)
    fresh = torch.load(out)
    assert fresh.dtype is torch.float32 and torch.equal(fresh, D32.cpu())
