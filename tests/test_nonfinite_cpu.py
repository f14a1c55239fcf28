"""What the CPU oracle -- the reference's own ATen operations -- does with NaN and Inf operands, pinned for every case
of tests/nonfinite_cases.py.  tests/test_nonfinite_gpu.py holds the HIP kernels to exactly these class maps, so the
expectations stand here on their own: a change of the installed torch's semantics fails this module before it looks
like a kernel bug.  No GPU."""
import math
import warnings

import pytest
import torch

import nonfinite_cases as nf
from nonfinite_cases import FINITE, IS_NAN, IS_NINF, IS_PINF, NAN, NINF, PINF, classes, poison
from oracle import lasso_oracle as orc

DTYPES = [torch.float32, torch.float64]


def _rows(t, idx):
    return t[torch.tensor(sorted(idx))]


def _others(n, idx):
    return torch.tensor([i for i in range(n) if i not in set(idx)], dtype=torch.long)


def test_helpers():
    t = torch.tensor([[1.0, NAN, PINF], [NINF, -0.0, 3.0]])
    assert classes(t).tolist() == [[FINITE, IS_NAN, IS_PINF], [IS_NINF, FINITE, FINITE]]
    assert classes(t.to(torch.bfloat16)).tolist() == classes(t).tolist() == classes(t.double()).tolist()
    p = poison(torch.zeros(3, 2), [(0, 1), (2, 0)], PINF)
    assert p.tolist() == [[0.0, PINF], [0.0, 0.0], [PINF, 0.0]]
    assert poison(torch.zeros(2), 1, NAN).isnan().tolist() == [False, True]
    for n, d, _ in nf.LINEAR_FUSED + nf.LINEAR_GENERAL + nf.CD_SHAPES:
        rows = nf.row_positions(n, d)
        assert rows[0] == (0, 0) and rows[-1] == (n - 1, d - 1) and all(0 <= r < n and 0 <= c < d for r, c in rows)


@pytest.mark.parametrize("dtype", DTYPES)
def test_softshrink_propagates_nan(dtype):
    """F.softshrink(NaN) is NaN in the scalar and in the vectorised path of ATen's CPU kernel (ista.py:40,52,90)"""
    F = torch.nn.functional
    assert math.isnan(F.softshrink(torch.tensor(NAN, dtype=dtype), 0.25).item())
    v = torch.linspace(-2, 2, 67, dtype=dtype)
    at = [0, 1, 15, 16, 33, 66]
    v[at] = NAN
    out = F.softshrink(v, 0.25)
    assert torch.nonzero(out.isnan()).flatten().tolist() == at
    assert F.softshrink(torch.tensor([PINF, NINF], dtype=dtype), 0.25).tolist() == [PINF, NINF]
    assert orc.soft_threshold(v, 0.25).isnan().sum().item() == len(at)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("n,d,k", nf.LINEAR_FUSED[:2] + nf.LINEAR_GENERAL[:1])
def test_fista_rows_are_independent_and_poison_fills_its_row(n, d, k, fast, dtype):
    X, W, z0, lr = nf.linear_problem(n, d, k, dtype=dtype)
    pos = nf.row_positions(n, d)
    bad = [r for r, _ in pos]
    rest = _others(n, bad)
    for T in nf.ITERS:
        clean = orc.fista(X, z0, W, nf.ALPHA, fast=fast, lr=lr, maxiter=T, tol=0.0)
        assert classes(clean).eq(FINITE).all()
        for name, value in nf.X_POISONS:
            got = orc.fista(poison(X, pos, value), z0, W, nf.ALPHA, fast=fast, lr=lr, maxiter=T, tol=0.0)
            assert torch.equal(got[rest], clean[rest]), (name, T)              # bitwise: rows never interact
            c = _rows(classes(got), bad)
            if name == "nan" or T >= 2:
                assert c.eq(IS_NAN).all(), (name, T)
            else:
                # one iteration: z = S(z0 - lr (z0 W^T - x) W), an infinite +-lr * Inf * W[j, :] per element -- the
                # sign of W's row decides; a unit-norm random W has no exact zero in it
                j = {r: col for r, col in pos}
                for r in bad:
                    sign = torch.sign(W[j[r]]) * (1 if value > 0 else -1)
                    want = torch.where(sign > 0, IS_PINF, IS_NINF).to(torch.int8)
                    assert torch.equal(classes(got[r]), want), (name, r)
        got = orc.fista(X, poison(z0, [(r, k - 1) for r in bad], NAN), W, nf.ALPHA, fast=fast, lr=lr, maxiter=T, tol=0.0)
        assert torch.equal(got[rest], clean[rest]) and _rows(classes(got), bad).eq(IS_NAN).all()
        got = orc.fista(X, z0, poison(W, (d - 1, k - 1), NAN), nf.ALPHA, fast=fast, lr=lr, maxiter=T, tol=0.0)
        assert classes(got).eq(IS_NAN).all()                                   # a NaN in W reaches every element


@pytest.mark.parametrize("dtype", DTYPES)
def test_fista_stop_rule_never_fires_on_a_poisoned_batch(dtype):
    """ista.py:93: NaN <= budget is False -- maxiter iterations, a NaN last sum, no warning"""
    n, d, k = nf.LINEAR_FUSED[0]
    X, W, z0, lr = nf.linear_problem(n, d, k, dtype=dtype)
    for name, value in nf.X_POISONS:
        tr = orc.FistaTrace()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            orc.fista(poison(X, (3, 2), value), z0, W, nf.ALPHA, lr=lr, maxiter=12, tol=1e-4, trace=tr)
        assert tr.iterations == 12 and not tr.stopped and math.isnan(tr.delta[-1])
        # +-Inf: the first sum is +Inf (no stop either), NaN from the second on
        assert (math.isinf(tr.delta[0]) and tr.delta[0] > 0) if name != "nan" else math.isnan(tr.delta[0])
        assert all(math.isnan(v) for v in tr.delta[1:])


@pytest.mark.parametrize("dtype", DTYPES)
def test_backtracking_on_a_nan_objective(dtype):
    """ista.py:45: F <= Q is False for a NaN F on every trial -- all 1000 trials are spent, the search warns and
    reverts to lr0 (:48-52), so each outer iteration is the fixed-step iteration: clean rows bitwise those of the
    fixed-step run of the CLEAN batch at lr0, poisoned rows NaN."""
    n, d, k = nf.LINEAR_FUSED[0]
    X, W, z0, lr = nf.linear_problem(n, d, k, dtype=dtype)
    pos = nf.row_positions(n, d)
    bad = [r for r, _ in pos]
    tr = orc.FistaTrace()
    with pytest.warns(UserWarning, match="backtracking line search failed"):
        got = orc.fista(poison(X, pos, NAN), z0, W, nf.ALPHA, lr=lr, maxiter=2, tol=0.0, backtrack=True, trace=tr)
    assert tr.trials == [1000, 1000] and tr.accepted_lr == [lr, lr]
    fixed = orc.fista(X, z0, W, nf.ALPHA, lr=lr, maxiter=2, tol=0.0)
    assert torch.equal(got[_others(n, bad)], fixed[_others(n, bad)])
    assert _rows(classes(got), bad).eq(IS_NAN).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,k", nf.CD_SHAPES)
def test_coordinate_descent(n, d, k, dtype):
    X, W, z0, _ = nf.linear_problem(n, d, k, dtype=dtype)
    bad = [0, n - 1]
    rest = _others(n, bad)
    clean, cinfo = orc.coordinate_descent(X, W, z0.clone(), nf.ALPHA, maxiter=30, return_info=True)
    for what in ("x", "z0"):
        xp = poison(X, [(0, 0), (n - 1, d - 1)], NAN) if what == "x" else X
        zp = poison(z0, [(0, 0), (n - 1, k - 1)], NAN) if what == "z0" else z0.clone()
        got, info = orc.coordinate_descent(xp, W, zp, nf.ALPHA, maxiter=30, return_info=True)
        assert torch.equal(got[rest], clean[rest]), what
        assert torch.equal(info["row_steps"][rest], cinfo["row_steps"][rest]), what
        if what == "x":
            assert _rows(classes(got), bad).eq(IS_NAN).all()
        else:
            # coordinate_descent.py:19,52: b starts at x W whatever z0 holds and the result is S(b): a NaN in z0[i, j]
            # reaches b only once coordinate j is committed (:36, the NaN move times column j of S) -- and it is
            # committed at once: |NaN| is the argmax (:34)
            assert _rows(classes(got), bad).eq(IS_NAN).all()


@pytest.mark.parametrize("name", sorted(nf.CONV_CASES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_fista_nan_block_grows_with_the_receptive_field(name, dtype):
    x, w, z0, lr, st, pd = nf.conv_problem(name, dtype=dtype)
    xp = poison(x, (1,) + nf.CONV_PIXEL[name], NAN)
    for T in nf.CONV_ITERS:
        clean = orc.conv_fista(x, z0, w, nf.ALPHA, stride=st, padding=pd, maxiter=T, lr=lr, tol=0.0)
        got = orc.conv_fista(xp, z0, w, nf.ALPHA, stride=st, padding=pd, maxiter=T, lr=lr, tol=0.0)
        assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
        reach = nf.conv_reach(name, T, x.shape[2:], z0.shape[2:])
        want = torch.where(reach, IS_NAN, FINITE).to(torch.int8).expand(z0.shape[1], -1, -1)
        assert torch.equal(classes(got[1]), want), (name, T)
        assert torch.equal(got[1][:, ~reach], clean[1][:, ~reach])            # outside the block: bitwise clean
        if name == "fused":     # the centre pixel of a 9 x 9 image under a 3 x 3 kernel: 3 x 3, 7 x 7, the clipped 11 x 11
            assert int(reach.sum()) == {1: 9, 2: 49, 3: 81}[T]
    if name == "bands":
        r1 = torch.nonzero(nf.conv_reach(name, 1, x.shape[2:], z0.shape[2:]).any(1)).flatten().tolist()
        assert r1 == [9, 10, 11]
    _, info = orc.conv_fista(xp, z0, w, nf.ALPHA, stride=st, padding=pd, maxiter=12, lr=lr, tol=1e-4, return_info=True)
    assert info["iterations"] == 12 and math.isnan(info["last_delta"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("n,d,k", nf.MSTEP_SHAPES)
def test_update_dict(n, d, k, positive, dtype):
    X, W, _, _ = nf.linear_problem(n, d, k, dtype=dtype)
    g = torch.Generator().manual_seed(5)
    Z = torch.randn(n, k, generator=g, dtype=dtype) * (torch.rand(n, k, generator=g) < 0.4)
    for what in ("Z", "X"):
        Zp = poison(Z, (n // 2, k // 2), NAN) if what == "Z" else Z.clone()
        Xp = poison(X, (n // 2, d - 1), NAN) if what == "X" else X
        D = orc.update_dict(W.clone(), Xp, Zp, positive=positive)
        # dict_learning.py:82: the residual row n // 2 is NaN, and every atom's update Z[:, j] @ R reads it (NaN * 0
        # is NaN); clamp_(0, None) keeps NaN (:87-88) and NaN < eps is False (:92)
        assert classes(D).eq(IS_NAN).all(), what
    for what in ("Z", "X"):
        Zp = poison(Z, (n // 2, k // 2), NAN) if what == "Z" else Z
        Xp = poison(X, (n // 2, d - 1), NAN) if what == "X" else X
        try:
            V = orc.update_dict_ridge(Xp, Zp, lambd=1e-2)
        except RuntimeError as e:            # linalg.cholesky refuses a Gram matrix it cannot factor
            assert what == "Z" and "cholesky" in str(e)
            continue
        assert V.shape == (d, k)
        if what == "X":                       # Z^T X: column d - 1 of the right-hand side is NaN, nothing else
            assert classes(V)[d - 1].eq(IS_NAN).all() and classes(V)[:d - 1].eq(FINITE).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bounds_and_objectives(dtype):
    x, w, z0, lr, st, pd = nf.conv_problem("synth", dtype=dtype)
    for value in (NAN, PINF):
        # lip_const.py:126-131: Inf * cos and Inf * sin of both signs meet in the matmul: NaN either way
        # (the reference's bound is float32 arithmetic whatever the kernel's dtype: its frequency grid is)
        assert math.isnan(orc.conv_lipschitz_bound(poison(w, (3, 2, 1, 1), value).float(), pd).item())
    with pytest.raises(RuntimeError, match="lambda must be"):      # lr='auto' on such a kernel: softshrink refuses 1 / NaN
        orc.conv_fista(x.float(), z0.float(), poison(w, (3, 2, 1, 1), NAN).float(), nf.ALPHA, padding=pd, maxiter=2, tol=0.0)
    z = orc.conv_fista(x, z0, w, nf.ALPHA, padding=pd, maxiter=2, lr=lr, tol=0.0)
    assert math.isnan(orc.conv_objective(poison(x, (1, 0, 0, 0), NAN), z, w, nf.ALPHA, st, pd).item())
    assert math.isnan(orc.conv_objective(x, poison(z, (1, 0, 0, 0), NAN), w, nf.ALPHA, st, pd).item())
    assert orc.conv_objective(poison(x, (1, 0, 0, 0), PINF), z, w, nf.ALPHA, st, pd).item() == PINF
    n, d, k = nf.LINEAR_FUSED[0]
    X, W, z0, lr = nf.linear_problem(n, d, k, dtype=dtype)
    Z = orc.fista(X, z0, W, nf.ALPHA, lr=lr, maxiter=2, tol=0.0)
    assert math.isnan(orc.lasso_objective(poison(X, (3, 2), NAN), Z, W, nf.ALPHA).item())
    assert math.isnan(orc.lasso_objective(X, poison(Z, (3, 2), NAN), W, nf.ALPHA).item())
    assert orc.lasso_objective(poison(X, (3, 2), NINF), Z, W, nf.ALPHA).item() == PINF
    assert orc.lasso_objective(X, poison(Z, (3, 2), PINF), W, nf.ALPHA).item() == PINF       # one Inf: no Inf - Inf
    # ista.py:8-14 has no value for such a dictionary: ARPACK cannot start on a Gram matrix with a NaN (Inf * W is NaN
    # somewhere in it), so the reference's lr='auto' raises before the first iteration -- and so does LAPACK in the
    # deterministic variant.  (The HIP path returns NaN instead: README "Non-finite inputs".)
    from scipy.sparse.linalg import ArpackError
    for value in (NAN, PINF):
        with pytest.raises(ArpackError):
            orc.lipschitz_constant(poison(W, (d - 1, 0), value).float())
        with pytest.raises(torch.linalg.LinAlgError):
            orc.lipschitz_constant(poison(W, (d - 1, 0), value), "exact")


def test_autograd_through_the_oracle_with_a_nan_cotangent():
    """torch.autograd through the unrolled loop: a NaN in row i of grad_z, at a coordinate whose code is not zero
    (softshrink's backward SELECTS: a zero code passes 0 whatever the cotangent), makes row i of dx and dz0 NaN through
    the row's products with W, leaves the other rows bitwise, and makes every dW NaN."""
    n, d, k = nf.LINEAR_FUSED[0]
    X, W, z0, lr = nf.linear_problem(n, d, k)
    g = torch.Generator().manual_seed(9)
    gz = torch.randn(n, k, generator=g)
    for T in (1, 6):
        col = nf.nonzero_column(orc.fista(X, z0, W, nf.ALPHA, lr=lr, maxiter=T, tol=0.0)[5])
        gzp = poison(gz, (5, col), NAN)
        grads = []
        for cot in (gz, gzp):
            xs, ws, zs = (t.clone().requires_grad_(True) for t in (X, W, z0))
            orc.fista(xs, zs, ws, nf.ALPHA, lr=lr, maxiter=T, tol=0.0).backward(cot)
            grads.append((xs.grad, zs.grad, ws.grad))
        (dx, dz0, dw), (dxp, dz0p, dwp) = grads
        rest = _others(n, [5])
        assert torch.equal(dxp[rest], dx[rest]) and torch.equal(dz0p[rest], dz0[rest])
        assert classes(dxp[5]).eq(IS_NAN).all() and classes(dz0p[5]).eq(IS_NAN).all()
        assert classes(dwp).eq(IS_NAN).all()


@pytest.mark.parametrize("center", [True, False])
def test_unfold_fold_carry_one_nan_pixel(center):
    """F.unfold / F.fold move values only: the NaN appears in exactly the 9 patches that hold the pixel -- in that one
    element of each, or, centred, in all of it (the patch's mean is NaN) -- and folding them back gives NaN at that
    pixel alone, or at every pixel those 9 patches cover."""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(2)
    img = poison(torch.randn(2, 1, 9, 10, generator=g), (1, 0, 4, 5), NAN)
    cols = F.unfold(img, 3)
    if center:
        cols = cols - cols.mean(1, keepdim=True)
    per_patch = cols.isnan().any(1) if not center else cols.isnan().all(1)
    assert int(per_patch[0].sum()) == 0 and int(per_patch[1].sum()) == 9
    back = F.fold(cols, (9, 10), 3)
    nanmap = back.isnan()
    want = torch.zeros(9, 10, dtype=torch.bool)
    if center:
        want[2:7, 3:8] = True
    else:
        want[4, 5] = True
    assert int(nanmap[0].sum()) == 0 and torch.equal(nanmap[1, 0], want)
