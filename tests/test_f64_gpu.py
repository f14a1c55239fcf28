"""float64 tensors on the HIP path (fp64-MFMA FISTA, loss, lr='auto', init='transpose') against the oracle run in
float64 on the CPU on the same seeded inputs.

The bar is the project's fp32 parity bar (max|dz| <= 5e-5, tests/test_fista_gpu.py) scaled by the ratio of the unit
round-offs: 5e-5 * 2^-29 = 9.3e-14.  A correct double kernel differs from the oracle by summation order only (the
float64 oracle against itself with atoms and features permuted: 5e-16 at 1 iteration .. 1.5e-14 at 1000), while
anything with a single-precision step inside is 3e-7 .. 3.6e-5 away.  Every test records the deviation it measured
(tests/margins.py)."""
import warnings

import numpy as np
import pytest
import torch

from recipes import recipe_xw, LAMBDA_MAX_C2

from margins import record_margins

pytestmark = pytest.mark.gpu

BAR = 5e-5 * 2.0 ** -29            # 9.3e-14
LOSS_RTOL = 2e-6 * 2.0 ** -29      # 3.7e-15: the fp32 loss test's bar, scaled the same way

SHAPES = [(37, 10, 50), (64, 256, 1024), (100, 48, 200), (1, 3, 2), (257, 256, 1000), (33, 200, 513),
          (65, 65, 256), (50, 300, 40), (33, 64, 1500), (20, 784, 1100)]


def _orc():
    from oracle import lasso_oracle as orc
    return orc


def xw64(n, d, k, seed=0):
    X, W = recipe_xw(n, d, k, seed)
    return X.double(), W.double()


def step_for(W):
    return 1.0 / _orc().lipschitz_constant(W, "exact")


def check(name, got, ref):
    assert got.dtype is torch.float64 and tuple(got.shape) == tuple(ref.shape)
    err = (got.cpu() - ref).abs().max().item() if ref.numel() else 0.0
    record_margins(name, dict(max_abs_dz=err, bar=BAR))
    print("%s: max|dz| = %.3g (bar %.3g)" % (name, err, BAR))
    assert err <= BAR, (name, err)
    return err


# 1 -- fixed step -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxiter", [1, 7, 30])
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_fixed_step_matches_float64_oracle(n, d, k, fast, maxiter):
    from lasso_amd.linear.solvers import ista
    orc = _orc()
    X, W = xw64(n, d, k)
    lr = step_for(W)
    z0 = X.new_zeros(n, k)
    ref = orc.fista(X, z0, W, 0.3, fast=fast, lr=lr, maxiter=maxiter, tol=0.0)
    got = ista(X.cuda(), z0.cuda(), W.cuda(), 0.3, fast=fast, lr=lr, maxiter=maxiter, tol=0.0)
    assert got.is_cuda
    check("f64_fixed_%dx%dx%d_%s_M%d" % (n, d, k, "fista" if fast else "ista", maxiter), got, ref)


def test_fixed_step_nonzero_z0_strided_x_cpu_inputs_and_empty_batch():
    from lasso_amd.linear import sparse_encode
    from lasso_amd.linear.solvers import ista
    orc = _orc()
    X, W = xw64(33, 200, 513)
    lr = step_for(W)
    g = torch.Generator().manual_seed(5)
    z0 = 0.1 * torch.randn(33, 513, generator=g, dtype=torch.float64)
    ref = orc.fista(X, z0, W, 0.3, lr=lr, maxiter=7, tol=0.0)
    z0g = z0.cuda()
    got = ista(X.cuda(), z0g, W.cuda(), 0.3, lr=lr, maxiter=7, tol=0.0)
    check("f64_fixed_z0", got, ref)
    assert torch.equal(z0g.cpu(), z0)                              # inputs are never modified
    # a non-contiguous x: a column slice of a wider matrix
    wide = torch.randn(33, 260, generator=g, dtype=torch.float64)
    Xs = wide[:, 30:230]
    assert not Xs.is_contiguous()
    ref = orc.fista(Xs, z0, W, 0.3, lr=lr, maxiter=7, tol=0.0)
    got = ista(wide.cuda()[:, 30:230], z0.cuda(), W.cuda(), 0.3, lr=lr, maxiter=7, tol=0.0)
    check("f64_fixed_strided_x", got, ref)
    # CPU tensors are staged through the device; the result comes back where z0 lives
    ref = orc.sparse_encode(X, W, alpha=0.3, lr=lr, maxiter=7, tol=0.0)
    got = sparse_encode(X, W, alpha=0.3, lr=lr, maxiter=7, tol=0.0)
    assert not got.is_cuda
    check("f64_fixed_cpu_inputs", got, ref)
    # the sparse_encode boundary on device tensors (zero init through the lazy_zeros sentinel)
    got = sparse_encode(X.cuda(), W.cuda(), alpha=0.3, lr=lr, maxiter=7, tol=0.0)
    assert got.is_cuda
    check("f64_fixed_sparse_encode", got, ref)
    # maxiter = 0 returns z0 itself
    assert ista(X.cuda(), z0g, W.cuda(), 0.3, lr=lr, maxiter=0) is z0g
    # n = 0
    empty = sparse_encode(X[:0].cuda(), W.cuda(), alpha=0.3, lr=lr, maxiter=7, tol=0.0)
    assert empty.dtype is torch.float64 and tuple(empty.shape) == (0, 513) and empty.is_cuda


# 2 -- long runs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxiter", [100, 1000])
def test_long_runs_stay_inside_the_bar(maxiter):
    from lasso_amd.linear.solvers import ista
    orc = _orc()
    X, W = xw64(64, 256, 1024)
    lr = step_for(W)
    z0 = X.new_zeros(64, 1024)
    ref = orc.fista(X, z0, W, 0.3, lr=lr, maxiter=maxiter, tol=0.0)
    got = ista(X.cuda(), z0.cuda(), W.cuda(), 0.3, lr=lr, maxiter=maxiter, tol=0.0)
    check("f64_long_M%d" % maxiter, got, ref)


# 3 -- stop rule --------------------------------------------------------------------------------------------------
def test_stop_rule_fires_at_the_oracles_iteration():
    from lasso_amd.linear.solvers import ista
    orc = _orc()
    X, W = xw64(256, 256, 1024)
    lr = 1.0 / LAMBDA_MAX_C2
    z0 = X.new_zeros(256, 1024)
    trace = orc.FistaTrace()
    ref = orc.fista(X, z0, W, 0.5, lr=lr, maxiter=2000, tol=1e-5, trace=trace)
    assert trace.stopped and trace.iterations == 263               # (the decision has a relative margin of 2e-4)
    got, info = ista(X.cuda(), z0.cuda(), W.cuda(), 0.5, lr=lr, maxiter=2000, tol=1e-5, return_info=True)
    print("iterations %d (oracle %d), last sum %.17g (oracle %.17g)" % (info['iterations'], trace.iterations,
                                                                        info['last_delta'], trace.delta[-1]))
    assert info['iterations'] == trace.iterations
    assert isinstance(info['last_delta'], float)
    # (two codes within BAR of the oracle's, element by element: their sums |z - z_next| differ by <= 2 n k BAR)
    assert abs(info['last_delta'] - trace.delta[-1]) <= 2 * 256 * 1024 * BAR
    assert info['last_delta'] <= 256 * 1024 * 1e-5
    record_margins("f64_stop_rule", dict(iterations=info['iterations'], last_delta=info['last_delta'],
                                         oracle_last_delta=trace.delta[-1]))
    check("f64_stop_rule_code", got, ref)
    got2, info2 = ista(X.cuda(), z0.cuda(), W.cuda(), 0.5, lr=lr, maxiter=2000, tol=1e-5, return_info=True,
                       stop_mode='chunked')
    assert info2['iterations'] == info['iterations'] and torch.equal(got2, got)
    # stop_mode='none' runs every iteration
    got3, info3 = ista(X.cuda()[:16], z0.cuda()[:16], W.cuda(), 0.5, lr=lr, maxiter=12, tol=1e-1, return_info=True,
                       stop_mode='none')
    assert info3['iterations'] == 12


# 4 -- lr='auto' --------------------------------------------------------------------------------------------------
def test_lipschitz_constant_of_a_float64_dictionary_and_lr_auto():
    from lasso_amd.linear import sparse_encode
    from lasso_amd.linear.lipschitz import lipschitz_constant
    orc = _orc()
    X, W = xw64(64, 256, 1024)
    L = lipschitz_constant(W.cuda())
    print("lambda_max %.17g (recipe constant %.17g)" % (L, LAMBDA_MAX_C2))
    assert isinstance(L, float)
    assert abs(L - LAMBDA_MAX_C2) <= 1e-9 * LAMBDA_MAX_C2
    assert lipschitz_constant(W.cuda()) == L                       # bitwise reproducible
    g = torch.Generator().manual_seed(3)
    worst = 0.0
    for d, k in [(10, 50), (50, 10), (64, 256), (200, 513), (3, 2), (256, 100)]:
        Wr = torch.randn(d, k, generator=g).double()
        ref = orc.lipschitz_constant(Wr, "exact")
        got = lipschitz_constant(Wr.cuda())
        worst = max(worst, abs(got - ref) / ref)
        assert abs(got - ref) <= 2e-6 * ref, (d, k, got, ref)
    record_margins("f64_lipschitz", dict(recipe_rel=abs(L - LAMBDA_MAX_C2) / LAMBDA_MAX_C2, ragged_worst_rel=worst))
    with pytest.raises(TypeError):                                   # bf16 keeps its TypeError (ista.py:12)
        lipschitz_constant(W.bfloat16().cuda())
    ref = orc.sparse_encode(X, W, alpha=0.3, lr=1.0 / L, maxiter=30, tol=0.0)
    got = sparse_encode(X.cuda(), W.cuda(), alpha=0.3, lr='auto', maxiter=30, tol=0.0)
    check("f64_lr_auto", got, ref)


# 5 -- line search ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k,maxiter,alpha", [(256, 256, 1024, 10, 0.5), (50, 300, 1500, 5, 0.5)])
def test_line_search_takes_the_oracles_decisions(n, d, k, maxiter, alpha):
    from lasso_amd.linear.solvers import ista
    orc = _orc()
    X, W = xw64(n, d, k)
    z0 = X.new_zeros(n, k)
    trace = orc.FistaTrace()
    ref = orc.fista(X, z0, W, alpha, lr=1.0, maxiter=maxiter, tol=0.0, backtrack=True, trace=trace)
    if (n, d, k) == (256, 256, 1024):
        assert trace.trials == [5, 3, 5, 4, 4, 4, 4, 3, 4, 4]
    got, info = ista(X.cuda(), z0.cuda(), W.cuda(), alpha, lr=1.0, maxiter=maxiter, tol=0.0, backtrack=True,
                     return_info=True)
    print("trials", info['trials'], "oracle", trace.trials)
    assert info['iterations'] == maxiter
    assert info['trials'] == trace.trials
    assert info['accepted_lr'] == trace.accepted_lr                # the same chain of double divisions lr / eta
    assert all(isinstance(v, float) for v in info['accepted_lr'] + info['accepted_f'])
    check("f64_line_search_%dx%dx%d" % (n, d, k), got, ref)


def test_line_search_that_cannot_succeed_warns_and_reverts_to_lr0():
    """ista.py:48-52: after 1000 refused trials the iteration takes the step lr0 and the solve warns.  eta = 1.0001
    shrinks a step of 2 (more than ten times 1 / lambda_max here) to 1.81 in 1000 trials: F <= Q never holds, every
    value stays finite, and the oracle takes the same road."""
    from lasso_amd.linear.solvers import ista
    orc = _orc()
    X, W = xw64(16, 32, 64)
    z0 = X.new_zeros(16, 64)
    trace = orc.FistaTrace()
    with pytest.warns(UserWarning, match="line search failed"):
        ref = orc.fista(X, z0, W, 0.5, lr=2.0, maxiter=2, tol=0.0, backtrack=True, eta_backtrack=1.0001, trace=trace)
    assert trace.trials == [1000, 1000] and trace.accepted_lr == [2.0, 2.0]
    with pytest.warns(UserWarning, match="line search failed"):
        got, info = ista(X.cuda(), z0.cuda(), W.cuda(), 0.5, lr=2.0, maxiter=2, tol=0.0, backtrack=True,
                         eta_backtrack=1.0001, return_info=True)
    assert info['iterations'] == 2 and info['trials'] == trace.trials and info['accepted_lr'] == trace.accepted_lr
    assert bool(torch.isfinite(got).all())
    # the bar is set for codes of max|z| ~ 4 (5e-5 * 2^-29 absolute); steps this long give larger entries, and a
    # rounding error scales with the value it belongs to
    scale = max(1.0, ref.abs().max().item() / 4.0)
    err = (got.cpu() - ref).abs().max().item()
    record_margins("f64_line_search_revert", dict(max_abs_dz=err, bar=BAR * scale, max_abs_z=ref.abs().max().item()))
    print("revert: max|dz| = %.3g, max|z| = %.3g (bar %.3g)" % (err, ref.abs().max().item(), BAR * scale))
    assert err <= BAR * scale


# 6 -- objective --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k", [(37, 10, 50), (64, 256, 1024), (100, 48, 200), (1000, 64, 256),
                                   (90, 300, 40), (50, 64, 1500), (130, 784, 1100)])
def test_lasso_loss_in_double(n, d, k):
    from lasso_amd.linear import lasso_loss
    orc = _orc()
    g = torch.Generator().manual_seed(n)
    X, W = torch.randn(n, d, generator=g).double(), torch.randn(d, k, generator=g).double()
    Z = (torch.randn(n, k, generator=g) * (torch.rand(n, k, generator=g) < 0.2)).double()
    ref = orc.lasso_objective(X, Z, W, 0.7).item()
    got = lasso_loss(X.cuda(), Z.cuda(), W.cuda(), 0.7)
    assert got.dim() == 0 and got.is_cuda and got.dtype is torch.float64
    rel = abs(got.item() - ref) / abs(ref)
    record_margins("f64_lasso_loss_%dx%dx%d" % (n, d, k), dict(rel=rel, bar=LOSS_RTOL))
    print("loss %.17g oracle %.17g rel %.3g (bar %.3g)" % (got.item(), ref, rel, LOSS_RTOL))
    assert abs(got.item() - ref) <= LOSS_RTOL * abs(ref)


def test_return_info_objective_agrees_with_lasso_loss():
    from lasso_amd.linear import lasso_loss
    from lasso_amd.linear.solvers import ista
    X, W = xw64(64, 256, 1024)
    Xg, Wg = X.cuda(), W.cuda()
    z, info = ista(Xg, Xg.new_zeros(64, 1024), Wg, 0.3, lr=step_for(W), maxiter=10, tol=0.0, return_info='objective')
    loss = lasso_loss(Xg, z, Wg, 0.3).item()
    assert isinstance(info['objective'], float)
    assert abs(info['objective'] - loss) <= LOSS_RTOL * abs(loss)
    ref = _orc().lasso_objective(X, z.cpu(), W, 0.3).item()
    assert abs(info['objective'] - ref) <= LOSS_RTOL * abs(ref)


# 7 -- init='transpose' -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k", [(37, 10, 50), (64, 256, 1024), (33, 200, 513), (1, 3, 2), (20, 784, 1100)])
def test_init_transpose_in_double(n, d, k):
    from lasso_amd.linear.sparse_encode import initialize_code
    X, W = xw64(n, d, k)
    ref = X @ W
    bound = d * 2.0 ** -53 * (X.abs() @ W.abs())                    # the standard dot-product bound
    for xin, win in ((X.cuda(), W.cuda()), (X, W)):
        got = initialize_code(xin, win, 1.0, 'transpose')
        assert got.dtype is torch.float64 and got.device == xin.device and tuple(got.shape) == (n, k)
        err = (got.cpu() - ref).abs()
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        record_margins("f64_init_transpose_%dx%dx%d" % (n, d, k), dict(worst_error_over_bound=ratio))
        assert bool((err <= bound).all()), ratio


# 8 -- refusals ---------------------------------------------------------------------------------------------------
def test_float64_refusals_name_the_argument():
    from lasso_amd.linear.solvers import ista
    X, W = xw64(16, 32, 64)
    Xg, Wg = X.cuda(), W.cuda()
    z0 = Xg.new_zeros(16, 64)
    with pytest.raises(NotImplementedError, match="verbose"):
        ista(Xg, z0, Wg, 0.3, lr=0.1, verbose=True)
    with pytest.raises(NotImplementedError, match="begin"):
        ista(Xg, z0, Wg, 0.3, lr=0.1, begin=True)
    with pytest.raises(NotImplementedError, match="shard"):
        ista(Xg, z0, Wg, 0.3, lr=0.1, shard=True)
    for kernel in ('tile', 'splitk'):
        with pytest.raises(NotImplementedError, match="kernel"):
            ista(Xg, z0, Wg, 0.3, lr=0.1, kernel=kernel)
    Wr = Wg.clone().requires_grad_(True)
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="requires_grad"):
            ista(Xg, z0, Wr, 0.3, lr=0.1)
    with torch.no_grad():                                            # ... and the same tensors solve under no_grad
        assert ista(Xg, z0, Wr, 0.3, lr=0.1, maxiter=2).dtype is torch.float64
    with pytest.raises(RuntimeError):
        ista(Xg, z0, Wg.float(), 0.3, lr=0.1)
    with pytest.raises(ValueError):                                  # ista.py:18-19
        ista(Xg, z0, Wg, 0.3, lr=0.1, backtrack=True, eta_backtrack=1.0)


def test_other_entry_points_refuse_float64_tensors():
    """the C ABI: every entry point outside the float64 list answers LASSO_ERR_UNSUPPORTED for LASSO_F64 instead of
    reading doubles as floats"""
    import ctypes as C
    from lasso_amd import _native as nat
    L = nat.lib()
    n, d, k = 16, 32, 64
    X, W = xw64(n, d, k)
    Xg, Wg = X.cuda(), W.cuda()
    Z = Xg.new_zeros(n, k)
    ws = torch.empty(1 << 24, dtype=torch.uint8, device='cuda')
    st = nat.stream_ptr(Xg.device)
    F64, UNS = nat.LASSO_F64, nat.LASSO_ERR_UNSUPPORTED
    A = torch.zeros(k * k + k * d, device='cuda')
    assert L.lasso_fista_prepare(nat.ptr(Wg), k, d, k, F64, 4, nat.ptr(ws), ws.numel(), st) == UNS
    assert L.lasso_fista_run(nat.ptr(Xg), d, nat.ptr(Z), k, None, 0, nat.ptr(Z), k, None, 0, n, d, k, F64, 0.3, 0.1, 1, 0,
                             1, 4, 0, None, nat.ptr(ws), ws.numel(), st) == UNS
    assert L.lasso_gram_accumulate(nat.ptr(Z), k, nat.ptr(Xg), d, n, d, k, F64, nat.ptr(A), nat.ptr(A), nat.ptr(ws),
                                   ws.numel(), st) == UNS
    assert L.lasso_cd_prepare(nat.ptr(Xg), d, nat.ptr(Wg), k, None, 0, n, d, k, F64, nat.ptr(ws), ws.numel(), st) == UNS
    assert L.lasso_fista_backward(nat.ptr(Xg), d, nat.ptr(Wg), k, nat.ptr(Z), nat.ptr(Z), n, d, k, F64, 0.1, 1, 1,
                                  None, None, nat.ptr(Z), nat.ptr(ws), ws.numel(), st) == UNS
    assert L.lasso_ridge_solve(nat.ptr(A), nat.ptr(A), nat.ptr(Wg), k, d, k, F64, 0.1, None, nat.ptr(ws), ws.numel(),
                               st) == UNS
    assert L.lasso_zero_columns(nat.ptr(Z), k, n, k, F64, nat.ptr(ws), st) == UNS
    # asynchronous / sharded flags and the fused-kernel hints with float64 tensors
    for flags in (nat.SOLVE_ASYNC, nat.SOLVE_ASYNC | nat.SOLVE_SHARDED, nat.KERNEL_TILE, nat.KERNEL_SPLITK):
        assert L.lasso_fista_solve(nat.ptr(Xg), d, nat.ptr(Wg), k, None, 0, nat.ptr(Z), k, n, d, k, F64, 0.3, 0.1, 1, 3,
                                   0.0, flags, 0, 1.5, None, None, None, None, None, None, nat.ptr(ws), ws.numel(),
                                   st) == UNS
    torch.cuda.synchronize()


def test_lasso_fista_solve_accepts_f64_and_rounds_its_float_slots():
    """lasso_fista_solve with LASSO_F64 is the same solve as lasso_fista_solve_f64: same code bit for bit, the float
    slots hold the doubles rounded once"""
    import ctypes as C
    from lasso_amd import _native as nat
    from lasso_amd.linear.solvers import ista
    L = nat.lib()
    n, d, k = 40, 70, 130
    X, W = xw64(n, d, k)
    Xg, Wg = X.cuda(), W.cuda()
    lr = step_for(W)
    ref, info = ista(Xg, Xg.new_zeros(n, k), Wg, 0.3, lr=lr, maxiter=40, tol=1e-3, return_info='objective')
    z = torch.empty(n, k, dtype=torch.float64, device='cuda')
    nbytes = L.lasso_fista_workspace_bytes(n, d, k, nat.LASSO_F64, 40, 1e-3, nat.STOP_GLOBAL, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    iters, last, obj = C.c_int32(0), C.c_float(0.0), C.c_float(0.0)
    nat.check(L.lasso_fista_solve(nat.ptr(Xg), d, nat.ptr(Wg), k, None, 0, nat.ptr(z), k, n, d, k, nat.LASSO_F64, 0.3, lr,
                                  1, 40, 1e-3, nat.STOP_GLOBAL, 0, 1.5, C.byref(iters), C.byref(last), None, None, None,
                                  C.byref(obj), nat.ptr(ws), ws.numel(), nat.stream_ptr(Xg.device)))
    assert torch.equal(z, ref) and iters.value == info['iterations']
    assert last.value == np.float32(info['last_delta']) and obj.value == np.float32(info['objective'])
    # lasso_objective / lasso_objective_throttled with LASSO_F64: the double loss rounded once into their float slot,
    # the two sums as doubles
    from lasso_amd.linear import lasso_loss
    want = lasso_loss(Xg, ref, Wg, 0.3).item()
    ows = torch.empty(L.lasso_objective_f64_workspace_bytes(n, d, k), dtype=torch.uint8, device='cuda')
    for throttled in (False, True):
        loss32 = torch.zeros((), dtype=torch.float32, device='cuda')
        sums = torch.zeros(2, dtype=torch.float64, device='cuda')
        head = (nat.ptr(Xg), d, nat.ptr(Wg), k, nat.ptr(ref), k, n, d, k, nat.LASSO_F64, 0.3, nat.ptr(loss32), nat.ptr(sums))
        tail = (nat.ptr(ows), ows.numel(), nat.stream_ptr(Xg.device))
        nat.check(L.lasso_objective_throttled(*head, 8, *tail) if throttled else L.lasso_objective(*head, *tail))
        assert loss32.item() == np.float32(want)
        rss, l1 = sums.tolist()
        assert (0.5 * rss + 0.3 * l1) / n == want


def test_objective_sums_refuses_a_float32_loss_slot_for_float64_tensors():
    from lasso_amd.engine import HipEngine
    X, W = xw64(16, 32, 64)
    Xg, Wg = X.cuda(), W.cuda()
    Z = Xg.new_zeros(16, 64)
    eng = HipEngine(Xg.device)
    with pytest.raises(RuntimeError, match="loss_out"):
        eng.objective_sums(Xg, Z, Wg, 0.5, loss_out=torch.zeros((), device='cuda'))
    slot = torch.zeros(3, dtype=torch.float64, device='cuda')
    loss, _ = eng.objective_sums(Xg, Z, Wg, 0.5, loss_out=slot[1])
    want = 0.5 * X.pow(2).sum().item() / 16                          # Z = 0: the loss is 0.5 ||X||^2 / n
    assert loss.dtype is torch.float64 and abs(slot[1].item() - want) <= LOSS_RTOL * want
    assert slot[0].item() == 0.0 and slot[2].item() == 0.0
    # an empty batch: nothing is launched, the caller's slot says 0 / 0 like the reference
    eng.objective_sums(Xg[:0], Z[:0], Wg, 0.5, loss_out=slot[2])
    assert bool(torch.isnan(slot[2]))


# 9 -- determinism ------------------------------------------------------------------------------------------------
def test_float64_solves_are_bitwise_reproducible():
    from lasso_amd.linear.solvers import ista
    X, W = xw64(257, 256, 1000)
    Xg, Wg = X.cuda(), W.cuda()
    z0 = Xg.new_zeros(257, 1000)
    lr = step_for(W)
    a = ista(Xg, z0, Wg, 0.3, lr=lr, maxiter=30, tol=0.0)
    b = ista(Xg, z0, Wg, 0.3, lr=lr, maxiter=30, tol=0.0)
    assert torch.equal(a, b)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a, ia = ista(Xg, z0, Wg, 0.5, lr=1.0, maxiter=6, tol=0.0, backtrack=True, return_info=True)
        b, ib = ista(Xg, z0, Wg, 0.5, lr=1.0, maxiter=6, tol=0.0, backtrack=True, return_info=True)
    assert torch.equal(a, b) and ia == ib


# reference pinning -----------------------------------------------------------------------------------------------
def test_hip_path_reproduces_the_references_float64_codes(golden):
    """tests/golden/f64_cases.npz: float64 codes of the REAL reference (generate_golden_f64.py)"""
    from lasso_amd.linear.solvers import ista
    from golden_f64 import CASES, case_inputs
    g = golden("f64_cases")
    for tag, case in CASES.items():
        X, W, z0, kw = case_inputs(case, lr=float(g[tag + "_lr"]))
        got = ista(X.cuda(), z0.cuda(), W.cuda(), case["alpha"], **kw)
        check("f64_golden_" + tag, got, torch.from_numpy(g[tag + "_z"]))
