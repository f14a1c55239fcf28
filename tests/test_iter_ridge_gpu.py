"""iterative_ridge on the GPU against the reference's recorded runs (tests/golden/iter_ridge_cases.npz), the host model
(tests/iter_ridge_model.py) and, for the row kernel alone, a float64 solve of each row's compacted system.

Bars.  Codes: max|z - z_ref32| <= max(5e-5, 4 x spread_z), where spread_z is how far "another correct float32
implementation" (the model with permuted supports and summation orders) moved the codes when the fixture was made; the
factor 4 and the 5e-5 floor are the project's rule (tests/test_gpsr_gpu.py).  A case is compared by its codes only if
spread_z <= 2.5e-3.  Several Brent iterations are compared by objective only (tests/iter_ridge_cases.py says why):
max(1e-6, 4 x spread_f).  The row kernel: 4 x e_ref and never below 8 float32 ulp, where e_ref is the relative
infinity-norm error of torch's own float32 cholesky_ex + cholesky_solve on the reference's masked full-size system,
measured by the test on the CPU against the same double solve.  Fresh shapes: 4 x the model's float32 / float64 gap,
after asserting that no stop decision of the model is within 1 % of tol."""
import contextlib
import ctypes as C
import io
import warnings

import numpy as np
import pytest
import torch

import iter_ridge_model
from gpsr_cases import same_line
from iter_ridge_cases import CASES, admitted_f, admitted_z, case_inputs, load_case, ridge_start, rtol_of
from margins import record_margins
from recipes import recipe_xw

pytestmark = pytest.mark.gpu
EPS = float(torch.finfo(torch.float32).eps)
LDS_CAP = 256                                     # largest support of the row kernel's LDS tier


@pytest.fixture(scope="module")
def cases(golden):
    return golden("iter_ridge_cases")


def run(z0, x, w, **kw):
    """-> (z on the CPU, info, warnings, printed text); inputs go to the GPU and must come back bitwise unchanged"""
    from lasso_amd.linear.solvers import iterative_ridge
    wg, xg, zg = w.cuda(), x.cuda(), z0.cuda()
    out = io.StringIO()
    with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(out):
        warnings.simplefilter("always")
        z, info = iterative_ridge(zg, xg, wg, return_info=True, **kw)
    assert z.is_cuda and z.dtype == x.dtype and z.data_ptr() != zg.data_ptr()
    assert torch.equal(wg.cpu(), w) and torch.equal(xg.cpu(), x) and torch.equal(zg.cpu(), z0)
    return z.cpu(), info, [str(c.message) for c in caught], out.getvalue()


def objective64(z, x, w, alpha):
    zd = z.double()
    return float(0.5 * (zd @ w.double().T - x.double()).pow(2).sum() + alpha * zd.abs().sum())


def pitched(t, ld, fill=777.0):
    """a device copy of t [rows, cols] with row pitch ld, 4 bytes off a 16-byte boundary -> (view, buffer)"""
    rows, cols = t.shape
    buf = torch.full((rows * ld + 5,), fill, dtype=torch.float32, device="cuda")
    view = buf[1:1 + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view, buf


def abi_solve(z0, x, w, alpha, maxiter, line_search=False, tol=1e-5, tikhonov=1e-4, eps=EPS, reserved=0, pitches=None):
    """lasso_iter_ridge_solve directly: `reserved` and pitched / offset operands are not reachable from Python.
    pitches = (ldx, ldw, ldz0, ldz) or None (packed) -> (status, z on the CPU, result struct, the buffers)"""
    from lasso_amd import _native as nat
    n, d = x.shape
    k = w.shape[1]
    ldx, ldw, ldz0, ldz = pitches or (d, k, k, k)
    (xv, xb), (wv, wb), (z0v, z0b) = pitched(x, ldx), pitched(w, ldw), pitched(z0, ldz0)
    zv, zb = pitched(torch.zeros(n, k), ldz)
    zb.fill_(-555.0)
    opts = nat.IterRidgeOptions(maxiter, int(line_search), tol, tikhonov, eps, reserved)
    res = nat.IterRidgeResult()
    cap = max(maxiter, 1)                                     # the per-iteration trace -> res.fval, res.support_max
    f_arr, u_arr, t_arr, sm_arr = ((C.c_double * cap)() for _ in range(4))
    ls_arr, sx_arr = (C.c_int32 * cap)(), (C.c_int32 * cap)()
    trace = nat.IterRidgeTrace(cap, 0, f_arr, u_arr, t_arr, ls_arr, sx_arr, sm_arr, None, None, None, 0)
    res.trace = C.pointer(trace)
    L = nat.lib()
    ws = torch.empty(L.lasso_iter_ridge_workspace_bytes(n, d, k, nat.LASSO_F32), dtype=torch.uint8, device="cuda")
    status = L.lasso_iter_ridge_solve(C.c_void_p(xv.data_ptr()), ldx, C.c_void_p(wv.data_ptr()), ldw,
                                      C.c_void_p(z0v.data_ptr()), ldz0, C.c_void_p(zv.data_ptr()), ldz, n, d, k, nat.LASSO_F32,
                                      alpha, C.byref(opts), C.byref(res), nat.ptr(ws), ws.numel(),
                                      nat.stream_ptr(torch.device("cuda", 0)))
    torch.cuda.synchronize()
    its = min(res.n_iter, cap) if status == 0 else 0
    res.fval, res.support_max = list(f_arr[:its]), list(sx_arr[:its])
    return status, zv.cpu(), res, dict(x=(xb, x, ldx), w=(wb, w, ldw), z0=(z0b, z0, ldz0), z=(zb, None, ldz))


def abi_rows(g, rhs, z, alpha, tikhonov, eps=EPS):
    """lasso_iter_ridge_rows -> (z_sol on the CPU, bad_row, bad_minor, support_max)"""
    from lasso_amd import _native as nat
    n, k = z.shape
    gg, rg, zg = g.cuda().contiguous(), rhs.cuda().contiguous(), z.cuda().contiguous()
    out = torch.full((n, k), -555.0, device="cuda")
    bad_row, bad_minor, smax = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    L = nat.lib()
    ws = torch.empty(L.lasso_iter_ridge_workspace_bytes(n, 1, k, nat.LASSO_F32), dtype=torch.uint8, device="cuda")
    nat.check(L.lasso_iter_ridge_rows(nat.ptr(gg), k, nat.ptr(rg), k, nat.ptr(zg), k, nat.ptr(out), k, n, k, nat.LASSO_F32,
                                      alpha, tikhonov, eps, C.byref(bad_row), C.byref(bad_minor), C.byref(smax), nat.ptr(ws),
                                      ws.numel(), nat.stream_ptr(torch.device("cuda", 0))))
    torch.cuda.synchronize()
    assert torch.equal(zg.cpu(), z)
    return out.cpu(), bad_row.value, bad_minor.value, smax.value


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case(cases, name):
    spec, g = CASES[name], load_case(cases, name)
    x, w, z0 = case_inputs(spec)
    kw = spec["kwargs"]
    ls = kw.get("line_search", True)
    z, info, caught, text = run(z0, x, w, alpha=spec["alpha"], verbose=True, **kw)
    assert torch.isfinite(z).all()
    assert sorted(caught) == sorted(m for m in str(g["warnings"]).split("\n") if m)
    got_lines, want_lines = text.strip().split("\n"), str(g["stdout"]).strip().split("\n")
    assert len(got_lines) == len(want_lines)
    assert abs(info["fval"][-1] - objective64(z, x, w, spec["alpha"])) <= 2e-6 * info["fval"][-1]
    if spec["compare"] == "z":
        assert admitted_z(g)
        bar = max(5e-5, 4.0 * float(g["spread_z"]))
        assert bar <= 1e-2
        dz = float((z - torch.from_numpy(g["z32"])).abs().max())
        print("%s: max|dz| = %.3g (bar %.3g), supports %s" % (name, dz, bar, info["support_max"]))
        assert info["iterations"] == len(g["f32"])
        assert info["status"] == ("converged" if spec.get("stops") else "maxiter")
        # support counts of the new z: an entry within the bar of the threshold eps may fall on either side of it
        unsure = int((np.abs(g["z32"]) < bar + EPS).sum() - (np.abs(g["z32"]) < EPS).sum())
        assert abs(info["support_mean"][-1] - g["smean32"][-1]) <= unsure / spec["n"] + 1e-12
        if not ls:                                             # (exact zeros and O(1) codes: nothing near eps)
            assert info["support_max"] == list(g["smax32"])
            assert np.allclose(info["support_mean"], g["smean32"], rtol=0, atol=1e-12)
        rel = {}
        for key, got, want in (("fval", info["fval"], g["f32"]), ("update", info["update"], g["update32"]),
                               ("t", info["t"], g["t32"])):
            rel[key] = float(np.max(np.abs(np.array(got) - want) / np.abs(want)))
            print("%s: %s rel %.3g (rtol %.3g)" % (name, key, rel[key], rtol_of(g, key)))
        assert dz <= bar, (name, dz, bar)
        for key in rel:
            assert rel[key] <= rtol_of(g, key), (name, key, rel[key], rtol_of(g, key))
        for a, b in zip(got_lines, want_lines):
            assert same_line(a, b), (a, b)
        margins = dict(dz=dz, bar=bar, **rel)
    else:
        assert admitted_f(g)
        f_ref = float(g["f64"][-1])
        err = abs(info["fval"][-1] - f_ref) / f_ref
        bar = max(1e-6, 4.0 * float(g["spread_f"]))
        print("%s: objective rel %.3g (bar %.3g)" % (name, err, bar))
        objs = [info["f0"]] + info["fval"]
        assert all(b <= a * (1 + 1e-6) for a, b in zip(objs, objs[1:])), objs      # non-increasing over the Brent iterations
        assert err <= bar, (name, err, bar)
        import re
        for a, b in zip(got_lines, want_lines):                # the line formats; the figures are compared above
            assert re.sub(r"[-+]?\d+\.?\d*", "#", a) == re.sub(r"[-+]?\d+\.?\d*", "#", b), (a, b)
        margins = dict(objective_rel=err, bar=bar)
    if not ls:
        assert info["t"] == [1.0] * info["iterations"] and info["ls_evals"] == [0] * info["iterations"]
    record_margins("iter_ridge/" + name, margins)


@pytest.mark.parametrize("name", ["brent_1a", "brent_1b"])
def test_brent_evaluations_are_the_line_objective(name):
    spec = CASES[name]
    x, w, z0 = case_inputs(spec)
    z, info, _, _ = run(z0, x, w, alpha=spec["alpha"], **spec["kwargs"])
    evals = info["evaluations"]
    assert len(evals) == info["ls_evals"][0] and 5 <= len(evals) <= 60 and all(e[0] == 1 for e in evals)
    assert all(0.0 < e[1] < 10.0 for e in evals)
    xd, wd, zd = x.double(), w.double(), z0.double()
    z_sol, bad = iter_ridge_model.solve_rows(wd.T @ wd, xd @ wd, zd, spec["alpha"], 1e-4, EPS)
    assert bad is None
    p = z_sol - zd
    line64 = lambda t: float(0.5 * ((zd + t * p) @ wd.T - xd).pow(2).sum() + spec["alpha"] * (zd + t * p).abs().sum())  # noqa: E731
    want = np.array([line64(float(np.float32(t))) for _, t, _ in evals])      # (the step is applied as a float32)
    err = float(np.max(np.abs(np.array([f for _, _, f in evals]) - want) / want))
    print("%s: %d evaluations, rel %.3g (rtol 1e-7)" % (name, len(evals), err))
    record_margins("iter_ridge/evaluations_" + name, dict(rel=err, rtol=1e-7, count=len(evals)))
    assert err <= 1e-7
    best = min(reversed(evals), key=lambda e: e[2])          # (a tie goes to the later evaluation)
    assert info["t"][0] == best[1] and info["fval"][0] == best[2]


# ---- the row kernel alone ------------------------------------------------------------------------------------------------
def ragged_codes(n, k, sizes, seed):
    """row i has exactly sizes[i] entries with |z| >= eps at random positions, magnitudes log-uniform in [1e-6, 3] (the
    diagonal spans six decades); the rest holds exact zeros and values in (0, eps)"""
    g = torch.Generator().manual_seed(seed)
    z = torch.zeros(n, k)
    small = torch.rand(n, k, generator=g) * (0.99 * EPS)
    z = torch.where(torch.rand(n, k, generator=g) < 0.5, small, z)
    for i, s in enumerate(sizes):
        pos = torch.randperm(k, generator=g)[:s]
        mag = torch.exp(torch.rand(s, generator=g) * (np.log(3.0) - np.log(1e-6)) + np.log(1e-6))
        sign = torch.where(torch.rand(s, generator=g) < 0.5, -1.0, 1.0)
        z[i, pos] = (mag * sign).float()
    assert [int(c) for c in (~(z.abs() < EPS)).sum(1)] == list(sizes)
    return z


def check_rows(tag, d, k, sizes, alpha=2.0, tikhonov=1e-4, seed=0):
    n = len(sizes)
    x, w = recipe_xw(n, d, k, seed=seed)
    g32 = w.T @ w
    g32 = torch.tril(g32) + torch.tril(g32, -1).T
    rhs = x @ w
    z = ragged_codes(n, k, sizes, seed + 100)
    got, bad_row, bad_minor, smax = abi_rows(g32, rhs, z, alpha, tikhonov)
    assert (bad_row, bad_minor) == (-1, 0) and smax == max(sizes)
    mask = z.abs() < EPS
    assert (got[mask] == 0).all()                            # masked entries are exact zeros
    # the yardstick: each row's compacted system in double; e_ref: torch's float32 Cholesky on the masked full-size system
    want, _ = iter_ridge_model.solve_rows(g32.double(), rhs.double(), z.double(), alpha, tikhonov, EPS)
    a = g32.expand(n, -1, -1).masked_fill(mask.unsqueeze(1) | mask.unsqueeze(2), 0.)
    a.diagonal(dim1=1, dim2=2).add_((alpha / z.abs()).masked_fill(mask, 0) + tikhonov)
    chol, info = torch.linalg.cholesky_ex(a)
    assert bool((info == 0).all())
    ref32 = torch.cholesky_solve(rhs.masked_fill(mask, 0.).unsqueeze(2), chol).squeeze(2)
    scale = want.abs().amax(1).clamp_min(1e-300)
    e_ref = float(((ref32.double() - want).abs().amax(1) / scale).max())
    err = float(((got.double() - want).abs().amax(1) / scale).max())
    bar = max(4.0 * e_ref, 8 * EPS)
    print("rows %s: err %.3g, e_ref %.3g, bar %.3g" % (tag, err, e_ref, bar))
    record_margins("iter_ridge/rows_" + tag, dict(err=err, e_ref=e_ref, bar=bar))
    assert err <= bar, (tag, err, e_ref)


@pytest.mark.parametrize("d", [210, 64])
def test_rows_every_support_size_up_to_200(d):
    check_rows("k200_d%d" % d, d, 200, list(range(201)))


def test_rows_around_the_lds_cap():
    check_rows("k300", 330, 300, [0, 1, LDS_CAP - 1, LDS_CAP, LDS_CAP + 1, 300], alpha=4.0)


def test_rows_small_odd():
    check_rows("k27", 45, 27, [27, 0, 13, 1, 26])


# ---- properties ----------------------------------------------------------------------------------------------------------
def test_zero_start_converges_at_once():
    x, w = recipe_xw(33, 40, 24, seed=0)
    for ls in (False, True):
        z, info, _, _ = run(torch.zeros(33, 24), x, w, alpha=2.0, line_search=ls)
        assert not z.any() and info["iterations"] == 1 and info["status"] == "converged"
        assert info["support_max"] == [0]


@pytest.mark.parametrize("line_search", [False, True])
def test_masked_entries_inputs_and_repeatability(line_search):
    spec = CASES["warm"]
    x, w, z0 = case_inputs(spec)
    z0 = torch.where((z0 == 0) & (torch.rand(z0.shape, generator=torch.Generator().manual_seed(3)) < 0.5),
                     torch.full_like(z0, 0.5 * EPS), z0)       # masked entries that are not zero keep their bits too
    a = run(z0, x, w, alpha=2.0, line_search=line_search, maxiter=3)
    b = run(z0, x, w, alpha=2.0, line_search=line_search, maxiter=3)
    assert torch.equal(a[0], b[0]) and a[1] == b[1]          # two solves are bitwise equal
    mask = z0.abs() < EPS
    assert mask.any() and torch.equal(a[0][mask], z0[mask])
    assert a[1]["iterations"] == 3
    if line_search:
        objs = [a[1]["f0"]] + a[1]["fval"]
        assert all(q <= p * (1 + 1e-6) for p, q in zip(objs, objs[1:])), objs


def test_tikhonov_zero_and_the_small_tikhonov_warning():
    spec = CASES["wide"]
    x, w, z0 = case_inputs(spec)
    z, info, caught, _ = run(z0, x, w, alpha=3.0, tikhonov=0.0, line_search=False, maxiter=3)
    assert torch.isfinite(z).all() and info["iterations"] == 3
    assert caught == ['small regularization value 0.0000e+00 may lead to inprecise results.']
    _, _, caught, _ = run(z0, x, w, alpha=3.0, tikhonov=1e-6, line_search=False, maxiter=1)
    assert caught == ['small regularization value 1.0000e-06 may lead to inprecise results.']
    _, _, caught, _ = run(z0, x, w, alpha=3.0, line_search=False, maxiter=1)
    assert caught == []


def test_nan_in_the_start_is_reported_by_row():
    from lasso_amd.linear.solvers import iterative_ridge
    x, w, z0 = case_inputs(CASES["small"])
    z0 = z0.clone()
    z0[7, 3] = float("nan")
    with pytest.raises(torch.linalg.LinAlgError, match="row 7 "):
        iterative_ridge(z0.cuda(), x.cuda(), w.cuda(), alpha=2.0, line_search=False, maxiter=2)
    torch.cuda.synchronize()                                  # a clean status: the device is usable
    z, info, _, _ = run(case_inputs(CASES["small"])[2], x, w, alpha=2.0, line_search=False, maxiter=1)
    assert torch.isfinite(z).all()


def test_edges_and_staging():
    from lasso_amd.linear.solvers import iterative_ridge
    x, w, z0 = case_inputs(CASES["small"])
    z = iterative_ridge(z0[:0].cuda(), x[:0].cuda(), w.cuda())
    assert z.shape == (0, 24) and z.is_cuda
    z, info, _, _ = run(z0, x, w, alpha=2.0, maxiter=0)
    assert torch.equal(z, z0) and info["iterations"] == 0 and info["status"] == "maxiter"
    zc = iterative_ridge(z0, x, w, alpha=2.0, line_search=False, maxiter=2)       # CPU tensors are staged
    assert zc.device.type == "cpu"
    zg = iterative_ridge(z0.cuda(), x.cuda(), w.cuda().requires_grad_(), alpha=2.0, line_search=False, maxiter=2)
    assert not zg.requires_grad and torch.equal(zg.cpu(), zc)
    zi = iterative_ridge(z0.cuda(), x.cuda(), w.cuda(), alpha=2.0, line_search=False, maxiter=2, cg_options=dict(rtol=1.0))
    assert torch.equal(zi.cpu(), zc)                          # cg_options without cg is ignored


# ---- the C ABI directly --------------------------------------------------------------------------------------------------
def test_pitched_and_offset_operands_through_the_c_abi():
    spec = CASES["odd"]
    x, w, z0 = case_inputs(spec)
    n, d, k = spec["n"], spec["d"], spec["k"]
    zp, ip, _, _ = run(z0, x, w, alpha=2.0, line_search=False, maxiter=3)
    status, z, res, bufs = abi_solve(z0, x, w, 2.0, 3, pitches=(d + 3, k + 1, k + 5, k + 7))
    assert status == 0 and res.n_iter == 3 and res.bad_row == -1
    assert float((z - zp).abs().max()) <= 5e-5
    for key, (buf, src, ld) in bufs.items():                  # inputs and every padding word are as they were
        rows = n if key != "w" else d
        cols = d if key == "x" else k
        host = buf.cpu()
        body = host[1:1 + rows * ld].view(rows, ld)
        if src is not None:
            assert torch.equal(body[:, :cols], src), key
            assert (body[:, cols:] == 777.0).all() and host[0] == 777.0 and (host[1 + rows * ld:] == 777.0).all(), key
        else:
            assert (body[:, cols:] == -555.0).all() and host[0] == -555.0 and (host[1 + rows * ld:] == -555.0).all(), key


def test_nonzero_reserved_is_refused():
    from lasso_amd import _native as nat
    x, w, z0 = case_inputs(CASES["small"])
    status, z, res, _ = abi_solve(z0, x, w, 2.0, 1, reserved=1)
    assert status == nat.LASSO_ERR_BAD_ARG
    assert (z == -555.0).all()


# ---- fresh shapes against the model --------------------------------------------------------------------------------------
FRESH = [(50, 70, 65, 2.0, 5), (19, 300, 290, 4.0, 3), (130, 96, 200, 3.0, 4)]


@pytest.mark.parametrize("n,d,k,alpha,maxiter", FRESH)
def test_fresh_shape_against_the_model(n, d, k, alpha, maxiter):
    x, w = recipe_xw(n, d, k, seed=22)
    z0 = ridge_start(x, w, alpha)
    kw = dict(alpha=alpha, line_search=False, maxiter=maxiter)
    z32, i32 = iter_ridge_model.iterative_ridge(z0, x, w, **kw)
    z64, i64 = iter_ridge_model.iterative_ridge(z0, x, w, dtype=torch.float64, **kw)
    assert min(i32["margin"], i64["margin"]) >= 0.01, "a model stop decision that rounding could flip: choose another seed"
    assert i32["iterations"] == i64["iterations"] == maxiter
    gap = float((z32.double() - z64).abs().max())
    bar = 4.0 * gap
    z, info, _, _ = run(z0, x, w, **kw)
    dz = float((z - z32).abs().max())
    print("fresh %s: max|dz| = %.3g (bar %.3g), supports %s" % ((n, d, k), dz, bar, info["support_max"]))
    record_margins("iter_ridge/fresh_%dx%dx%d" % (n, d, k), dict(dz=dz, bar=bar, gap=gap))
    assert info["iterations"] == maxiter and info["support_max"] == i32["support_max"]
    assert dz <= bar
    f64 = i64["fval"][-1]
    assert abs(info["fval"][-1] - f64) / f64 <= max(1e-6, 4.0 * abs(i32["fval"][-1] - f64) / f64)


# ---- 128 x 128 GEMM blocks, forced (LASSO_FORCE_BLOCKS_128) ---------------------------------------------------------------
# block_side() takes 128-blocks only from 2 x CUs blocks on, far above any shape here: the bit runs every product of the
# solve (StoreEpi for rhs = x W, Resid0Epi for the residual and its block partials) on Tile<128, 128>.  Shapes: more than
# one 128-block in a dimension and a nearly empty last one; contraction lengths for the three operand forms (a multiple
# of 32: LDS-DMA, of 4: 16-byte loads, odd: scalar loads) of both products.
F128 = [(130, 64, 288, 2.0, 4), (259, 36, 132, 2.0, 4), (131, 37, 131, 2.0, 4), (40, 200, 136, 3.0, 3), (1, 40, 24, 2.0, 4)]
_F128_MODEL = {}


def f128_model(n, d, k, alpha, maxiter):
    """the fresh-shape construction above, computed once per shape: (x, w, z0, z32, model info, bar, gap, f64, f bar)"""
    key = (n, d, k)
    if key not in _F128_MODEL:
        x, w = recipe_xw(n, d, k, seed=22)
        z0 = ridge_start(x, w, alpha)
        kw = dict(alpha=alpha, line_search=False, maxiter=maxiter)
        z32, i32 = iter_ridge_model.iterative_ridge(z0, x, w, **kw)
        z64, i64 = iter_ridge_model.iterative_ridge(z0, x, w, dtype=torch.float64, **kw)
        assert min(i32["margin"], i64["margin"]) >= 0.01, "a model stop decision that rounding could flip: choose another seed"
        assert i32["iterations"] == i64["iterations"] == maxiter
        gap = float((z32.double() - z64).abs().max())
        f64 = i64["fval"][-1]
        _F128_MODEL[key] = (x, w, z0, z32, i32, 4.0 * gap, gap, f64, max(1e-6, 4.0 * abs(i32["fval"][-1] - f64) / f64))
    return _F128_MODEL[key]


@pytest.mark.parametrize("reserved", [8, 0], ids=["f128", "s64"])
@pytest.mark.parametrize("n,d,k,alpha,maxiter", F128)
def test_forced_128_blocks_against_the_model(n, d, k, alpha, maxiter, reserved):
    from lasso_amd import _native as nat
    assert nat.FORCE_BLOCKS_128 == 8
    x, w, z0, z32, i32, bar, gap, f64, f_bar = f128_model(n, d, k, alpha, maxiter)
    status, z, res, _ = abi_solve(z0, x, w, alpha, maxiter, reserved=reserved)
    assert status == 0 and res.bad_row == -1
    dz = float((z - z32).abs().max())
    tag = "%dx%dx%d_%s" % (n, d, k, "f128" if reserved else "s64")
    print("fresh %s: max|dz| = %.3g (bar %.3g), supports %s" % (tag, dz, bar, res.support_max))
    record_margins("iter_ridge/fresh_" + tag, dict(dz=dz, bar=bar, gap=gap))
    assert res.n_iter == maxiter and res.support_max == i32["support_max"]
    assert dz <= bar
    assert abs(res.fval[-1] - f64) / f64 <= f_bar


def test_forced_128_blocks_pitched_repeatable_and_refused():
    from lasso_amd import _native as nat
    n, d, k, alpha, maxiter = F128[1]
    x, w, z0, z32, i32, bar = f128_model(n, d, k, alpha, maxiter)[:6]
    force = nat.FORCE_BLOCKS_128
    _, a, ra, _ = abi_solve(z0, x, w, alpha, maxiter, reserved=force)
    _, b, rb, _ = abi_solve(z0, x, w, alpha, maxiter, reserved=force)
    assert torch.equal(a, b) and ra.fval == rb.fval            # two forced solves are bitwise equal
    status, zp, rp, bufs = abi_solve(z0, x, w, alpha, maxiter, reserved=force, pitches=(d + 3, k + 1, k + 5, k + 7))
    assert status == 0 and rp.n_iter == maxiter and rp.support_max == i32["support_max"]
    dz = float((zp - z32).abs().max())
    print("pitched f128: max|dz| = %.3g (bar %.3g), against the packed forced solve %.3g" % (dz, bar, float((zp - a).abs().max())))
    record_margins("iter_ridge/pitched_%dx%dx%d_f128" % (n, d, k), dict(dz=dz, bar=bar))
    assert dz <= bar                                          # (odd pitches take the scalar loads: another summation order)
    for key, (buf, src, ld) in bufs.items():                  # inputs and every padding word are as they were
        rows, cols = (n if key != "w" else d), (d if key == "x" else k)
        host = buf.cpu()
        body = host[1:1 + rows * ld].view(rows, ld)
        fill = 777.0 if src is not None else -555.0
        assert src is None or torch.equal(body[:, :cols], src), key
        assert (body[:, cols:] == fill).all() and host[0] == fill and (host[1 + rows * ld:] == fill).all(), key
    for bad in (force | 1, force | 4, force | (1 << 40)):
        status, z, _, _ = abi_solve(z0, x, w, alpha, maxiter, reserved=bad)
        assert status == nat.LASSO_ERR_BAD_ARG and (z == -555.0).all(), bad
