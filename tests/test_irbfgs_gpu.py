"""iterative_ridge_bfgs on the GPU against the reference's recorded runs (tests/golden/irbfgs_cases.npz) and the host
model (tests/irbfgs_model.py).

Bars.  Codes: max|z - z_ref32| <= max(5e-5, 4 x spread_z), where spread_z is how far "another correct float32
implementation" (the model with permuted summation orders, dots in double, the symmetric update and the quadratic line
objective) moved the codes when the fixture was made; the factor 4 and the 5e-5 floor are the project's rule
(tests/test_own_gpu.py).  A case is compared by its codes only if spread_z <= 2.5e-3, so the bar never exceeds 1e-2.
Several Brent iterations are compared by objective only, max(1e-6, 4 x spread_f) against the float64 run
(tests/irbfgs_cases.py says why).

lasso_irbfgs_update is compared with the reference's BFGS.update formula and masked system in double
(irbfgs_model.update_reference), relative to the largest entry of the matrix: the bar is 4 x what the float32 model in
the reference's own operation order achieves on the same operands, never below 1e-6 (eight units of float32 rounding)."""
import contextlib
import ctypes as C
import io
import warnings

import numpy as np
import pytest
import torch

import irbfgs_model
from irbfgs_cases import CASES, admitted_f, admitted_z, case_inputs, load_case, recipe, rtol_of
from layouts import place
from margins import record_margins
from test_owlqn_gpu import same_line

pytestmark = pytest.mark.gpu
EPS = float(torch.finfo(torch.float32).eps)


@pytest.fixture(scope="module")
def cases(golden):
    return golden("irbfgs_cases")


def run(w, x, z0, **kw):
    """-> (z on the CPU, info, warnings, printed text); inputs go to the GPU and must come back bitwise unchanged"""
    from lasso_amd.nonlinear import iterative_ridge_bfgs, rss
    wg, xg, zg = w.cuda(), x.cuda(), z0.cuda()
    out = io.StringIO()
    with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(out):
        warnings.simplefilter("always")
        z, info = iterative_ridge_bfgs(rss(xg, wg), zg, return_info=True, **kw)
    assert z.is_cuda and z.dtype == x.dtype and z.data_ptr() != zg.data_ptr()
    assert torch.equal(wg.cpu(), w) and torch.equal(xg.cpu(), x) and torch.equal(zg.cpu(), z0)
    return z.cpu(), info, [str(c.message) for c in caught], out.getvalue()


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case(cases, name):
    spec, g = CASES[name], load_case(cases, name)
    x, w, z0 = case_inputs(spec)
    kw = spec["kwargs"]
    brent = bool(kw["line_search"])
    z, info, caught, text = run(w, x, z0, alpha=spec["alpha"], verbose=2, **kw)
    assert torch.isfinite(z).all()
    assert caught == [] and str(g["warnings"]) == ""
    assert info["iterations"] == len(g["f32"])
    assert info["lu"] == [False] * info["iterations"]
    if kw["maxiter"] == 0:
        assert torch.equal(z, z0) and text == ""
        return
    # the updates judged their rows as the reference's did (no update follows the iteration that stops, or the last)
    want_invalid = [int(v) for v in g["invalid_rows"]]
    if info["iterations"] == kw["maxiter"]:
        want_invalid[-1] = -1
    assert info["invalid_rows"] == want_invalid
    # frozen zeros stay bitwise zero; the all-zero row stays zero
    assert (z[z0 == 0].view(torch.int32) == 0).all()
    f_z = irbfgs_model.objective64(w, x, z, spec["alpha"])
    f_last = info["objective"][-1]
    print("%s: reported objective %.9g, objective of z %.9g" % (name, f_last, f_z))
    assert abs(f_last - f_z) <= 1e-6 * f_z
    if spec["compare"] == "z":
        assert admitted_z(g)
        bar = max(5e-5, 4.0 * float(g["spread_z"]))
        assert bar <= 1e-2
        dz = float((z - torch.from_numpy(g["z32"])).abs().max())
        print("%s: max|dz| = %.3g (bar %.3g)" % (name, dz, bar))
        rel = {}
        for key, got, want in (("t", info["t"], g["t32"]), ("objective", info["objective"], g["f32"]),
                               ("delta", info["delta_x"], g["dx32"])):
            if len(want) and (np.abs(want) > 0).all():
                rel[key] = float(np.max(np.abs(np.array(got) - want) / np.abs(want)))
                print("%s: %s rel %.3g (rtol %.3g)" % (name, key, rel[key], rtol_of(g, key)))
            else:
                assert list(got) == list(want)                        # (a step of length 0)
        assert dz <= bar, (name, dz, bar)
        for key in rel:
            assert rel[key] <= rtol_of(g, key), (name, key, rel[key], rtol_of(g, key))
        got_lines, want_lines = text.strip().split("\n"), str(g["stdout"]).strip().split("\n")
        assert len(got_lines) == len(want_lines)
        for a, b in zip(got_lines, want_lines):
            assert same_line(a, b, max(rtol_of(g, key) for key in ("objective", "delta"))), (a, b)
        margins = dict(dz=dz, bar=bar, **rel)
    else:
        assert admitted_f(g)
        f_ref = float(g["f64"][-1])
        err = abs(info["objective"][-1] - f_ref) / f_ref
        bar = max(1e-6, 4.0 * float(g["spread_f"]))
        print("%s: objective rel %.3g (bar %.3g)" % (name, err, bar))
        objs = [float(text.split("\n")[0].split(":")[1])] + info["objective"]
        assert all(b <= a * (1 + 1e-6) for a, b in zip(objs, objs[1:])), objs      # (Brent never ascends)
        assert err <= bar, (name, err, bar)
        margins = dict(objective_rel=err, bar=bar)
    record_margins("irbfgs/" + name, margins)


@pytest.mark.parametrize("name", ["brent1_wave", "brent1_lds70", "brent1_general"])
def test_brent_evaluations_are_the_line_objective(cases, name):
    """every (t, f) the search evaluated is the line objective of the first iteration, taken from the float64 model"""
    spec = CASES[name]
    x, w, z0 = case_inputs(spec)
    z, info, _, _ = run(w, x, z0, alpha=spec["alpha"], **spec["kwargs"])
    evals = info["evaluations"]
    assert len(evals) == info["ls_iters"][0] and 5 <= len(evals) <= 60 and all(e[0] == 1 for e in evals)
    assert all(0.0 < e[1] < 10.0 for e in evals)

    def first_line(dtype):
        m = irbfgs_model.Model(w, x, spec["alpha"], dtype)
        zz = z0.to(dtype)
        _, g, _ = m.evaluate(zz)
        A, rhs, _ = irbfgs_model.masked_system(torch.diag_embed(torch.ones_like(zz)), zz, g, spec["alpha"], 1e-4, EPS)
        d = torch.linalg.solve(A, rhs.unsqueeze(2)).squeeze(2)
        return lambda t: float(m.smooth(zz.add(d, alpha=-t))[0] + spec["alpha"] * zz.add(d, alpha=-t).norm(p=1))
    line64, line32 = first_line(torch.float64), first_line(torch.float32)
    ts = [float(np.float32(t)) for _, t, _ in evals]                          # (the step is applied as a float32)
    want = np.array([line64(t) for t in ts])
    gap = float(np.max(np.abs(np.array([line32(t) for t in ts]) - want) / want))
    rtol = max(1e-6, 4.0 * gap)
    err = float(np.max(np.abs(np.array([f for _, _, f in evals]) - want) / want))
    print("%s: %d evaluations, rel %.3g (rtol %.3g, model gap %.3g)" % (name, len(evals), err, rtol, gap))
    assert err <= rtol
    best = min(reversed(evals), key=lambda e: e[2])          # (a tie goes to the later evaluation)
    assert info["t"][0] == best[1]
    record_margins("irbfgs/evaluations_" + name, dict(rel=err, rtol=rtol, count=len(evals)))


# ---- lasso_irbfgs_update --------------------------------------------------------------------------------------------
GUARD = 64
SENTINEL = -7.25


def guarded(t):
    """a device copy of t inside a buffer with GUARD sentinel words on either side -> (view, buffer)"""
    buf = torch.full((t.numel() + 2 * GUARD,), SENTINEL, dtype=t.dtype, device="cuda")
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def guards_hold(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def update_operands(n, k, seed):
    """B symmetric positive definite, a step with exact zeros kept, y = H s + noise (y.s > 0); the LAST row of a batch of
    three or more has s = 0 and y != 0: y.s = 0, an invalid row"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, k, k, generator=g)
    B = torch.diag_embed(torch.ones(n, k)) + 0.1 * (a @ a.transpose(1, 2)) / k
    B = 0.5 * (B + B.transpose(1, 2))
    h = torch.randn(n, k, k, generator=g)
    H = torch.diag_embed(torch.ones(n, k)) + 0.2 * (h @ h.transpose(1, 2)) / k
    zero = torch.rand(n, k, generator=g) < 0.3
    x_prev = (0.3 * torch.randn(n, k, generator=g)).masked_fill(zero, 0)
    s = (0.1 * torch.randn(n, k, generator=g)).masked_fill(zero, 0)
    g_prev = torch.randn(n, k, generator=g)
    y = torch.bmm(H, s.unsqueeze(2)).squeeze(2) + 0.01 * torch.randn(n, k, generator=g)
    if n >= 3:
        s[n - 1] = 0
    if k == 1:
        x_prev[:, 0] = 0.3
        s[:, 0] = 0.1
        y = 1.5 * s
        if n >= 3:
            s[n - 1] = 0
            y[n - 1] = 0.2
    return B, x_prev + s, g_prev + y, x_prev, g_prev


def abi_update(B, x, g, x_prev, g_prev, alpha, tikhonov, mode, first, max_wgs=0):
    from lasso_amd import _native as nat
    n, k = x.shape
    (Bv, Bb), (sv, sb) = guarded(B), guarded(torch.zeros(n, k, k))
    xv, gv, xpv, gpv = x.cuda(), g.cuda(), x_prev.cuda(), g_prev.cuda()
    (rv, rb) = guarded(torch.zeros(n, k))
    valid = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    nat.check(nat.lib().lasso_irbfgs_update(nat.ptr(Bv), nat.ptr(xv), nat.ptr(gv), nat.ptr(xpv), nat.ptr(gpv), nat.ptr(sv),
                                            nat.ptr(rv), nat.ptr(valid), n, k, nat.LASSO_F32, alpha, tikhonov, EPS, mode,
                                            first, max_wgs, nat.stream_ptr(torch.device("cuda", 0))))
    torch.cuda.synchronize()
    assert guards_hold(Bb) and guards_hold(sb) and guards_hold(rb)
    assert torch.equal(xv.cpu(), x) and torch.equal(gv.cpu(), g)
    assert torch.equal(xpv.cpu(), x) and torch.equal(gpv.cpu(), g)           # the pair became the new iterate
    return Bv.cpu(), sv.cpu(), rv.cpu(), valid.cpu()


# every k in front of, at and behind a 32-block and a vector of four, above 256 -- and (one row) the cap
@pytest.mark.parametrize("n,k", [(n, k) for k in (1, 31, 32, 33, 70, 257) for n in (1, 3, 5)] + [(1, 1024)])
def test_update_against_the_reference_formula(n, k):
    alpha, tik = 0.1, 1e-4
    B, x, g, x_prev, g_prev = update_operands(n, k, seed=100 * k + n)
    for first in (1, 0):
        want_B, want_A, want_rhs, want_valid = irbfgs_model.update_reference(B, x, g, x_prev, g_prev, alpha, tik, EPS, first)
        hess = irbfgs_model.Hessians(x_prev, g_prev, symmetric=False)
        hess.B, hess.n_updates = B.clone(), 0 if first else 1
        hess.update(x, g)
        for wgs in ((0, 2) if n == 5 else (0,)):                                # a grid smaller than n: rows are strided
            got_B, got_A, got_rhs, got_valid = abi_update(B, x, g, x_prev, g_prev, alpha, tik, 1, first, wgs)
            assert got_valid.bool().tolist() == want_valid.tolist()
            assert n < 3 or not got_valid[n - 1]
            scale = float(want_B.abs().max())
            err = float((got_B.double() - want_B).abs().max()) / scale
            gap = float((hess.B.double() - want_B).abs().max()) / scale
            bar = max(1e-6, 4.0 * gap)
            print("update n=%d k=%d first=%d wgs=%d: rel %.3g (bar %.3g, float32 model %.3g)" % (n, k, first, wgs, err, bar, gap))
            assert err <= bar
            # B is bitwise symmetric, the emitted lower triangle is B masked and loaded -- bit for bit, from the B that
            # was written -- and the right-hand side is the reference's float32 expression
            assert torch.equal(got_B, got_B.transpose(1, 2))
            A32, rhs32, _ = irbfgs_model.masked_system(got_B, x, g, alpha, tik, EPS)
            assert torch.equal(got_A.tril(), A32.tril())
            assert torch.equal(got_rhs, rhs32)
            assert float((got_A.tril().double() - want_A.tril()).abs().max()) / float(want_A.abs().max()) <= bar
            # an invalid row keeps its bits apart from the first update's scaling
            if n >= 3:
                r = n - 1
                if first:
                    y = (g[r] - g_prev[r])
                    factor = torch.tensor(1000., dtype=torch.float32) * (y.double() * y.double()).sum().float()
                    assert torch.equal(got_B[r], B[r] * factor)
                else:
                    assert torch.equal(got_B[r], B[r])
        record_margins("irbfgs/update_n%d_k%d_first%d" % (n, k, first), dict(rel=err, bar=bar, gap=gap))


@pytest.mark.parametrize("k", [1, 33, 72])
def test_update_modes_without_an_update(k):
    """mode 0 writes B = I and its system; mode 2 leaves B as it is"""
    n, alpha, tik = 3, 0.1, 1e-4
    B, x, g, x_prev, g_prev = update_operands(n, k, seed=7 + k)
    eye = torch.diag_embed(torch.ones(n, k))
    for mode, want_B in ((0, eye), (2, B)):
        got_B, got_A, got_rhs, got_valid = abi_update(B, x, g, x_prev, g_prev, alpha, tik, mode, 0)
        assert torch.equal(got_B, want_B) and got_valid.tolist() == [1] * n
        A32, rhs32, _ = irbfgs_model.masked_system(want_B, x, g, alpha, tik, EPS)
        assert torch.equal(got_A.tril(), A32.tril()) and torch.equal(got_rhs, rhs32)


# ---- the solve's contract -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("line_search", [True, False])
def test_two_identical_calls_are_bitwise_equal(line_search):
    spec = CASES["fixed4_lds70"]
    x, w, z0 = case_inputs(spec)
    kw = dict(alpha=0.1, line_search=line_search, lr=0.3, maxiter=5)
    a = run(w, x, z0, **kw)
    b = run(w, x, z0, **kw)
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    assert a[1]["iterations"] == 5
    assert set(a[1]) == {"iterations", "t", "ls_iters", "objective", "delta_x", "invalid_rows", "lu", "evaluations"}


def abi_solve(w, x, z0, alpha, line_search, maxiter, lr, xtol, plan, reserved=0, refused=None):
    """lasso_irbfgs_solve directly, every operand placed by tests/layouts.py -> (z on the CPU, result struct); the
    result carries the per-iteration trace as res.objective and res.invalid_rows.  refused: the status a refusal must
    have; nothing may have been written then"""
    from lasso_amd import _native as nat
    n, d = x.shape
    k = w.shape[1]
    ops = dict(x=place(x, plan["x"], float("nan"), "cuda", "x"), w=place(w, plan["w"], float("nan"), "cuda", "w"),
               z0=place(z0, plan["z0"], float("nan"), "cuda", "z0"))
    out = place(torch.zeros(n, k), plan["z"], -7.25, "cuda", "z", fill=-7.25)
    opts = nat.IrbfgsOptions(maxiter, 1 if line_search else 0, lr, xtol, 1e-4, EPS, reserved)
    res = nat.IrbfgsResult()
    cap = max(maxiter, 1)
    t_arr, f_arr, dx_arr = ((C.c_double * cap)() for _ in range(3))
    ls_arr, inv_arr, lu_arr = ((C.c_int32 * cap)() for _ in range(3))
    trace = nat.IrbfgsTrace(cap, 0, t_arr, ls_arr, f_arr, dx_arr, inv_arr, lu_arr, None, None, None, 0)
    res.trace = C.pointer(trace)
    L = nat.lib()
    ws = torch.empty(L.lasso_irbfgs_workspace_bytes(n, d, k, nat.LASSO_F32), dtype=torch.uint8, device="cuda")
    status = L.lasso_irbfgs_solve(nat.ptr(ops["x"].view), ops["x"].ld, nat.ptr(ops["w"].view), ops["w"].ld,
                                  nat.ptr(ops["z0"].view), ops["z0"].ld, nat.ptr(out.view), out.ld, n, d, k, nat.LASSO_F32,
                                  alpha, C.byref(opts), C.byref(res), nat.ptr(ws), ws.numel(),
                                  nat.stream_ptr(torch.device("cuda", 0)))
    torch.cuda.synchronize()
    for p in ops.values():
        p.check()
    if refused is not None:
        assert status == refused, (status, refused)
        out.check(written=False)
        return out.view.cpu(), res
    nat.check(status)
    out.check(written=True)
    its = min(res.n_iter, cap)
    res.objective, res.invalid_rows, res.lu = list(f_arr[:its]), list(inv_arr[:its]), list(lu_arr[:its])
    return out.view.cpu(), res


@pytest.mark.parametrize("layout", ["pitched", "odd", "offset"])
def test_pitched_and_offset_operands_through_the_c_abi(layout):
    spec = CASES["fixed4_lds33"]
    x, w, z0 = case_inputs(spec)
    names = ("x", "w", "z0", "z")
    want, res0 = abi_solve(w, x, z0, 0.1, False, 4, 0.3, 1e-5, {nm: "natural" for nm in names})
    got, res = abi_solve(w, x, z0, 0.1, False, 4, 0.3, 1e-5, {nm: layout for nm in names})
    assert res.n_iter == res0.n_iter == 4
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    z_py, _, _, _ = run(w, x, z0, alpha=0.1, line_search=False, lr=0.3, maxiter=4)
    assert torch.equal(want, z_py)


def test_a_row_does_not_depend_on_its_batch():
    """fixed steps, xtol = 0 and a start whose batch-wide |grad|_1 is below 1 (so the first step is lr whatever the batch):
    a row's code is bitwise the same alone, in a batch of five, and in another position of the batch"""
    n, d, k = 5, 16, 33
    x, w, z0 = case_inputs(dict(n=n, d=d, k=k, seed=3, start="sparse"))
    g1 = float(((z0 @ w.T - x) @ w).abs().sum())
    c = 0.5 / g1
    x, z0 = x * c, z0 * c
    assert float(((z0 @ w.T - x) @ w).abs().sum()) <= 1.0
    assert float(z0[z0 != 0].abs().min()) > 100 * EPS
    kw = dict(alpha=0.1 * c, line_search=False, lr=0.3, xtol=0.0, maxiter=4)
    full, info, _, _ = run(w, x, z0, **kw)
    assert info["iterations"] == 4 and info["t"] == [pytest.approx(0.3, rel=1e-6)] * 4
    perm = torch.tensor([3, 4, 0, 1, 2])
    moved, _, _, _ = run(w, x[perm], z0[perm], **kw)
    assert torch.equal(moved.view(torch.int32), full[perm].view(torch.int32))
    for r in (0, 2, 4):
        alone, _, _, _ = run(w, x[r:r + 1], z0[r:r + 1], **kw)
        assert torch.equal(alone.view(torch.int32), full[r:r + 1].view(torch.int32)), r


def test_edges_no_rows_cpu_tensors_and_grad_inputs():
    from lasso_amd.nonlinear import iterative_ridge_bfgs, rss
    x, w = recipe(7, 12, 24, seed=1)
    z0 = torch.randn(7, 24, generator=torch.Generator().manual_seed(5))
    z = iterative_ridge_bfgs(rss(x[:0].cuda(), w.cuda()), z0[:0].cuda())
    assert z.shape == (0, 24) and z.is_cuda
    z, info, _, text = run(w, x, z0, alpha=0.3, maxiter=0, verbose=2)
    assert torch.equal(z, z0) and info["iterations"] == 0 and text == ""
    zc = iterative_ridge_bfgs(rss(x, w), z0, alpha=0.3, line_search=False, maxiter=2, lr=0.3)
    assert zc.device.type == "cpu" and torch.isfinite(zc).all()
    zg = iterative_ridge_bfgs(rss(x.cuda(), w.cuda().requires_grad_()), z0.cuda().requires_grad_(), alpha=0.3, maxiter=1)
    assert not zg.requires_grad
    # the default maxiter is 5 k and the default xtol stops it
    zd, info = iterative_ridge_bfgs(rss(x.cuda(), w.cuda()), z0.cuda(), alpha=0.3, return_info=True)
    assert 1 <= info["iterations"] <= 5 * 24


# ---- 128 x 128 GEMM blocks, forced (LASSO_FORCE_BLOCKS_128) ---------------------------------------------------------------
# block_side() takes 128-blocks only from 2 x CUs blocks on, far above any shape here: the bit runs both products of the
# solve (the residual with its block partials, Resid0Epi, and the gradient r W on W^T, StoreEpi) on Tile<128, 128>.
# Shapes: more than one 128-block in a dimension and a nearly empty last one; contraction lengths for the three operand
# forms (a multiple of 32: LDS-DMA, of 4: 16-byte loads, odd: scalar loads) of both products.  The golden cases'
# dictionary, start and fixed-step arguments (fixed4_*); n = 1 takes the dense start (the sparse one zeroes the last row).
# The data is x = z0 W^T + 1e-6 noise, so the batch-wide |grad|_1 of the start is below 1 and the first step is lr: with
# the recipe's x a batch this large starts with t = lr / |grad|_1 ~ 1e-5, the first pair (s, y) is a difference of nearly
# equal float32 numbers, and the model's own summation orders end 1e-2 apart in the codes -- nothing to compare with.
F128 = [(130, 64, 288), (259, 36, 132), (131, 37, 131), (40, 200, 136), (1, 40, 24)]
F128_KW = dict(alpha=0.1, line_search=False, lr=0.3, maxiter=3)
NATURAL = {nm: "natural" for nm in ("x", "w", "z0", "z")}
_F128_MODEL = {}


def f128_model(n, d, k):
    """the model in float32, and how far other correct implementations move its codes and objective (the golden
    generator's measure, here with one other summation order and float64: the spread stays a hundredth of the floor) -> (x, w, z0, z32, i32, bar, spread_z, objective rtol)"""
    key = (n, d, k)
    if key not in _F128_MODEL:
        _, w, z0 = case_inputs(dict(n=n, d=d, k=k, seed=0, start="sparse" if n > 1 else "dense"))
        x = z0 @ w.T + 1e-6 * torch.randn(n, d, generator=torch.Generator().manual_seed(77))
        assert float(((z0 @ w.T - x) @ w).abs().sum()) <= 1.0
        z32, i32 = irbfgs_model.iterative_ridge_bfgs(w, x, z0, **F128_KW)
        irbfgs_model.assert_robust(i32)
        others = [irbfgs_model.iterative_ridge_bfgs(w, x, z0, order_seed=sd, **F128_KW) for sd in (1,)]
        others.append(irbfgs_model.iterative_ridge_bfgs(w, x, z0, dtype=torch.float64, **F128_KW))
        for _, info in others:
            assert info["iterations"] == i32["iterations"] == F128_KW["maxiter"] and min(i32["delta_x"]) > 0.05
            assert info["invalid_rows"] == i32["invalid_rows"]
        spread_z = max(float((z.double() - z32.double()).abs().max()) for z, _ in others)
        spread_f = max(abs(info["objective"][-1] - i32["objective"][-1]) / abs(i32["objective"][-1]) for _, info in others)
        assert spread_z <= 2.5e-3, "a case whose codes rounding alone moves: not comparable by its codes"
        _F128_MODEL[key] = (x, w, z0, z32, i32, max(5e-5, 4.0 * spread_z), spread_z, max(1e-6, 4.0 * spread_f))
    return _F128_MODEL[key]


def check_f128(tag, z, res, model):
    x, w, z0, z32, i32, bar, spread_z, f_rtol = model
    dz = float((z - z32).abs().max())
    f_rel = abs(res.objective[-1] - i32["objective"][-1]) / abs(i32["objective"][-1])
    print("%s: max|dz| = %.3g (bar %.3g), objective rel %.3g (rtol %.3g)" % (tag, dz, bar, f_rel, f_rtol))
    record_margins("irbfgs/fresh_" + tag, dict(dz=dz, bar=bar, spread_z=spread_z, objective_rel=f_rel, objective_rtol=f_rtol))
    assert res.n_iter == i32["iterations"] and res.lu == [0] * res.n_iter
    assert res.invalid_rows == i32["invalid_rows"][:-1] + [-1]     # (no update follows the last iteration)
    assert (z[z0 == 0].view(torch.int32) == 0).all()               # frozen zeros stay bitwise zero
    assert dz <= bar, (tag, dz, bar)
    assert f_rel <= f_rtol, (tag, f_rel, f_rtol)


@pytest.mark.parametrize("reserved", [8, 0], ids=["f128", "s64"])
@pytest.mark.parametrize("n,d,k", F128)
def test_forced_128_blocks_against_the_model(n, d, k, reserved):
    from lasso_amd import _native as nat
    assert nat.FORCE_BLOCKS_128 == 8
    model = f128_model(n, d, k)
    x, w, z0 = model[:3]
    z, res = abi_solve(w, x, z0, 0.1, False, F128_KW["maxiter"], 0.3, 1e-5, NATURAL, reserved=reserved)
    check_f128("%dx%dx%d_%s" % (n, d, k, "f128" if reserved else "s64"), z, res, model)


def test_forced_128_blocks_pitched_repeatable_and_refused():
    from lasso_amd import _native as nat
    model = f128_model(*F128[1])
    x, w, z0 = model[:3]
    force = nat.FORCE_BLOCKS_128
    a, ra = abi_solve(w, x, z0, 0.1, False, F128_KW["maxiter"], 0.3, 1e-5, NATURAL, reserved=force)
    b, rb = abi_solve(w, x, z0, 0.1, False, F128_KW["maxiter"], 0.3, 1e-5, NATURAL, reserved=force)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and ra.objective == rb.objective
    for layout in ("pitched", "odd", "offset"):               # as at 64: the layout does not change a bit
        got, res = abi_solve(w, x, z0, 0.1, False, F128_KW["maxiter"], 0.3, 1e-5, {nm: layout for nm in NATURAL}, reserved=force)
        assert res.n_iter == F128_KW["maxiter"]
        assert torch.equal(got.view(torch.int32), a.view(torch.int32)), layout
    # the timing bit keeps its meaning next to the force bit
    t, rt = abi_solve(w, x, z0, 0.1, False, F128_KW["maxiter"], 0.3, 1e-5, NATURAL, reserved=force | nat.IRBFGS_TIME_ROWS)
    assert torch.equal(t.view(torch.int32), a.view(torch.int32)) and rt.row_ms > 0.0 and ra.row_ms == 0.0
    for bad in (force | 1, force | 4, force | (1 << 40)):
        z, _ = abi_solve(w, x, z0, 0.1, False, F128_KW["maxiter"], 0.3, 1e-5, NATURAL, reserved=bad, refused=nat.LASSO_ERR_BAD_ARG)
        assert (z == -7.25).all(), bad
