"""interior_point on the GPU against the reference's recorded runs (tests/golden/interior_point_cases.npz), the host
model (tests/interior_point_model.py) and, for the row kernel alone, a float64 solve of each row's system.

Bars.  Codes: max|z - z_ref32| <= max(5e-5, 4 x spread_z), where spread_z is how far "another correct float32
implementation" (the model with permuted summation orders and unknowns) moved the codes when the fixture was made; the
factor 4 and the 5e-5 floor are the project's rule (tests/test_gpsr_gpu.py).  A case is compared by its codes only if
spread_z <= 2.5e-3.  The maxiter=20 cases are compared by the lasso objective of their codes only
(tests/interior_point_cases.py says why): max(1e-6, 4 x spread_f).  Per-iteration records: max(1e-5, 4 x their spread).
The row kernel: 4 x e_ref, where e_ref is the relative infinity-norm error of torch's own float32 Cholesky on the same
systems, measured by the test on the CPU against the same double solve.  Fresh shapes: 4 x the model's float32 / float64
gap."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import interior_point_model
from interior_point_cases import (CASES, RECORDS, admitted_f, admitted_z, case_inputs, lasso_objective, load_case,
                                  ridge_start, rtol_of)
from layouts import SENTINEL, place
from margins import record_margins
from recipes import recipe_xw

pytestmark = pytest.mark.gpu
INFO_KEYS = dict(obj="obj", prim="prim_feas", dual="dual_feas", gap="gap")


@pytest.fixture(scope="module")
def cases(golden):
    return golden("interior_point_cases")


def run(x, w, z0, **kw):
    """-> (z on the CPU, success, info, printed text); inputs go to the GPU and must come back bitwise unchanged"""
    from lasso_amd.linear.solvers import interior_point
    wg, xg = w.cuda(), x.cuda()
    zg = None if z0 is None else z0.cuda()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        z, ok, info = interior_point(xg, wg, z0=zg, return_info=True, **kw)
    assert z.is_cuda and z.dtype == x.dtype and isinstance(ok, bool)
    same = lambda a, b: torch.equal(a.cpu().view(torch.int32), b.view(torch.int32))      # noqa: E731  (bits: x may hold a NaN)
    assert same(wg, w) and same(xg, x) and (z0 is None or same(zg, z0))
    return z.cpu(), ok, info, out.getvalue()


def record_rel(info, g):
    return {key: float(np.max(np.abs(np.array(info[INFO_KEYS[key]]) - g[key + "32"]) / np.abs(g[key + "32"]))) for key in RECORDS}


@pytest.fixture(scope="module")
def solved(cases):
    """every golden case solved once (verbose), shared by the tests below"""
    out = {}
    for name, spec in CASES.items():
        x, w, z0 = case_inputs(spec)
        out[name] = run(x, w, z0, alpha=spec["alpha"], verbose=True, **spec["kwargs"])
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case(cases, solved, name):
    spec, g = CASES[name], load_case(cases, name)
    x, w, z0 = case_inputs(spec)
    z, ok, info, _ = solved[name]
    assert torch.isfinite(z).all()
    rel = record_rel(info, g) if info["iterations"] == len(g["obj32"]) else {}
    for key in rel:
        print("%s: %s rel %.3g (rtol %.3g)" % (name, key, rel[key], rtol_of(g, key)))
    if spec["compare"] == "z":
        assert admitted_z(g)
        bar = max(5e-5, 4.0 * float(g["spread_z"]))
        assert bar <= 1e-2
        dz = float((z - torch.from_numpy(g["z32"])).abs().max())
        print("%s: max|dz| = %.3g (bar %.3g), %d iterations" % (name, dz, bar, info["iterations"]))
        margins = dict(dz=dz, bar=bar, **rel)
        record_margins("interior_point/" + name, margins)
        assert dz <= bar, (name, dz, bar)
    else:
        assert admitted_f(g)
        f_ref = float(g["lasso64"])
        err = abs(lasso_objective(z, x, w, spec["alpha"]) - f_ref) / f_ref
        bar = max(1e-6, 4.0 * float(g["spread_f"]))
        print("%s: lasso objective rel %.3g (bar %.3g)" % (name, err, bar))
        record_margins("interior_point/" + name, dict(objective_rel=err, bar=bar, **rel))
        assert err <= bar, (name, err, bar)
    assert info["iterations"] == len(g["obj32"])
    assert ok == bool(g["success"]) == bool(spec.get("stops"))
    for key in rel:
        assert rel[key] <= rtol_of(g, key), (name, key, rel[key], rtol_of(g, key))


@pytest.mark.parametrize("name", ["odd", "stop_d256", "long_d33"])
def test_verbose_output(cases, solved, name):
    g = load_case(cases, name)
    _, _, info, text = solved[name]
    got, want = text.rstrip("\n").split("\n"), str(g["stdout"]).rstrip("\n").split("\n")
    assert len(got) == len(want) == 4 + info["iterations"]
    assert got[0].startswith("initial obj func: ") and want[0].startswith("initial obj func: ")
    assert abs(float(got[0].split(":")[1]) - float(want[0].split(":")[1])) <= 2e-4 * float(want[0].split(":")[1])
    assert got[1:4] == want[1:4]                              # the blank line, the header, the separators
    for a, b in zip(got[4:], want[4:]):
        fa, fb = a.split("|"), b.split("|")
        assert len(a) == len(b) and [len(s) for s in fa] == [len(s) for s in fb], (a, b)
        assert int(fa[1]) == int(fb[1])
        for col, key, digits in ((2, "obj", 1e-4), (3, "prim", 1e-2), (4, "dual", 1e-2), (5, "gap", 1e-2)):
            va, vb = float(fa[col]), float(fb[col])         # (printed to 5 / 3 digits: that much on top of the bar)
            assert abs(va - vb) <= (rtol_of(g, key) + digits) * abs(vb), (key, a, b)


# ---- the row kernel alone ------------------------------------------------------------------------------------------------
def abi_rows(w, c, b, layout="natural"):
    """lasso_interior_point_rows with every operand in `layout` -> y on the CPU"""
    from lasso_amd import _native as nat
    n, d = b.shape
    k = w.shape[1]
    nan = float("nan")
    pw, pc, pb = (place(t, layout, nan, device="cuda", name=nm) for t, nm in ((w, "w"), (c, "c"), (b, "b")))
    py = place(torch.zeros(n, d), layout, SENTINEL, device="cuda", name="y", fill=SENTINEL)
    L = nat.lib()
    nat.check(L.lasso_interior_point_rows(C.c_void_p(pw.view.data_ptr()), pw.ld, C.c_void_p(pc.view.data_ptr()), pc.ld,
                                          C.c_void_p(pb.view.data_ptr()), pb.ld, C.c_void_p(py.view.data_ptr()), py.ld,
                                          n, d, k, nat.LASSO_F32, nat.stream_ptr(torch.device("cuda", 0))))
    torch.cuda.synchronize()
    for p in (pw, pc, pb):
        p.check()
    py.check(written=True)
    return py.view.cpu()


def row_systems(n, d, k, seed):
    """W [d,k], c [n,k] >= 0 spanning six decades with exact zeros, b [n,d]"""
    g = torch.Generator().manual_seed(seed)
    x, w = recipe_xw(n, d, k, seed=seed)
    c = torch.exp(torch.rand(n, k, generator=g) * np.log(1e6) + np.log(1e-3)).float()
    c = torch.where(torch.rand(n, k, generator=g) < 0.2, torch.zeros(()), c)
    assert (c == 0).any() and float(c.max()) / float(c[c > 0].min()) > 1e5
    return w, c, x


ROW_SHAPES = [(1, 7), (31, 13), (31, 50), (32, 14), (32, 70), (33, 18), (33, 65), (64, 37), (64, 131), (255, 101),
              (255, 301), (256, 150), (256, 303)]


@pytest.mark.parametrize("d,k", ROW_SHAPES)
def test_rows_against_float64(d, k):
    assert k % 4 != 0
    n = 6
    w, c, b = row_systems(n, d, k, seed=3)
    got = abi_rows(w, c, b)
    wd = w.double()
    m64 = torch.matmul(wd.unsqueeze(0) * c.double().unsqueeze(1), wd.T) + torch.eye(d, dtype=torch.float64)
    want = torch.linalg.solve(m64, b.double().unsqueeze(2)).squeeze(2)
    m32 = torch.matmul(w.unsqueeze(0) * c.unsqueeze(1), w.T)
    m32.diagonal(dim1=1, dim2=2).add_(1)
    chol, info = torch.linalg.cholesky_ex(m32)
    assert bool((info == 0).all())
    ref32 = torch.cholesky_solve(b.unsqueeze(2), chol).squeeze(2)
    scale = want.abs().amax(1)
    e_ref = float(((ref32.double() - want).abs().amax(1) / scale).max())
    err = float(((got.double() - want).abs().amax(1) / scale).max())
    bar = 4.0 * e_ref
    print("rows d=%d k=%d: err %.3g, e_ref %.3g, bar %.3g" % (d, k, err, e_ref, bar))
    record_margins("interior_point/rows_d%d_k%d" % (d, k), dict(err=err, e_ref=e_ref, bar=bar))
    assert err <= bar, (d, k, err, e_ref)


@pytest.mark.parametrize("layout", ["pitched", "odd", "offset"])
def test_rows_pitched_and_offset_operands(layout):
    w, c, b = row_systems(5, 45, 28, seed=4)                 # k a multiple of 4: the natural layout reads W as float4
    want = abi_rows(w, c, b)
    got = abi_rows(w, c, b, layout)
    assert torch.equal(got, want)                             # the same operands in the same order, however they are read


def test_rows_zero_weights_give_the_identity():
    """c = 0 everywhere: the system is the identity, y = b exactly"""
    w, c, b = row_systems(3, 70, 33, seed=5)
    assert torch.equal(abi_rows(w, torch.zeros_like(c), b), b)


# ---- fresh shapes against the model --------------------------------------------------------------------------------------
# n = 1, and more rows than the row kernel's grid (six workgroups per CU at d <= 64: 1536 on 256 CUs)
FRESH = [(1, 40, 24, 0.3, 3), (1700, 16, 40, 0.3, 3)]


@pytest.mark.parametrize("n,d,k,alpha,maxiter", FRESH)
def test_fresh_shape_against_the_model(n, d, k, alpha, maxiter):
    x, w = recipe_xw(n, d, k, seed=22)
    z0 = ridge_start(x, w, alpha)
    kw = dict(alpha=alpha, maxiter=maxiter, tol=0.0)
    z32, _, i32 = interior_point_model.interior_point(x, w, z0, **kw)
    z64, _, i64 = interior_point_model.interior_point(x, w, z0, dtype=torch.float64, **kw)
    gap = float((z32.double() - z64).abs().max())
    bar = 4.0 * gap
    z, ok, info, _ = run(x, w, z0, **kw)
    dz = float((z.double() - z64).abs().max())
    print("fresh %s: max|z - z64| = %.3g (bar %.3g)" % ((n, d, k), dz, bar))
    record_margins("interior_point/fresh_%dx%dx%d" % (n, d, k), dict(dz=dz, bar=bar, gap=gap))
    assert info["iterations"] == maxiter and ok is False
    assert dz <= bar
    for key in ("obj", "prim", "gap"):                       # (dual_feas is rounding noise from this start: ra = 0 in exact arithmetic)
        want, got = np.array(i64[INFO_KEYS[key]]), np.array(info[INFO_KEYS[key]])
        model = np.array(i32[INFO_KEYS[key]])
        # prim_feas is the norm of x - z W^T - lambda, a difference of O(|x|) terms: its rounding floor is absolute,
        # a few float32 ulp of max |x| per entry, whatever is left of the residual
        floor = 4.0 * float(torch.finfo(torch.float32).eps) * float(x.abs().max()) if key == "prim" else 0.0
        assert (np.abs(got - want) <= np.maximum(np.maximum(4.0 * np.abs(model - want), 1e-5 * np.abs(want)), floor)).all(), key


# ---- properties ----------------------------------------------------------------------------------------------------------
def test_two_solves_are_bitwise_equal(solved):
    spec = CASES["wide"]
    x, w, z0 = case_inputs(spec)
    a = run(x, w, z0, alpha=spec["alpha"], verbose=True, **spec["kwargs"])
    b = solved["wide"]
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and a[3] == b[3]


def test_start_that_is_not_interior_raises():
    from lasso_amd.linear.solvers import interior_point
    x, w, z0 = case_inputs(CASES["small"])
    with pytest.raises(AssertionError):
        interior_point(x.cuda(), w.cuda(), z0=torch.zeros_like(z0).cuda(), alpha=0.3)
    one = z0.clone()
    one[7] = 0.0
    with pytest.raises(AssertionError):
        interior_point(x.cuda(), w.cuda(), z0=one.cuda(), alpha=0.3)
    torch.cuda.synchronize()                                  # a clean status: the device is usable
    z, ok, info, _ = run(x, w, z0, alpha=0.3, maxiter=1, tol=0.0)
    assert torch.isfinite(z).all() and info["iterations"] == 1


def test_default_start_is_the_ridge_code():
    from lasso_amd.linear.sparse_encode import _ridge_init
    spec = CASES["odd"]
    x, w, _ = case_inputs(spec)
    z0 = _ridge_init(x.cuda(), w.cuda(), spec["alpha"]).cpu()
    a = run(x, w, None, alpha=spec["alpha"], **spec["kwargs"])
    b = run(x, w, z0, alpha=spec["alpha"], **spec["kwargs"])
    assert torch.equal(a[0], b[0]) and a[2] == b[2]


def test_edges_and_staging():
    from lasso_amd.linear.solvers import interior_point
    x, w, z0 = case_inputs(CASES["small"])
    z, ok = interior_point(x[:0].cuda(), w.cuda(), z0=z0[:0].cuda())
    assert z.shape == (0, 24) and z.is_cuda and ok is False
    z, ok, info, _ = run(x, w, z0, alpha=0.3, maxiter=0)
    assert torch.equal(z, (torch.relu(z0) + 0.1) - (torch.relu(-z0) + 0.1)) and ok is False and info["iterations"] == 0
    zg, okg, _, _ = run(x, w, z0, alpha=0.3, maxiter=2, tol=0.0)
    zc, okc = interior_point(x, w, z0=z0, alpha=0.3, maxiter=2, tol=0.0)      # CPU tensors are staged
    assert zc.device.type == "cpu" and torch.equal(zc, zg) and okc is okg is False
    with torch.no_grad():
        zn, _ = interior_point(x.cuda(), w.cuda().requires_grad_(), z0=z0.cuda(), alpha=0.3, maxiter=2, tol=0.0)
    assert not zn.requires_grad and torch.equal(zn.cpu(), zc)


def test_nan_in_one_row_of_x_stays_in_that_row(cases):
    spec = CASES["stop_odd"]
    x, w, z0 = case_inputs(spec)
    bad = x.clone()
    bad[5, 2] = float("nan")
    clean = run(x, w, z0, alpha=spec["alpha"], maxiter=4, tol=0.0)
    dirty = run(bad, w, z0, alpha=spec["alpha"], maxiter=4, tol=0.0)
    assert torch.isnan(dirty[0][5]).all()
    keep = [i for i in range(spec["n"]) if i != 5]
    assert torch.equal(dirty[0][keep], clean[0][keep])       # every other row is bitwise what it is without the NaN
    assert dirty[1] is False and dirty[2]["iterations"] == 4
    # with the default tol the clean solve stops at iteration 4; a NaN mean never stops the loop
    z, ok, info, _ = run(bad, w, z0, alpha=spec["alpha"])
    assert ok is False and info["iterations"] == 20 and len(info["gap"]) == 20
    assert all(v != v for v in info["prim_feas"])
    assert torch.isnan(z[5]).all() and torch.isfinite(z[keep]).all()


# ---- the C ABI directly --------------------------------------------------------------------------------------------------
def abi_solve(x, w, z0, alpha, maxiter, layout="natural", tol=0.0, reserved=0, shape=None, trace=None):
    """lasso_interior_point_solve directly: `reserved` and pitched / offset operands are not reachable from Python
    -> (status, z on the CPU, result struct)"""
    from lasso_amd import _native as nat
    n, d = x.shape
    k = w.shape[1]
    nan = float("nan")
    px, pw, pz0 = (place(t, layout, nan, device="cuda", name=nm) for t, nm in ((x, "x"), (w, "w"), (z0, "z0")))
    pz = place(torch.zeros(n, k), layout, SENTINEL, device="cuda", name="z", fill=SENTINEL)
    opts = nat.InteriorPointOptions(maxiter, 0, 0.1, tol, 1e-5, reserved)
    res = nat.InteriorPointResult()
    if trace is not None:
        res.trace = C.pointer(trace)
    L = nat.lib()
    ws = torch.empty(max(L.lasso_interior_point_workspace_bytes(n, d, k, nat.LASSO_F32), 16), dtype=torch.uint8, device="cuda")
    dd, kk = shape or (d, k)
    status = L.lasso_interior_point_solve(C.c_void_p(px.view.data_ptr()), max(px.ld, dd), C.c_void_p(pw.view.data_ptr()),
                                          max(pw.ld, kk), C.c_void_p(pz0.view.data_ptr()), max(pz0.ld, kk),
                                          C.c_void_p(pz.view.data_ptr()), max(pz.ld, kk), n, dd, kk, nat.LASSO_F32, alpha,
                                          C.byref(opts), C.byref(res), nat.ptr(ws), ws.numel(),
                                          nat.stream_ptr(torch.device("cuda", 0)))
    torch.cuda.synchronize()
    for p in (px, pw, pz0):
        p.check()
    pz.check(written=True)
    return status, pz.view.cpu(), res


def test_pitched_and_offset_operands_through_the_c_abi(cases):
    spec, g = CASES["odd"], load_case(cases, "odd")
    x, w, z0 = case_inputs(spec)
    bar = max(5e-5, 4.0 * float(g["spread_z"]))
    status, want, res = abi_solve(x, w, z0, spec["alpha"], 4)
    assert status == 0 and res.n_iter == 4 and res.status == 1
    assert float((want - torch.from_numpy(g["z32"])).abs().max()) <= bar
    for layout in ("pitched", "odd", "offset"):
        status, z, res = abi_solve(x, w, z0, spec["alpha"], 4, layout)
        assert status == 0 and res.n_iter == 4
        assert float((z - want).abs().max()) <= bar, layout


def test_refusals_of_the_c_abi_write_nothing():
    from lasso_amd import _native as nat
    x, w, z0 = case_inputs(CASES["small"])
    status, z, _ = abi_solve(x, w, z0, 0.3, 1, reserved=1)
    assert status == nat.LASSO_ERR_BAD_ARG and (z == SENTINEL).all()
    status, z, _ = abi_solve(x, w, z0, 0.3, 1, shape=(257, 24))
    assert status == nat.LASSO_ERR_UNSUPPORTED and (z == SENTINEL).all()
    status, z, _ = abi_solve(x, w, z0, 0.3, 1, shape=(40, 4097))
    assert status == nat.LASSO_ERR_UNSUPPORTED and (z == SENTINEL).all()
    status, z, res = abi_solve(x, w, torch.zeros_like(z0), 0.3, 1)      # not interior: refused after the start pass
    assert status == nat.LASSO_ERR_BAD_ARG and res.status == nat.INTERIOR_POINT_BAD_START and (z == SENTINEL).all()


# ---- 128 x 128 GEMM blocks, forced (LASSO_FORCE_BLOCKS_128) ---------------------------------------------------------------
# block_side() takes 128-blocks only from 2 x CUs blocks on, far above any shape here: the bit runs both products of the
# solve ([n,d] x W on W^T and [n,k] x W^T, StoreEpi) on Tile<128, 128>.  Shapes: more than one 128-block in a dimension
# and a nearly empty last one; contraction lengths for the three operand forms (a multiple of 32: LDS-DMA, of 4: 16-byte
# loads, odd: scalar loads) of both products.
F128 = [(130, 64, 288, 0.3, 3), (259, 36, 132, 0.3, 3), (131, 37, 131, 0.3, 3), (40, 200, 136, 0.3, 3), (1, 40, 24, 0.3, 3)]
_F128_MODEL = {}


def f128_model(n, d, k, alpha, maxiter):
    """the fresh-shape construction above, computed once per shape -> (x, w, z0, z64, i32, i64, bar, gap)"""
    key = (n, d, k)
    if key not in _F128_MODEL:
        x, w = recipe_xw(n, d, k, seed=22)
        z0 = ridge_start(x, w, alpha)
        kw = dict(alpha=alpha, maxiter=maxiter, tol=0.0)
        z32, _, i32 = interior_point_model.interior_point(x, w, z0, **kw)
        z64, _, i64 = interior_point_model.interior_point(x, w, z0, dtype=torch.float64, **kw)
        gap = float((z32.double() - z64).abs().max())
        _F128_MODEL[key] = (x, w, z0, z64, i32, i64, 4.0 * gap, gap)
    return _F128_MODEL[key]


def abi_solve_traced(x, w, z0, alpha, maxiter, layout="natural", reserved=0):
    """abi_solve with the per-iteration records -> (status, z, result struct, {obj, prim_feas, dual_feas, gap})"""
    from lasso_amd import _native as nat
    arrays = [(C.c_double * max(maxiter, 1))() for _ in range(4)]
    trace = nat.InteriorPointTrace(maxiter, 0, *arrays)
    status, z, res = abi_solve(x, w, z0, alpha, maxiter, layout, reserved=reserved, trace=trace)
    its = min(res.n_iter, maxiter) if status == 0 else 0
    return status, z, res, {key: list(a[:its]) for key, a in zip(("obj", "prim_feas", "dual_feas", "gap"), arrays)}


@pytest.mark.parametrize("reserved", [8, 0], ids=["f128", "s64"])
@pytest.mark.parametrize("n,d,k,alpha,maxiter", F128)
def test_forced_128_blocks_against_the_model(n, d, k, alpha, maxiter, reserved):
    from lasso_amd import _native as nat
    assert nat.FORCE_BLOCKS_128 == 8
    x, w, z0, z64, i32, i64, bar, gap = f128_model(n, d, k, alpha, maxiter)
    status, z, res, info = abi_solve_traced(x, w, z0, alpha, maxiter, reserved=reserved)
    assert status == 0
    dz = float((z.double() - z64).abs().max())
    tag = "%dx%dx%d_%s" % (n, d, k, "f128" if reserved else "s64")
    print("fresh %s: max|z - z64| = %.3g (bar %.3g)" % (tag, dz, bar))
    record_margins("interior_point/fresh_" + tag, dict(dz=dz, bar=bar, gap=gap))
    assert res.n_iter == maxiter and res.status == nat.INTERIOR_POINT_MAXITER
    assert dz <= bar
    for key in ("obj", "prim", "gap"):                       # the records, as test_fresh_shape_against_the_model
        want, got = np.array(i64[INFO_KEYS[key]]), np.array(info[INFO_KEYS[key]])
        model = np.array(i32[INFO_KEYS[key]])
        floor = 4.0 * float(torch.finfo(torch.float32).eps) * float(x.abs().max()) if key == "prim" else 0.0
        assert (np.abs(got - want) <= np.maximum(np.maximum(4.0 * np.abs(model - want), 1e-5 * np.abs(want)), floor)).all(), key


def test_forced_128_blocks_pitched_repeatable_and_refused():
    from lasso_amd import _native as nat
    n, d, k, alpha, maxiter = F128[1]
    x, w, z0, z64, _, _, bar, _ = f128_model(n, d, k, alpha, maxiter)
    force = nat.FORCE_BLOCKS_128
    _, a, _, ia = abi_solve_traced(x, w, z0, alpha, maxiter, reserved=force)
    _, b, _, ib = abi_solve_traced(x, w, z0, alpha, maxiter, reserved=force)
    assert torch.equal(a, b) and ia == ib                     # two forced solves are bitwise equal
    margins = {}
    for layout in ("pitched", "odd", "offset"):
        status, z, res = abi_solve(x, w, z0, alpha, maxiter, layout, reserved=force)
        assert status == 0 and res.n_iter == maxiter
        margins[layout] = float((z.double() - z64).abs().max())
        print("f128 %s: max|z - z64| = %.3g (bar %.3g), bitwise the natural forced solve: %s" % (layout, margins[layout], bar,
                                                                                                torch.equal(z, a)))
    record_margins("interior_point/layouts_%dx%dx%d_f128" % (n, d, k), dict(bar=bar, **margins))
    assert max(margins.values()) <= bar
    for bad in (force | 1, force | 4, force | (1 << 40)):
        status, z, _ = abi_solve(x, w, z0, alpha, 1, reserved=bad)
        assert status == nat.LASSO_ERR_BAD_ARG and (z == SENTINEL).all(), bad
