"""lasso_amd.linear.utils on the device: batch_cholesky_solve on every tier in both dtypes against the recorded
reference (tests/golden/batch_solve_cases.npz, tests/batch_solve_cases.py), and ridge / lstsq against the inits they
were.  Every expectation comes from the fixture or from a CPU solve: no torch.linalg call on the device.

Bar: per system max|x - x_ref| / max|x_ref| <= max(floor, 4 x spread), floor 5e-5 (float32) / 1e-12 (float64), spread
measured by the generator (see tests/batch_solve_cases.py).  Achieved margins go to tests/margins.py ("batch_solve/...")."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import batch_solve_cases as bc
from layouts import SENTINEL, place, plans
from margins import record_margins
from ws_poison import MODES, Poison

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
WARNING = "Cholesky factorization failed. Reverting to LU decomposition..."
SPD = [n for n, s in bc.CASES.items() if s["kind"] in ("spd", "iter-ridge")]
FALLBACK = [n for n, s in bc.CASES.items() if s["kind"] in ("indef", "zerodiag", "nonsym")]


def _pairs(names):
    return [(n, k) for n in names for k in bc.dtypes_of(bc.CASES[n])]


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("batch_solve_cases")


def _utils():
    from lasso_amd.linear import utils
    return utils


@functools.lru_cache(maxsize=None)
def _inputs(name, key):
    """the recipe's CPU tensors: computed once, shared, never written"""
    return bc.inputs(bc.CASES[name], bc.DTYPES[key])


def _call(b, A):
    """-> x (on the device of b), info, the warnings' texts"""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        x, info = _utils().batch_cholesky_solve(b, A, return_info=True)
    return x, info, [str(c.message) for c in caught]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int64)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _tier(D, key):
    utils = _utils()
    dtype = bc.DTYPES[key]
    return "wave" if D <= utils.WAVE_CAP else "lds" if D <= utils.LDS_CAP[dtype] else "general"


# ---- golden cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,key", _pairs(SPD))
def test_golden_cholesky_route(fixture, name, key):
    spec, g = bc.CASES[name], bc.load_case(fixture, name)
    b, A = _inputs(name, key)
    bg, Ag = b.cuda(), A.cuda()
    x, info, said = _call(bg, Ag)
    assert said == []
    assert info == dict(route="cholesky", tier=_tier(spec["D"], key), bad_system=None, bad_minor=None)
    assert x.is_cuda and x.dtype == b.dtype and x.shape == b.shape
    assert x.data_ptr() not in (bg.data_ptr(), Ag.data_ptr())
    assert _same(bg.cpu(), b) and _same(Ag.cpu(), A)                         # operands bitwise unchanged
    rel = bc.rel_rows(x.cpu().numpy(), g["x" + key])
    print("batch_solve/%s/f%s: worst %.3g, bar %.3g" % (name, key, rel.max(), bc.bar(g, key)))
    record_margins("batch_solve/%s/f%s" % (name, key), dict(worst=float(rel.max()), bar=bc.bar(g, key), tier=info["tier"]))
    assert rel.max() <= bc.bar(g, key), rel
    x2, _, _ = _call(bg, Ag)
    assert _same(x2, x)                                                      # two calls, the same bits
    xc, infoc, _ = _call(b, A)                                               # CPU tensors are staged; the result is on b's device
    assert not xc.is_cuda and _same(xc, x.cpu()) and infoc == info


@pytest.mark.parametrize("name,key", [("d257_b5", "32"), ("d161_b5", "64")])
def test_a_workgroup_takes_a_second_system(fixture, name, key):
    """B = the general tier's workgroup count + 1 at D = LDS cap + 1: the batch is the case's five systems over and over"""
    from lasso_amd import _native as nat
    utils = _utils()
    spec, g = bc.CASES[name], bc.load_case(fixture, name)
    dtype = bc.DTYPES[key]
    assert spec["D"] == utils.LDS_CAP[dtype] + 1
    wgs = nat.lib().lasso_batch_solve_workgroups(10 ** 6, spec["D"], nat.DT[dtype])
    assert wgs == utils.GENERAL_WORKGROUPS
    B = wgs + 1
    b, A = _inputs(name, key)
    idx = torch.arange(B) % spec["B"]
    x5, info5, _ = _call(b.cuda(), A.cuda())
    x, info, said = _call(b.cuda()[idx.cuda()], A.cuda()[idx.cuda()])
    assert said == [] and info == info5 and info["tier"] == "general"
    assert _same(x.cpu(), x5.cpu()[idx])
    assert bc.rel_rows(x.cpu().numpy(), g["x" + key][idx.numpy()]).max() <= bc.bar(g, key)


# ---- the lower triangle alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,key", _pairs(["d2_b5", "d31_b7", "d97_b5", "d300_b2"]) + [("d257_b5", "32"), ("d161_b5", "64")])
def test_cholesky_route_reads_the_lower_triangle_only(name, key):
    b, A = _inputs(name, key)
    D = A.shape[1]
    upper = torch.triu(torch.ones(D, D, dtype=torch.bool), diagonal=1)
    clean, info, _ = _call(b.cuda(), A.cuda())
    for fill in (7.0, float("nan")):
        Ap = A.clone()
        Ap[:, upper] = fill
        x, infop, said = _call(b.cuda(), Ap.cuda())
        assert said == [] and infop == info and info["route"] == "cholesky"
        assert _same(x, clean), fill


# ---- systems are independent -----------------------------------------------------------------------------------------
def _abi(fn_name, b, A, batch_stride=None, x=None):
    """one C-ABI call on device tensors (A: [B,D,D] view with a unit last stride, or [D,D] with batch_stride=0)"""
    from lasso_amd import _native as nat
    utils = _utils()
    L = nat.lib()
    B, D = b.shape
    dt = nat.DT[b.dtype]
    if x is None:
        x = torch.full((B, D), SENTINEL, dtype=b.dtype, device=b.device)
    if batch_stride is None:
        batch_stride, lda = A.stride(0), A.stride(1)
    else:
        lda = A.stride(-2)
    ws = nat.workspace(b.device, L.lasso_batch_solve_workspace_bytes(B, D, dt), "batch_solve")
    res = utils.BatchSolveResult()
    status = getattr(L, fn_name)(nat.ptr(A), batch_stride, lda, nat.ptr(b), b.stride(0), nat.ptr(x), x.stride(0), B, D, dt,
                                 C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(b.device))
    nat.check(status)
    torch.cuda.synchronize()
    return x, res


@pytest.mark.parametrize("name,key", _pairs(["d31_b7", "d65_b5", "d300_b2"]))
def test_each_system_alone_equals_its_row_cholesky(name, key):
    b, A = _inputs(name, key)
    x, _, _ = _call(b.cuda(), A.cuda())
    for i in range(b.shape[0]):
        xi, _, _ = _call(b[i:i + 1].cuda(), A[i:i + 1].cuda())
        assert _same(xi[0], x[i]), i


@pytest.mark.parametrize("name,key", _pairs(["indef_d33_b5", "nonsym_d65_b3"]))
def test_each_system_alone_equals_its_row_lu(name, key):
    b, A = _inputs(name, key)
    bg, Ag = b.cuda(), A.cuda()
    x, res = _abi("lasso_batch_lu_solve", bg, Ag)
    assert res.bad_system == -1
    x2, _ = _abi("lasso_batch_lu_solve", bg, Ag)
    assert _same(x2, x)
    for i in range(b.shape[0]):
        xi, _ = _abi("lasso_batch_lu_solve", bg[i:i + 1].contiguous(), Ag[i:i + 1].contiguous())
        assert _same(xi[0], x[i]), i
    xa, info, said = _call(bg, Ag)                       # ... and it is what the Python call returns
    assert info["route"] == "lu" and _same(xa, x)


# ---- fallback --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,key", _pairs(FALLBACK))
def test_fallback_to_lu(fixture, name, key):
    spec, g = bc.CASES[name], bc.load_case(fixture, name)
    b, A = _inputs(name, key)
    x, info, said = _call(b.cuda(), A.cuda())
    assert said == [WARNING] and str(fixture["warning"]) == WARNING
    failing = np.nonzero(g["info" + key])[0]
    assert info == dict(route="lu", tier=_tier(spec["D"], key), bad_system=int(failing[0]),
                        bad_minor=int(g["info" + key][failing[0]]))
    rel = bc.rel_rows(x.cpu().numpy(), g["x" + key])
    print("batch_solve/%s/f%s: worst %.3g, bar %.3g" % (name, key, rel.max(), bc.bar(g, key)))
    record_margins("batch_solve/%s/f%s" % (name, key), dict(worst=float(rel.max()), bar=bc.bar(g, key), route="lu"))
    assert rel.max() <= bc.bar(g, key), rel


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("D", [8, 33])
def test_singular_systems_raise_like_torch(dtype, D):
    key = "32" if dtype == F32 else "64"
    b, A = _inputs("d33_b5", key)
    b, A = b[:, :D].clone(), A[:, :D, :D].clone()         # (leading principal blocks of SPD matrices are SPD)
    Az = A.clone()
    Az[3] = 0.0                                          # an all-zero system
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with pytest.raises(torch.linalg.LinAlgError, match=r"\(Batch element 3\): The solver failed because the input matrix is singular\."):
            _utils().batch_cholesky_solve(b.cuda(), Az.cuda())
    assert [str(c.message) for c in caught] == [WARNING]
    try:                                                 # torch's own text on the CPU, word for word
        torch.linalg.solve(Az, b.unsqueeze(2))
        raise AssertionError("torch solved a singular system")
    except torch.linalg.LinAlgError as e:
        want = str(e)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(torch.linalg.LinAlgError) as got:
            _utils().batch_cholesky_solve(b.cuda(), Az.cuda())
    assert str(got.value) == want
    j = D // 2
    Aj = A.clone()
    for i in (4, 2):                                     # row and column j zero in two systems: the lowest is named
        Aj[i, j, :] = 0.0
        Aj[i, :, j] = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(torch.linalg.LinAlgError, match=r"\(Batch element 2\)"):
            _utils().batch_cholesky_solve(b.cuda(), Aj.cuda())


# ---- non-finite inputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["32", "64"])
@pytest.mark.parametrize("name", [n for n, v in bc.NONFINITE.items() if v[1] == "b"])
def test_nonfinite_right_hand_side_stays_in_its_system(fixture, name, key):
    base, _, system, _, _ = bc.NONFINITE[name]
    g = bc.load_case(fixture, "nonfinite_" + name)
    b, A = bc.nonfinite_inputs(name, bc.DTYPES[key])
    x, info, said = _call(b.cuda(), A.cuda())
    assert said == [] and info["route"] == "cholesky"
    clean, _, _ = _call(_inputs(base, key)[0].cuda(), A.cuda())
    others = [i for i in range(b.shape[0]) if i != system]
    assert _same(x[others], clean[others])
    assert np.array_equal(bc.classes(x.cpu().numpy()), bc.classes(g["x" + key])), (bc.classes(x.cpu().numpy())[system],
                                                                                   bc.classes(g["x" + key])[system])


@pytest.mark.parametrize("key", ["32", "64"])
def test_nan_in_a_lower_triangle_takes_the_lu_route(fixture, key):
    base, _, system, _, _ = bc.NONFINITE["a_nan"]
    g = bc.load_case(fixture, "nonfinite_a_nan")
    b, A = bc.nonfinite_inputs("a_nan", bc.DTYPES[key])
    x, info, said = _call(b.cuda(), A.cuda())
    assert said == [WARNING] and info["route"] == "lu" and info["bad_system"] == system
    x = x.cpu().numpy()
    assert np.array_equal(bc.classes(x), bc.classes(g["x" + key]))
    assert np.isnan(x[system]).all()
    others = [i for i in range(b.shape[0]) if i != system]
    rel = bc.rel_rows(x[others], g["x" + key][others])
    assert rel.max() <= bc.bar(g, key), rel


# ---- layouts, through the C ABI --------------------------------------------------------------------------------------
LAYOUT_CASES = [("lasso_batch_chol_solve", "d31_b7", "32"), ("lasso_batch_chol_solve", "d31_b7", "64"),
                ("lasso_batch_chol_solve", "d97_b5", "32"), ("lasso_batch_chol_solve", "d257_b5", "32"),
                ("lasso_batch_chol_solve", "d161_b5", "64"), ("lasso_batch_lu_solve", "indef_d33_b5", "32"),
                ("lasso_batch_lu_solve", "nonsym_d65_b3", "64")]


@pytest.mark.parametrize("fn,name,key", LAYOUT_CASES)
def test_pitched_odd_and_offset_operands(fn, name, key):
    b, A = _inputs(name, key)
    B, D = b.shape
    anchor = None
    for tag, plan in plans(("a", "b", "x")):
        pa = place(A.reshape(B * D, D), plan["a"], float("nan"), device="cuda", name="a")
        pb = place(b, plan["b"], float("nan"), device="cuda", name="b")
        px = place(b, plan["x"], SENTINEL, device="cuda", name="x", fill=SENTINEL)
        Av = pa.view.as_strided((B, D, D), (D * pa.ld, pa.ld, 1), pa.view.storage_offset())
        x, res = _abi(fn, pb.view, Av, x=px.view)
        assert res.bad_system == -1
        pa.check()
        pb.check()
        px.check(written=True)                           # the sentinel padding intact
        got = px.view.cpu().contiguous()
        assert not torch.isnan(got).any(), tag
        if anchor is None:
            anchor = got
        assert _same(got, anchor), tag


@pytest.mark.parametrize("fn,name,key", [c for c in LAYOUT_CASES if c[1] != "nonsym_d65_b3"])
def test_batch_stride_zero(fn, name, key):
    """one matrix for every system (what G.expand(n, -1, -1) hands the reference)"""
    b, A = _inputs(name, key)
    bg = b.cuda()
    one = A[0].cuda().contiguous()
    want, _ = _abi(fn, bg, one.expand(b.shape[0], -1, -1).contiguous())
    got, _ = _abi(fn, bg, one, batch_stride=0)
    assert _same(got, want)
    if fn.endswith("chol_solve"):                        # ... and through Python, which passes the expanded view as it is
        x, info, _ = _call(bg, one.expand(b.shape[0], -1, -1))
        assert _same(x, want)


# ---- scratch and stream ----------------------------------------------------------------------------------------------
SCRATCH_CASES = [("d31_b7", "32"), ("d97_b5", "64"), ("d257_b5", "32"), ("d161_b5", "64"), ("indef_d97_b5", "32"),
                 ("zerodiag_d34_b3", "64")]


@pytest.mark.parametrize("name,key", SCRATCH_CASES)
def test_poisoned_scratch(name, key):
    b, A = _inputs(name, key)
    anchor = None
    for mode in MODES:
        bg, Ag = b.cuda(), A.cuda()
        torch.cuda.synchronize()
        with Poison(mode).installed() as poison:             # (the guards are checked on the way out)
            x, info, _ = _call(bg, Ag)
            got = x.cpu()
            torch.cuda.synchronize()
        assert poison.requests, "the call asked for no workspace: the patch did not reach it"
        if anchor is None:
            anchor = (got, info)
        assert _same(got, anchor[0]) and info == anchor[1], mode


@pytest.mark.parametrize("name,key", [("d31_b7", "32"), ("d161_b5", "64"), ("indef_d97_b5", "32")])
def test_late_side_stream(name, key):
    """the call on a side stream whose operands are still NaN when the host reaches the library (the harness of
    tests/test_workspace_gpu.py): a launch on another stream would read them early"""
    from test_workspace_gpu import _run_late
    b, A = _inputs(name, key)
    want, info_want, _ = _call(b.cuda(), A.cuda())

    def call(ops):
        x, info, said = _call(ops["b"], ops["A"])
        return dict(x=x), dict(info=info, said=said)
    tensors, host = _run_late(call, dict(b=b, A=A))
    assert _same(tensors["x"], want.cpu()) and host["info"] == info_want


# ---- ridge / lstsq ---------------------------------------------------------------------------------------------------
def test_ridge_and_lstsq_are_the_inits(golden):
    from lasso_amd.linear import initialize_code
    utils = _utils()
    g = golden("init_modes")
    for tag in ("under", "over"):
        X, W = torch.from_numpy(g[tag + "_X"]).cuda(), torch.from_numpy(g[tag + "_W"]).cuda()
        r = utils.ridge(X.T, W, 0.3).T
        assert _same(r, initialize_code(X, W, 0.3, "ridge")) and r.shape == (X.shape[0], W.shape[1])
        assert (r.cpu() - torch.from_numpy(g[tag + "_z0_ridge"])).abs().max().item() <= 5e-5      # tests/test_fista_gpu.py
        q = utils.lstsq(X.T, W).T
        assert _same(q, initialize_code(X, W, 0.3, "lstsq"))
        assert (q.cpu() - torch.from_numpy(g[tag + "_z0_lstsq"])).abs().max().item() <= 5e-5
        assert utils.ridge(X.T, W).shape == (W.shape[1], X.shape[0])             # alpha defaults to 1e-4
    with pytest.raises(RuntimeError, match="not positive definite"):
        utils.ridge(X.T, torch.zeros_like(W), alpha=0.0)                         # utils.py:36-38
