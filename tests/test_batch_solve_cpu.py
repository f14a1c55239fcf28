"""lasso_amd.linear.utils without a device: the module and its four names, their signatures against the recorded
reference's (tests/golden/batch_solve_cases.npz), the fixture's self-consistency, the C ABI's host-side refusals and
every refusal of batch_cholesky_solve before a native call."""
import ctypes as C
import inspect
import json

import numpy as np
import pytest
import torch

import batch_solve_cases as bc

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("batch_solve_cases")


def test_module_exports_the_reference_names():
    from lasso_amd.linear import utils
    for name in ("qr", "lstsq", "ridge", "batch_cholesky_solve"):
        assert callable(getattr(utils, name)), name
    assert sorted(utils.__all__) == ["batch_cholesky_solve", "lstsq", "qr", "ridge"]
    from lasso_amd.linear.utils import ridge, lstsq, batch_cholesky_solve      # noqa: F401  (the drop-in import)


def test_utils_is_an_attribute_of_linear():
    import lasso_amd.linear
    import lasso_amd.linear.utils as utils
    assert lasso_amd.linear.utils is utils
    import lasso_amd
    assert lasso_amd.linear.utils is utils


def test_signatures_match_the_recorded_reference(fixture):
    from lasso_amd.linear import utils
    want = json.loads(str(fixture["signatures"]))
    assert sorted(want) == ["batch_cholesky_solve", "lstsq", "qr", "ridge"]
    for name, params in want.items():
        sig = inspect.signature(getattr(utils, name)).parameters
        mine = [[p, None if v.default is inspect.Parameter.empty else v.default] for p, v in sig.items()]
        if name == "batch_cholesky_solve":                  # the project's one extra keyword, behind the reference's
            assert mine[-1] == ["return_info", False]
            mine = mine[:-1]
        assert mine == params, (name, mine, params)


def test_constants_are_the_library_s():
    from lasso_amd import _native as nat
    from lasso_amd.linear import utils
    L = nat.lib()
    for dtype, key in ((F32, "32"), (F64, "64")):
        dt = nat.DT[dtype]
        assert L.lasso_batch_solve_tier_cap(dt, 0) == utils.WAVE_CAP == 32
        assert L.lasso_batch_solve_tier_cap(dt, 1) == utils.LDS_CAP[dtype] == bc.LDS_CAP[key]
        assert L.lasso_batch_solve_tier_cap(dt, 2) == utils.CAP[dtype] == bc.CAP[key]
        # one workgroup per system up to the fixed count at LDS cap + 1; none on the other tiers
        assert L.lasso_batch_solve_workgroups(10 ** 6, utils.LDS_CAP[dtype] + 1, dt) == utils.GENERAL_WORKGROUPS
        assert L.lasso_batch_solve_workgroups(3, utils.LDS_CAP[dtype] + 1, dt) == 3
        assert L.lasso_batch_solve_workgroups(10 ** 6, utils.LDS_CAP[dtype], dt) == 0
        # the scratch is a fixed budget: it stops growing with the batch
        big = L.lasso_batch_solve_workspace_bytes(10 ** 6, utils.CAP[dtype], dt)
        assert 0 < big - 4 * 10 ** 6 <= (256 << 20) + 4096
        assert L.lasso_batch_solve_workspace_bytes(5, utils.CAP[dtype] + 1, dt) == 0
    assert L.lasso_batch_solve_workspace_bytes(5, 8, nat.LASSO_BF16) == 0
    assert L.lasso_batch_solve_workspace_bytes(0, 8, nat.LASSO_F32) == 0


def test_c_abi_refusals_before_any_hip_call():
    from lasso_amd import _native as nat
    from lasso_amd.linear import utils
    L = nat.lib()
    BAD, UNS, WSP = nat.LASSO_ERR_BAD_ARG, nat.LASSO_ERR_UNSUPPORTED, nat.LASSO_ERR_WORKSPACE
    res = utils.BatchSolveResult()
    r, p, none = C.byref(res), C.c_void_p(256), C.c_void_p(0)
    big = 1 << 30
    for fn in (L.lasso_batch_chol_solve, L.lasso_batch_lu_solve):
        assert fn(none, 64, 8, p, 8, p, 8, 3, 8, 0, r, p, big, none) == BAD
        assert fn(p, 64, 8, none, 8, p, 8, 3, 8, 0, r, p, big, none) == BAD
        assert fn(p, 64, 8, p, 8, none, 8, 3, 8, 0, r, p, big, none) == BAD
        assert fn(p, 64, 8, p, 8, p, 8, 3, 8, 0, none, p, big, none) == BAD
        assert fn(p, 64, 8, p, 8, p, 8, 3, 8, 0, r, none, big, none) == BAD
        assert fn(p, 64, 8, p, 8, p, 8, 0, 8, 0, r, p, big, none) == BAD          # sizes
        assert fn(p, 64, 8, p, 8, p, 8, -1, 8, 0, r, p, big, none) == BAD
        assert fn(p, 64, 8, p, 8, p, 8, 3, 0, 0, r, p, big, none) == BAD
        assert fn(p, 64, 7, p, 8, p, 8, 3, 8, 0, r, p, big, none) == BAD          # pitches
        assert fn(p, 64, 8, p, 7, p, 8, 3, 8, 0, r, p, big, none) == BAD
        assert fn(p, 64, 8, p, 8, p, 7, 3, 8, 0, r, p, big, none) == BAD
        assert fn(p, -1, 8, p, 8, p, 8, 3, 8, 0, r, p, big, none) == BAD
        assert fn(p, 64, 8, p, 8, p, 8, 3, 8, 1, r, p, big, none) == UNS          # bf16
        assert fn(p, 0, 1025, p, 1025, p, 1025, 3, 1025, 0, r, p, big, none) == UNS
        assert b"1024" in L.lasso_hip_last_error()
        assert fn(p, 0, 513, p, 513, p, 513, 3, 513, 2, r, p, big, none) == UNS
        assert b"512" in L.lasso_hip_last_error()
        need = L.lasso_batch_solve_workspace_bytes(3, 8, 0)
        assert fn(p, 64, 8, p, 8, p, 8, 3, 8, 0, r, p, need - 1, none) == WSP


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_fixture_is_self_consistent(fixture, name):
    """torch's own cholesky_ex / cholesky_solve / linalg.solve on the recipe reproduce what the reference returned"""
    spec = bc.CASES[name]
    g = bc.load_case(fixture, name)
    for key in bc.dtypes_of(spec):
        b, A = bc.inputs(spec, bc.DTYPES[key])
        assert b.shape == (spec["B"], spec["D"]) and A.shape == (spec["B"], spec["D"], spec["D"])
        L, info = torch.linalg.cholesky_ex(A)
        assert np.array_equal(info.numpy(), g["info" + key])
        warned = bool(g["warned" + key])
        assert warned == bool((info != 0).any()) == (spec["kind"] in ("indef", "zerodiag", "nonsym"))
        x = torch.linalg.solve(A, b.unsqueeze(2)) if warned else torch.cholesky_solve(b.unsqueeze(2), L)
        ref = g["x" + key]
        assert ref.dtype == (np.float32 if key == "32" else np.float64) and np.isfinite(ref).all()
        # (another thread count may reorder a sum inside LAPACK: the bar the GPU tests use, not bitwise)
        assert bc.rel_rows(x.squeeze(2).numpy(), ref).max() <= bc.bar(g, key)
        assert 0.0 <= float(g["spread" + key]) <= bc.SPREAD_CAP


def test_fixture_nonfinite_cases(fixture):
    assert str(fixture["warning"]) == "Cholesky factorization failed. Reverting to LU decomposition..."
    for name, (base, which, system, index, value) in bc.NONFINITE.items():
        for key in bc.DTYPES:
            g = bc.load_case(fixture, "nonfinite_" + name)
            x = g["x" + key]
            assert bool(g["warned" + key]) == (which == "A")
            others = [i for i in range(x.shape[0]) if i != system]
            assert np.isfinite(x[others]).all() and not np.isfinite(x[system]).any()


def _spd(B, D, dtype):
    A = torch.eye(D, dtype=dtype).expand(B, D, D).clone()
    return torch.ones(B, D, dtype=dtype), A


def test_refusals_come_before_any_native_call(monkeypatch):
    from lasso_amd import _native as nat
    from lasso_amd.linear import utils

    def no_native(*a, **k):
        raise AssertionError("a native call was reached")
    monkeypatch.setattr(nat, "lib", no_native)
    monkeypatch.setattr(nat, "require_gpu", no_native)
    for dtype in (torch.bfloat16, torch.float16):
        b, A = _spd(2, 4, dtype)
        with pytest.raises(NotImplementedError, match=str(dtype).replace("torch.", "")):
            utils.batch_cholesky_solve(b, A)
    b, A = _spd(2, 4, F32)
    with pytest.raises(NotImplementedError, match="one dtype"):
        utils.batch_cholesky_solve(b, A.double())
    with pytest.raises(NotImplementedError, match="one dtype"):
        utils.batch_cholesky_solve(b.double(), A)
    for dtype in (F32, F64):
        cap = utils.CAP[dtype]
        with pytest.raises(NotImplementedError, match="cap"):
            utils.batch_cholesky_solve(torch.ones(1, cap + 1, dtype=dtype), torch.eye(cap + 1, dtype=dtype)[None])
    with pytest.raises(NotImplementedError, match=str(utils.CAP[F32])):
        utils.batch_cholesky_solve(torch.ones(1, 1025), torch.eye(1025)[None])
    for which in (0, 1):
        b, A = _spd(2, 4, F32)
        (b, A)[which].requires_grad_(True)
        with pytest.raises(NotImplementedError, match="requires_grad"):
            utils.batch_cholesky_solve(b, A)
        with torch.no_grad():                                # (outside grad mode the flag means nothing -- but then the
            with pytest.raises(AssertionError, match="native call"):      # call goes on to the device)
                utils.batch_cholesky_solve(b, A)
    with pytest.raises(AssertionError):
        utils.batch_cholesky_solve(torch.ones(4), torch.eye(4)[None])
    with pytest.raises(AssertionError):
        utils.batch_cholesky_solve(torch.ones(1, 4), torch.eye(4))
    with pytest.raises(AssertionError):
        utils.batch_cholesky_solve(torch.ones(2, 4), torch.eye(4)[None])
    with pytest.raises(NotImplementedError, match="2-D"):
        utils.lstsq(torch.ones(2, 4, 1), torch.ones(2, 4, 3))


def test_empty_batch_without_a_native_call(monkeypatch):
    from lasso_amd import _native as nat
    from lasso_amd.linear import utils

    def no_native(*a, **k):
        raise AssertionError("a native call was reached")
    monkeypatch.setattr(nat, "lib", no_native)
    monkeypatch.setattr(nat, "require_gpu", no_native)
    for dtype in (F32, F64):
        x, info = utils.batch_cholesky_solve(torch.ones(0, 7, dtype=dtype), torch.ones(0, 7, 7, dtype=dtype), return_info=True)
        assert x.shape == (0, 7) and x.dtype == dtype
        assert info == dict(route="cholesky", tier="wave", bad_system=None, bad_minor=None)
        assert utils.batch_cholesky_solve(torch.ones(0, 7, dtype=dtype), torch.ones(0, 7, 7, dtype=dtype)).shape == (0, 7)


def test_qr_is_the_reference_s_shim():
    from lasso_amd.linear import utils
    A = torch.randn(7, 4, generator=torch.Generator().manual_seed(0))
    q, r = utils.qr(A)
    q2, r2 = torch.linalg.qr(A, mode="reduced")
    assert torch.equal(q, q2) and torch.equal(r, r2) and q.shape == (7, 4)


def test_ridge_and_lstsq_off_the_kernels_follow_torch():
    """float64 tensors go to torch.linalg: the reference's own arithmetic, on the CPU here"""
    from lasso_amd.linear import utils, initialize_code
    g = torch.Generator().manual_seed(1)
    A, b = torch.randn(12, 5, generator=g, dtype=F64), torch.randn(12, 3, generator=g, dtype=F64)
    x = utils.ridge(b, A, alpha=0.1)
    want = torch.linalg.solve(A.T @ A + 0.1 * torch.eye(5, dtype=F64), A.T @ b)
    assert x.shape == (5, 3) and torch.allclose(x, want, rtol=1e-10, atol=1e-12)
    assert torch.equal(initialize_code(b.T, A, 0.1, "ridge"), utils.ridge(b, A, alpha=0.1).T)
    x = utils.lstsq(b, A)
    assert x.shape == (5, 3) and torch.allclose(x, torch.linalg.lstsq(A, b).solution, rtol=1e-9, atol=1e-11)
    wide = torch.randn(4, 9, generator=g, dtype=F64)
    x = utils.lstsq(b[:4], wide)
    assert x.shape == (9, 3) and torch.allclose(wide @ x, b[:4], rtol=1e-9, atol=1e-11)
    assert torch.equal(initialize_code(b.T, A, 0.1, "lstsq"), utils.lstsq(b, A).T)
    with pytest.raises(RuntimeError, match="not positive definite"):
        utils.ridge(torch.zeros(6, 2, dtype=F64), torch.zeros(6, 4, dtype=F64), alpha=0.0)
