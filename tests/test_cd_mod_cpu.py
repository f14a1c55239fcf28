"""coord_descent_mod without a GPU: the Python surface equals the reference's, the C boundary declares and exports the
new symbols, refusals and asserts come before any native call, the host model (tests/cd_mod_model.py) reproduces the
fixture recorded from the reference, and without a GPU the solver fails loudly instead of computing on the CPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import cd_mod_model
from cd_mod_cases import CASES, MAX_ITER, REFERENCE_CASES, TOL, case_inputs, gap_f64, load_case, tol_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = ("sq48_zero_atom", "sq24_all_zero", "one_row", "n300_a08", "tiny", "d1", "k1")    # the model in a second or two


@pytest.fixture(scope="module")
def cases(golden):
    return golden("cd_mod_cases")


def test_python_surface():
    from lasso_amd.linear.solvers import coord_descent_mod
    from lasso_amd.linear.solvers.coordinate_descent import coord_descent_mod as direct
    import sys
    import lasso_amd.linear  # noqa: F401
    assert coord_descent_mod is direct
    sig = inspect.signature(coord_descent_mod)
    assert list(sig.parameters) == ["x", "W", "z0", "alpha", "max_iter", "tol", "return_info"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["z0"], d["alpha"], d["max_iter"], d["tol"], d["return_info"]) == (None, 1.0, 1000, 1e-4, False)
    # not an algorithm= arm: sparse_encode's table is as it was
    se = sys.modules["lasso_amd.linear.sparse_encode"]
    assert set(se._OFF_PATH_ALGOS) == {"iter-ridge", "interior-point", "split-bregman", "own"}
    assert "deviation" in coord_descent_mod.__doc__.lower() and "n_samples" in coord_descent_mod.__doc__


def test_symbols_declared_and_exported():
    from lasso_amd import _native
    text = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()
    for name in ("lasso_cd_mod_workspace_bytes", "lasso_cd_mod_solve"):
        assert name in text, name
    assert "#define LASSO_HIP_ABI_VERSION 7" in text          # additive: the version stays
    raw = ctypes.CDLL(_native.lib_path())
    assert hasattr(raw, "lasso_cd_mod_workspace_bytes") and hasattr(raw, "lasso_cd_mod_solve")
    L = _native.lib()
    small = L.lasso_cd_mod_workspace_bytes(64, 32, 128, _native.LASSO_F32)
    assert small >= 256 * 256 * 4 + 64 * 256 * 4
    assert L.lasso_cd_mod_workspace_bytes(4096, 256, 1024, _native.LASSO_F32) > small
    assert L.lasso_cd_mod_workspace_bytes(64, 32, 4097, _native.LASSO_F32) == 0
    for dtype in (_native.LASSO_BF16, _native.LASSO_F64):
        assert L.lasso_cd_mod_workspace_bytes(64, 32, 128, dtype) == 0


def _solve_status(L, nat, n=4, d=3, k=5, dtype=None, ldx=None, ldw=None, ldz=None, x=1, w=1, z=1, gap=1, ws=1,
                  max_iter=10, alpha=0.1):
    """lasso_cd_mod_solve with fake (never dereferenced) pointers: every refusal comes before the first HIP call"""
    p = lambda on: ctypes.c_void_p(0x1000 if on else 0)                                  # noqa: E731
    return L.lasso_cd_mod_solve(p(x), d if ldx is None else ldx, p(w), k if ldw is None else ldw, p(z),
                                k if ldz is None else ldz, 0, p(gap), None, None, n, d, k,
                                nat.LASSO_F32 if dtype is None else dtype, alpha, max_iter, 1e-4, None, None, p(ws), 0, None)


def test_c_abi_refusals_need_no_device():
    from lasso_amd import _native as nat
    L = nat.lib()
    bad, unsup = nat.LASSO_ERR_BAD_ARG, nat.LASSO_ERR_UNSUPPORTED
    assert _solve_status(L, nat, dtype=nat.LASSO_F64) == unsup
    assert _solve_status(L, nat, dtype=nat.LASSO_BF16) == unsup
    assert _solve_status(L, nat, k=4097) == unsup
    for kw in (dict(x=0), dict(w=0), dict(z=0), dict(gap=0), dict(ws=0), dict(ldx=2), dict(ldw=4), dict(ldz=4),
               dict(n=-1), dict(d=0), dict(k=0), dict(max_iter=-1), dict(alpha=-1.0)):
        assert _solve_status(L, nat, **kw) == bad, kw
    # a well-formed call gets as far as the workspace check (0 bytes given), still without a launch
    assert _solve_status(L, nat) == nat.LASSO_ERR_WORKSPACE


def test_refusals_come_before_any_native_call(monkeypatch):
    from lasso_amd import _native
    from lasso_amd.linear.solvers import coord_descent_mod

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_native, "lib", boom)
    monkeypatch.setattr(_native, "require_gpu", boom)
    x, w = torch.randn(24, 16), torch.randn(16, 40)
    with pytest.raises(AssertionError) as e:
        coord_descent_mod(torch.randn(24, 15), w)                    # :71
    assert "native call" not in str(e.value)
    with pytest.raises(AssertionError) as e:
        coord_descent_mod(x, w, z0=torch.zeros(16, 40))              # the reference's own shape is NOT ours when n != d
    assert "native call" not in str(e.value)
    for dt, word in ((torch.float64, "float64"), (torch.bfloat16, "bfloat16"), (torch.float16, "float16")):
        with pytest.raises(NotImplementedError, match=word):
            coord_descent_mod(x.to(dt), w.to(dt))
    with pytest.raises(NotImplementedError, match="float64"):
        coord_descent_mod(x, w, z0=torch.zeros(24, 40, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="4096"):
        coord_descent_mod(torch.randn(2, 3), torch.randn(3, 5000))
    with pytest.raises(ValueError):
        coord_descent_mod(x, w, max_iter=-1)
    with pytest.raises(RuntimeError):
        coord_descent_mod(x[0], w)


def test_no_gpu_is_a_native_error_not_a_cpu_result():
    from lasso_amd import _native
    from lasso_amd.linear.solvers import coord_descent_mod
    if torch.cuda.is_available():        # a GPU is visible: tests/test_cd_mod_gpu.py covers the solve
        return
    with pytest.raises(_native.NativeError):
        coord_descent_mod(torch.randn(4, 3), torch.randn(3, 5), alpha=0.1, max_iter=3)


def test_fixture_has_every_case(cases):
    for name, spec in CASES.items():
        g = load_case(cases, name)
        n, k = spec["n"], spec["k"]
        assert g["z32"].shape == (n, k) and g["z64"].shape == (n, k) and g["z64"].dtype == np.float64
        for key in ("gap32", "gap64", "sweeps32", "sweeps64", "certified", "decisive", "spread", "converged32",
                    "converged64", "rule_margin32", "rule_margin64"):
            assert g[key].shape == (n,), (name, key)
        assert ("z_ref" in g) == (name in REFERENCE_CASES)
        assert not (g["decisive"] & ~g["certified"]).any()
        if n > 1:
            assert g["decisive"].mean() >= 0.75, name
        # certified rows took the same sweeps and converged in both precisions
        c = g["certified"]
        assert (g["sweeps32"][c] == g["sweeps64"][c]).all() and g["converged32"][c].all() and g["converged64"][c].all()
        if name in REFERENCE_CASES:      # the model equalled the reference bit for bit when the fixture was made
            assert np.array_equal(g["z_ref"], g["z32"]) and np.array_equal(g["gap_ref"], g["gap32"])
    assert not cases["sq24_all_zero/z32"].any() and (cases["sq24_all_zero/sweeps32"] == 1).all()
    assert len(REFERENCE_CASES) == 4


@pytest.mark.parametrize("name", QUICK)
def test_model_reproduces_fixture(cases, name):
    spec, g = CASES[name], load_case(cases, name)
    x, w = case_inputs(spec)
    keep = x.clone(), w.clone()
    z, gap, info = cd_mod_model.coord_descent_mod(x, w, alpha=spec["alpha"], max_iter=MAX_ITER, tol=TOL)
    assert torch.equal(x, keep[0]) and torch.equal(w, keep[1])
    c = torch.from_numpy(g["decisive"])
    # another CPU may round a product differently: decisive rows keep their sweeps, and z within the recorded spread
    assert torch.equal(info["sweeps"][c], torch.from_numpy(g["sweeps32"])[c])
    bar = max(10 * float(g["spread"][g["decisive"]].max()), 1e-6 * float(np.abs(g["z32"]).max()))
    assert float((z - torch.from_numpy(g["z32"]))[c].abs().max()) <= bar
    if name == "sq24_all_zero":
        assert info["committed"] == int(g["committed32"]) == 0
    # the reported gap is the gap of the returned code, and `converged` is gap < tol_row
    tr = tol_row(x)
    g64 = gap_f64(z, x, w, spec["alpha"])
    assert float(((gap.double() - g64).abs() - 0.05 * tr.double()).max()) <= 0
    assert torch.equal(info["converged"], gap < TOL * x.pow(2).sum(1))


def test_model_sweep_limits_and_zero_row():
    spec = CASES["tiny"]
    x, w = case_inputs(spec)
    x[3] = 0.0
    z, gap, info = cd_mod_model.coord_descent_mod(x, w, alpha=spec["alpha"], max_iter=0, tol=TOL)
    assert not z.any() and torch.equal(gap, torch.full((40,), TOL + 1.)) and not info["sweeps"].any()
    z, gap, info = cd_mod_model.coord_descent_mod(x, w, alpha=spec["alpha"], max_iter=6, tol=TOL)
    assert info["sweeps"][3] == 6 and not info["converged"][3] and gap[3] == 0 and not z[3].any()
    unconv = ~info["converged"]
    assert (info["sweeps"][unconv] == 6).all()
    # warm start: in place, a nonzero start on a zero atom is kept
    w[:, 2] = 0.0
    z0 = torch.full((40, 5), 0.25)
    z, _, _ = cd_mod_model.coord_descent_mod(x, w, z0=z0, alpha=spec["alpha"], max_iter=50, tol=TOL)
    assert z is z0 and (z0[:, 2] == 0.25).all()
