"""Convolutional GPSR-Basic without a GPU: the host model (tests/gpsr_conv_model.py) matches every golden case
recorded from the reference on this CPU; argument errors come before any native call; the boundary declares and
exports the two entry points; and without a GPU the solver fails loudly instead of computing on the CPU."""
import ctypes
import inspect
import os
import warnings

import numpy as np
import pytest
import torch

import gpsr_conv_model
from gpsr_conv_cases import CASES, case_inputs, load_case, rows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    return golden("gpsr_conv_cases")


def model(spec, **extra):
    x, w, z0 = case_inputs(spec)
    return gpsr_conv_model.gpsr_conv2d(x, w, spec["tau"], z0=z0, stride=spec["stride"], padding=spec["padding"],
                                       return_info=True, **dict(spec["kwargs"], **extra))


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_matches_the_recorded_reference(cases, name):
    """counts exactly; z within the float32-float64 gap the generator recorded for this case (another CPU's
    convolutions may sum in another order than the generator's did)"""
    spec, gold = CASES[name], load_case(cases, name)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        z, info = model(spec)
    n_main, gap = int(gold["n_iter"]), float(gold["model_gap"])
    assert info["iterations"] == n_main + int(gold["db_iters"])
    assert list(info["trials"]) == list(gold["trials"])
    assert len(info["objective"]) == n_main
    rows = gold["z_rows"]
    dz = float(np.abs(rows_of(z).numpy()[rows] - gold["z"]).max())
    print(name, "max|dz| %.3g, recorded float32-float64 gap %.3g" % (dz, gap))
    assert dz <= gap, (name, dz, gap)
    np.testing.assert_allclose(info["objective"], gold["objective"], rtol=1e-6, err_msg=name)
    np.testing.assert_allclose(info["accepted_lambda"], gold["lam"], rtol=1e-5, err_msg=name)
    assert sorted(str(c.message) for c in caught) == sorted(m for m in str(gold["warnings"]).split("\n") if m)
    if name == "zero":
        assert not z.any() and info["iterations"] == 0
    if name == "debias":
        assert int(gold["db_iters"]) > 0
    if name == "search":
        assert max(gold["trials"]) > 1


def test_golden_cases_are_certified(cases):
    """what the generator certified, re-read from the model's run and from the fixture"""
    for name, spec in CASES.items():
        gold = load_case(cases, name)
        assert float(gold["decision_margin"]) >= 1e-4, name
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, info = model(spec)
        for fn, bound, f in info["decisions"]:
            assert abs(fn - bound) >= 0.5e-4 * abs(f), (name, fn, bound, f)
        for crit, tol, crit_id in info["stops"]:
            if np.isfinite(crit):
                assert crit != tol if crit_id == 0 else abs(crit - tol) >= 0.005 * abs(tol), (name, crit, tol)


def test_python_surface():
    from lasso_amd.conv2d import gpsr_conv2d
    from lasso_amd.linear.solvers import gpsr_basic
    sig = inspect.signature(gpsr_conv2d)
    d = {k: v.default for k, v in sig.parameters.items()}
    assert list(sig.parameters)[:6] == ["x", "weight", "tau", "z0", "stride", "padding"]
    assert (d["z0"], d["stride"], d["padding"]) == (None, 1, 0)
    lin = {k: v.default for k, v in inspect.signature(gpsr_basic).parameters.items()}
    for key in ("stop_criterion", "tol", "maxiter", "miniter", "init", "continuation", "debias", "verbose", "return_info"):
        assert d[key] == lin[key], key


def test_argument_errors_come_before_any_native_call(monkeypatch):
    from lasso_amd import _native
    from lasso_amd.conv2d import gpsr_conv2d

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_native, "lib", boom)
    monkeypatch.setattr(_native, "require_gpu", boom)
    x, w = torch.randn(2, 3, 9, 9), torch.randn(5, 3, 3, 3)
    with pytest.raises(ValueError, match="Unknown stopping criterion"):
        gpsr_conv2d(x, w, 0.1, stop_criterion=5)
    with pytest.raises(ValueError, match="Unknown initialization option"):
        gpsr_conv2d(x, w, 0.1, init=3)
    with pytest.raises(TypeError, match="nonsense"):
        gpsr_conv2d(x, w, 0.1, nonsense=1)
    with pytest.raises(NotImplementedError, match="float64"):
        gpsr_conv2d(x.double(), w.double(), 0.1)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        gpsr_conv2d(x.bfloat16(), w.bfloat16(), 0.1)
    with pytest.raises(NotImplementedError, match="requires_grad"):
        gpsr_conv2d(x, w.clone().requires_grad_(), 0.1)
    # geometry: conv_transpose2d of the code does not give back the image
    with pytest.raises(RuntimeError, match="must match the size of x"):
        gpsr_conv2d(x, w, 0.1, z0=torch.zeros(2, 5, 6, 7))                       # 8 x 9 != 9 x 9
    with pytest.raises(RuntimeError, match="must match the size of x"):
        gpsr_conv2d(torch.randn(2, 3, 10, 10), w, 0.1, stride=2)                 # (10 - 3) % 2 != 0
    with pytest.raises(RuntimeError, match="shape mismatch"):
        gpsr_conv2d(x, torch.randn(5, 2, 3, 3), 0.1)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        gpsr_conv2d(x, w, 0.1, z0=torch.zeros(2, 4, 7, 7))


def test_abi_surface():
    from lasso_amd import _native
    text = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()
    for name in ("lasso_conv_gpsr_workspace_bytes", "lasso_conv_gpsr_solve", "lasso_conv_gpsr_form"):
        assert name in text, name
    assert "#define LASSO_HIP_ABI_VERSION 7" in text          # additive: the version stays
    raw = ctypes.CDLL(_native.lib_path())
    assert hasattr(raw, "lasso_conv_gpsr_workspace_bytes") and hasattr(raw, "lasso_conv_gpsr_solve")
    L = _native.lib()
    geom = lambda N: (N, 3, 16, 16, 16, 12, 12, 5, 5, 1, 1, 0, 0)     # noqa: E731
    small = L.lasso_conv_gpsr_workspace_bytes(*geom(4))
    assert small > 10 * 4 * 12 * 12 * 16 * 4
    assert L.lasso_conv_gpsr_workspace_bytes(*geom(64)) > small
    bad = (4, 3, 16, 16, 16, 11, 12, 5, 5, 1, 1, 0, 0)                # (11 - 1) + 5 != 16
    assert L.lasso_conv_gpsr_workspace_bytes(*bad) == 0

    def solve(geometry, dtype, stop_criterion=3, with_pointers=True):
        res, opt = _native.GpsrResult(), _native.GpsrOptions()
        opt.stop_criterion, opt.maxiter, opt.lambda_backtrack, opt.mu = stop_criterion, 3, 0.5, 0.1
        ptr = ctypes.c_void_p(256) if with_pointers else None        # never dereferenced: every answer comes first
        return L.lasso_conv_gpsr_solve(ptr, ptr, None, ptr, *geometry, dtype, 0.5, ctypes.byref(opt), ctypes.byref(res),
                                       ptr, 1 << 40, None)
    assert solve(geom(4), _native.LASSO_F64) == _native.LASSO_ERR_UNSUPPORTED
    assert solve(geom(4), _native.LASSO_BF16) == _native.LASSO_ERR_UNSUPPORTED
    assert solve(bad, _native.LASSO_F32) == _native.LASSO_ERR_BAD_ARG
    huge = (3000, 1, 64, 64, 4, 64, 64, 1, 1, 1, 1, 0, 0)            # 12.3 M code pixels: beyond 32-bit block offsets
    assert L.lasso_conv_gpsr_workspace_bytes(*huge) == 0 and L.lasso_conv_gpsr_form(*huge, 0) == b""
    assert solve(huge, _native.LASSO_F32) == _native.LASSO_ERR_UNSUPPORTED
    assert L.lasso_conv_gpsr_form(*geom(4), 1) == b"patches"
    assert solve(geom(4), _native.LASSO_F32, stop_criterion=7) == _native.LASSO_ERR_BAD_ARG
    assert solve(geom(4), _native.LASSO_F32, with_pointers=False) == _native.LASSO_ERR_BAD_ARG      # null pointers
    assert solve(geom(0), _native.LASSO_F32, with_pointers=False) == _native.LASSO_OK               # N = 0: nothing to do


def test_no_gpu_is_a_native_error_not_a_cpu_result():
    from lasso_amd import _native
    from lasso_amd.conv2d import gpsr_conv2d
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: tests/test_gpsr_conv_gpu.py covers the solve")
    x, w = torch.randn(2, 3, 9, 9), torch.randn(5, 3, 3, 3)
    with pytest.raises(_native.NativeError):
        gpsr_conv2d(x, w, 0.1, maxiter=3)
