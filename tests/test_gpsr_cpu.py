"""GPSR-Basic without a GPU: the host model (tests/gpsr_model.py) reproduces every golden case recorded from the
reference; the boundary declares and exports the new symbols; argument errors come before any HIP call; and
without a GPU the solver fails loudly instead of computing on the CPU."""
import ctypes
import inspect
import io
import os
import warnings
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import gpsr_model
from gpsr_cases import CASES, case_inputs, check_against_golden, load_case, same_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    return golden("gpsr_cases")


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_reproduces_reference(cases, name):
    spec, gold = CASES[name], load_case(cases, name)
    x, w, z0 = case_inputs(spec)
    keep = x.clone(), w.clone(), None if z0 is None else z0.clone()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        z, info = gpsr_model.gpsr_basic(x, w, spec["alpha"], x0=z0, return_info=True, **spec["kwargs"])
    check_against_golden(name, z, info, gold, 5e-5, caught)
    assert torch.equal(x, keep[0]) and torch.equal(w, keep[1]) and (z0 is None or torch.equal(z0, keep[2]))
    if name == "zero":
        assert not z.any() and info["iterations"] == 0


def test_golden_cases_are_certified(cases):
    """what the generator certified, re-read from the model's run: no decision is within 1e-4 |f| of its bound"""
    for name, spec in CASES.items():
        x, w, z0 = case_inputs(spec)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, info = gpsr_model.gpsr_basic(x, w, spec["alpha"], x0=z0, return_info=True, **spec["kwargs"])
        for fn, bound, f in info["decisions"]:
            assert abs(fn - bound) >= 0.5e-4 * abs(f), (name, fn, bound, f)


def test_model_verbose_lines_match_the_reference(cases):
    spec, gold = CASES["default"], load_case(cases, "default")
    x, w, z0 = case_inputs(spec)
    out = io.StringIO()
    with redirect_stdout(out):
        gpsr_model.gpsr_basic(x, w, spec["alpha"], x0=z0, verbose=2, **spec["kwargs"])
    ref = str(gold["stdout"])
    assert ref.count("\n") > 30
    ours, theirs = out.getvalue().splitlines(), ref.splitlines()
    assert len(ours) == len(theirs)
    for a, b in zip(ours, theirs):
        assert same_line(a, b), (a, b)


def test_symbols_declared_and_exported():
    from lasso_amd import _native
    text = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()
    for name in ("lasso_gpsr_workspace_bytes", "lasso_gpsr_solve", "lasso_gpsr_options", "lasso_gpsr_result",
                 "lasso_gpsr_trace", "lasso_solver_block_side", "#define LASSO_FORCE_BLOCKS_128 8"):
        assert name in text, name
    assert "#define LASSO_HIP_ABI_VERSION 7" in text          # additive: the version stays
    lib = ctypes.CDLL(_native.lib_path())
    assert hasattr(lib, "lasso_gpsr_workspace_bytes") and hasattr(lib, "lasso_gpsr_solve")
    assert hasattr(lib, "lasso_solver_block_side") and _native.FORCE_BLOCKS_128 == 8
    L = _native.lib()
    small = L.lasso_gpsr_workspace_bytes(64, 32, 128, _native.LASSO_F32)
    assert small > 10 * 64 * 128 * 4
    assert L.lasso_gpsr_workspace_bytes(4096, 256, 1024, _native.LASSO_F32) > small
    for dtype in (_native.LASSO_BF16, _native.LASSO_F64):
        assert L.lasso_gpsr_workspace_bytes(64, 32, 128, dtype) == 0
        res, opt = _native.GpsrResult(), _native.GpsrOptions()
        st = L.lasso_gpsr_solve(None, 32, None, 128, None, 0, None, 128, 64, 32, 128, dtype, 0.5,
                                ctypes.byref(opt), ctypes.byref(res), None, 0, None)
        assert st == _native.LASSO_ERR_UNSUPPORTED
    # the ctypes mirrors have the C layout (x86-64: 10 ints + 5 doubles; ...)
    assert ctypes.sizeof(_native.GpsrOptions) == 80
    assert ctypes.sizeof(_native.GpsrResult) == 64


def test_python_surface():
    from lasso_amd.linear.solvers import gpsr_basic
    import sys
    import lasso_amd.linear  # noqa: F401
    se = sys.modules["lasso_amd.linear.sparse_encode"]
    sig = inspect.signature(gpsr_basic)
    d = {k: v.default for k, v in sig.parameters.items()}
    assert list(sig.parameters)[:3] == ["x", "weight", "tau"]
    assert (d["x0"], d["stop_criterion"], d["tol"], d["maxiter"], d["miniter"], d["init"], d["continuation"],
            d["debias"], d["verbose"], d["return_info"]) == (None, 3, 1e-2, 1000, 5, 0, False, False, 0, False)
    assert "gpsr" not in se._OFF_PATH_ALGOS
    assert set(se._OFF_PATH_ALGOS) == {"iter-ridge", "interior-point", "split-bregman", "own"}


def test_argument_errors_come_before_any_hip_call(monkeypatch):
    from lasso_amd import _native
    from lasso_amd.linear import sparse_encode
    from lasso_amd.linear.solvers import gpsr_basic

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_native, "lib", boom)
    monkeypatch.setattr(_native, "require_gpu", boom)
    x, w = torch.randn(4, 3), torch.randn(3, 5)
    with pytest.raises(ValueError, match="Unknown stopping criterion"):
        gpsr_basic(x, w, 0.1, stop_criterion=5)
    with pytest.raises(ValueError, match="Unknown initialization option"):
        gpsr_basic(x, w, 0.1, init=3)
    with pytest.raises(TypeError, match="nonsense"):
        gpsr_basic(x, w, 0.1, nonsense=1)
    with pytest.raises(TypeError, match="nonsense"):
        sparse_encode(x, w, 0.1, algorithm="gpsr", nonsense=1)
    with pytest.raises(NotImplementedError, match="float64"):
        sparse_encode(x.double(), w.double(), 0.1, algorithm="gpsr")
    with pytest.raises(NotImplementedError, match="requires_grad"):
        sparse_encode(x, w.clone().requires_grad_(), 0.1, algorithm="gpsr")
    for other in ("iter-ridge", "interior-point", "split-bregman", "own"):
        with pytest.raises(NotImplementedError):
            sparse_encode(x, w, 0.1, algorithm=other)


def test_no_gpu_is_a_native_error_not_a_cpu_result():
    from lasso_amd import _native
    from lasso_amd.linear import sparse_encode
    if torch.cuda.is_available():        # a GPU is visible: tests/test_gpsr_gpu.py covers the solve
        return
    x, w = torch.randn(4, 3), torch.randn(3, 5)
    with pytest.raises(_native.NativeError):
        sparse_encode(x, w, 0.1, algorithm="gpsr", maxiter=3)
