"""iterative_ridge without a GPU: the Python surface equals the reference's, the C boundary declares and exports the new
symbols and its structs have the size of their ctypes mirrors, the workspace is linear in n, refusals come before any
native call, the host model (tests/iter_ridge_model.py) reproduces the fixture recorded from the reference, and every
stored case satisfies the caps it was admitted under."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import iter_ridge_model
from iter_ridge_cases import CASES, SPREAD_F_CAP, SPREAD_Z_CAP, case_inputs, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    return golden("iter_ridge_cases")


def test_python_surface():
    import lasso_amd.linear.solvers.iterative_ridge  # noqa: F401  (the module; absent before this solver)
    from lasso_amd.linear.solvers import iterative_ridge
    import lasso_amd.linear  # noqa: F401
    direct = sys.modules["lasso_amd.linear.solvers.iterative_ridge"].iterative_ridge
    assert iterative_ridge is direct
    sig = inspect.signature(iterative_ridge)
    assert list(sig.parameters) == ["z0", "x", "weight", "alpha", "tol", "tikhonov", "eps", "maxiter", "line_search", "cg",
                                    "cg_options", "verbose", "return_info"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["alpha"], d["tol"], d["tikhonov"], d["eps"], d["maxiter"], d["line_search"], d["cg"], d["cg_options"],
            d["verbose"], d["return_info"]) == (1.0, 1e-5, 1e-4, None, 10, True, False, None, False, False)
    # not an algorithm= arm: sparse_encode's table is as it was, and 'iter-ridge' still raises
    se = sys.modules["lasso_amd.linear.sparse_encode"]
    assert set(se._OFF_PATH_ALGOS) == {"iter-ridge", "interior-point", "split-bregman", "own"}
    doc = iterative_ridge.__doc__
    for word in ("Deviations", "un-rounded", "LinAlgError", "LU", "tikhonov=0", "maxiter", "cg=True", "Out of scope"):
        assert word in doc, word


def test_symbols_declared_and_exported():
    from lasso_amd import _native
    text = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()
    for name in ("lasso_iter_ridge_workspace_bytes", "lasso_iter_ridge_solve", "lasso_iter_ridge_rows",
                 "lasso_iter_ridge_options", "lasso_iter_ridge_trace", "lasso_iter_ridge_result",
                 "LASSO_ITER_RIDGE_CONVERGED", "LASSO_ITER_RIDGE_NAN", "LASSO_ITER_RIDGE_MAXITER"):
        assert name in text, name
    assert "#define LASSO_HIP_ABI_VERSION 7" in text          # additive: the version stays
    raw = ctypes.CDLL(_native.lib_path())
    for name in ("lasso_iter_ridge_workspace_bytes", "lasso_iter_ridge_solve", "lasso_iter_ridge_rows"):
        assert hasattr(raw, name), name
    L = _native.lib()
    assert L.lasso_hip_abi_version() == 7


def test_workspace_is_monotone_and_linear_in_n():
    from lasso_amd import _native
    L = _native.lib()
    ws = lambda n, d, k, dt=_native.LASSO_F32: L.lasso_iter_ridge_workspace_bytes(n, d, k, dt)  # noqa: E731
    sizes = [ws(n, 64, 256) for n in (0, 1, 64, 256, 4096, 65536)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert ws(64, 32, 128) >= (64 * 128 * 3 + 128 * 128 + 2 * 64 * 32) * 4      # rhs, z, z_sol; G; r, q
    assert ws(64, 32, 1025) == 0
    for dtype in (_native.LASSO_BF16, _native.LASSO_F64):
        assert ws(64, 32, 128, dtype) == 0
    # k = 256 is the LDS tier: no per-row matrix at all, so the workspace is three [n,k] and two [n,d] arrays plus
    # O(k^2 + k d) -- 16 times the rows is at most 16 times the bytes, and far below the reference's n k^2 floats
    assert ws(4096, 64, 256) < 10 * ws(256, 64, 256) * 16 // 10
    assert ws(4096, 64, 256) < 4096 * 256 * 256 * 4 // 50
    # the general tier's scratch is a fixed budget: at most 256 triangles and 256 MiB, whatever n is
    per_row = (3 * 1024 + 2 * 256) * 4 + 64
    assert ws(65536, 256, 1024) - ws(1024, 256, 1024) <= (65536 - 1024) * per_row
    assert ws(1024, 256, 1024) <= (256 << 20) + 1024 * per_row + (1024 * 1024 + 1024 * 256) * 4 + (1 << 20)
    assert ws(65536, 256, 1024) < 65536 * 1024 * 1024 * 4 // 100


def test_struct_sizes_match_the_header(tmp_path):
    from lasso_amd import _native as nat
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lasso_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(lasso_iter_ridge_options), sizeof(lasso_iter_ridge_trace), sizeof(lasso_iter_ridge_result), '
                   '__builtin_offsetof(lasso_iter_ridge_options, reserved), __builtin_offsetof(lasso_iter_ridge_result, trace), '
                   '__builtin_offsetof(lasso_iter_ridge_result, bad_row), __builtin_offsetof(lasso_iter_ridge_trace, eval_count)); '
                   'return 0; }\n')
    exe = str(tmp_path / "sizes")
    build = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [ctypes.sizeof(nat.IterRidgeOptions), ctypes.sizeof(nat.IterRidgeTrace), ctypes.sizeof(nat.IterRidgeResult),
                   nat.IterRidgeOptions.reserved.offset, nat.IterRidgeResult.trace.offset, nat.IterRidgeResult.bad_row.offset,
                   nat.IterRidgeTrace.eval_count.offset]


def _solve_status(L, nat, n=4, d=3, k=5, dtype=None, ldx=None, ldw=None, ldz0=None, ldz=None, x=1, w=1, z0=1, z=1, ws=1,
                  alpha=0.1, opts=1, result=1, **fields):
    """lasso_iter_ridge_solve with fake (never dereferenced) pointers: every refusal comes before the first HIP call"""
    p = lambda on: ctypes.c_void_p(0x1000 if on else 0)                                  # noqa: E731
    o = nat.IterRidgeOptions(fields.get("maxiter", 3), fields.get("line_search", 1), fields.get("tol", 1e-5),
                             fields.get("tikhonov", 1e-4), fields.get("eps", 1e-7), fields.get("reserved", 0))
    r = nat.IterRidgeResult()
    return L.lasso_iter_ridge_solve(p(x), d if ldx is None else ldx, p(w), k if ldw is None else ldw, p(z0),
                                    k if ldz0 is None else ldz0, p(z), k if ldz is None else ldz, n, d, k,
                                    nat.LASSO_F32 if dtype is None else dtype, alpha, ctypes.byref(o) if opts else None,
                                    ctypes.byref(r) if result else None, p(ws), 0, None)


def _rows_status(L, nat, n=4, k=5, dtype=None, ld=None, g=1, rhs=1, z=1, zs=1, ws=1, alpha=0.1, tikhonov=1e-4, eps=1e-7, out=1):
    p = lambda on: ctypes.c_void_p(0x1000 if on else 0)                                  # noqa: E731
    row, minor = ctypes.c_int64(7), ctypes.c_int32(7)
    ld = k if ld is None else ld
    return L.lasso_iter_ridge_rows(p(g), ld, p(rhs), ld, p(z), ld, p(zs), ld, n, k, nat.LASSO_F32 if dtype is None else dtype,
                                   alpha, tikhonov, eps, ctypes.byref(row) if out else None, ctypes.byref(minor), None, p(ws), 0,
                                   None)


def test_c_abi_refusals_need_no_device():
    from lasso_amd import _native as nat
    L = nat.lib()
    bad, unsup = nat.LASSO_ERR_BAD_ARG, nat.LASSO_ERR_UNSUPPORTED
    assert _solve_status(L, nat, dtype=nat.LASSO_F64) == unsup
    assert _solve_status(L, nat, dtype=nat.LASSO_BF16) == unsup
    assert _solve_status(L, nat, k=1025) == unsup
    for kw in (dict(x=0), dict(w=0), dict(z0=0), dict(z=0), dict(ws=0), dict(ldx=2), dict(ldw=4), dict(ldz0=4), dict(ldz=4),
               dict(n=-1), dict(d=0), dict(k=0), dict(alpha=-1.0), dict(alpha=float("nan")), dict(line_search=2),
               dict(line_search=-1), dict(maxiter=-1), dict(tol=-1.0), dict(tikhonov=-1e-4), dict(eps=float("nan")),
               dict(reserved=1), dict(reserved=1 << 40), dict(opts=0), dict(result=0)):
        assert _solve_status(L, nat, **kw) == bad, kw
    assert _solve_status(L, nat, n=0, x=0, z0=0, z=0, ws=0) == nat.LASSO_OK           # nothing to do, nothing written
    # a well-formed call gets as far as the workspace check (0 bytes given), still without a launch
    for mode in (0, 1):
        assert _solve_status(L, nat, line_search=mode) == nat.LASSO_ERR_WORKSPACE
    assert _solve_status(L, nat, k=1024, tikhonov=0.0) == nat.LASSO_ERR_WORKSPACE
    # the row kernel's entry point
    assert _rows_status(L, nat, dtype=nat.LASSO_F64) == unsup and _rows_status(L, nat, k=1025) == unsup
    for kw in (dict(g=0), dict(rhs=0), dict(z=0), dict(zs=0), dict(ws=0), dict(ld=4), dict(n=-1), dict(k=0), dict(alpha=-1.0),
               dict(tikhonov=-1.0), dict(eps=-1.0), dict(out=0)):
        assert _rows_status(L, nat, **kw) == bad, kw
    assert _rows_status(L, nat, n=0, g=0, rhs=0, z=0, zs=0, ws=0) == nat.LASSO_OK
    assert _rows_status(L, nat) == nat.LASSO_ERR_WORKSPACE


def test_refusals_come_before_any_native_call(monkeypatch):
    from lasso_amd import _native
    from lasso_amd.linear.solvers import iterative_ridge

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_native, "lib", boom)
    monkeypatch.setattr(_native, "require_gpu", boom)
    w, x, z0 = torch.randn(16, 40), torch.randn(24, 16), torch.zeros(24, 40)
    with pytest.raises(NotImplementedError, match="cg"):
        iterative_ridge(z0, x, w, cg=True)
    with pytest.raises(NotImplementedError, match="cg"):
        iterative_ridge(z0, x, w, cg=True, cg_options=dict(rtol=0.1))
    with pytest.raises(AssertionError) as e:
        iterative_ridge(z0[0], x, w)                                     # assert z0.dim() == 2
    assert "native call" not in str(e.value)
    with pytest.raises(AssertionError) as e:
        iterative_ridge(torch.zeros(24, 39), x, w)
    assert "native call" not in str(e.value)
    for t in ((z0.double(), x.double(), w.double()), (z0.double(), x, w)):
        with pytest.raises(NotImplementedError, match="float64"):
            iterative_ridge(*t)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        iterative_ridge(z0.bfloat16(), x.bfloat16(), w.bfloat16())
    with pytest.raises(NotImplementedError, match="1024"):
        iterative_ridge(torch.zeros(2, 1025), torch.randn(2, 3), torch.randn(3, 1025))
    # and a well-formed call reaches the native layer; cg_options without cg is ignored
    with pytest.raises(AssertionError, match="native call"):
        iterative_ridge(z0, x, w.requires_grad_(), cg_options=dict(rtol=0.1))


def test_no_gpu_is_a_native_error_not_a_cpu_result():
    from lasso_amd import _native
    from lasso_amd.linear.solvers import iterative_ridge
    if torch.cuda.is_available():        # a GPU is visible: tests/test_iter_ridge_gpu.py covers the solve
        return
    with pytest.raises(_native.NativeError):
        iterative_ridge(torch.zeros(4, 5), torch.randn(4, 3), torch.randn(3, 5), maxiter=2)


def test_every_stored_case_satisfies_its_caps(cases):
    assert {key.split("/")[0] for key in cases.files} == set(CASES)
    for name, spec in CASES.items():
        g = load_case(cases, name)
        n, k = spec["n"], spec["k"]
        assert g["z32"].shape == (n, k) and g["z32"].dtype == np.float32
        assert g["z64"].shape == (n, k) and g["z64"].dtype == np.float64
        its = len(g["f32"])
        assert 1 <= its <= spec["kwargs"]["maxiter"] and len(g["t32"]) == len(g["update32"]) == len(g["smax32"]) == its
        if spec["compare"] == "z":
            assert float(g["spread_z"]) <= SPREAD_Z_CAP, name
        if spec["compare"] == "f":
            assert float(g["spread_f"]) <= SPREAD_F_CAP, name
        tol = float(g["tol"])
        assert tol == n * k * spec["kwargs"].get("tol", 1e-5)
        for key in ("update32", "update64"):                                 # no stop decision within 1 % of tol
            assert (np.abs(g[key] - tol) >= 0.01 * tol).all(), name
        assert float(g["model_gap64"]) <= 1e-7 or spec["compare"] == "f"
        if spec["compare"] == "z":
            assert float(g["model_gap32"]) <= 64 * np.finfo(np.float32).eps * max(1.0, float(np.abs(g["z32"]).max()))
    # the cases that are there for a path took it
    assert len(cases["tolstop/f32"]) < CASES["tolstop"]["kwargs"]["maxiter"] and cases["tolstop/update32"][-1] <= cases["tolstop/tol"]
    assert len(cases["tolstop2/f32"]) == 9
    assert int(cases["k300/smax32"][-1]) <= 256 and CASES["k300"]["k"] > 256      # general tier first, LDS tier later
    assert int((np.abs(case_inputs(CASES["warm"])[2].numpy()) == 0).sum()) > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_reproduces_fixture(cases, name):
    """The compacted model sums in another order than the reference's masked full-size solve, so it is "another correct
    float32 implementation" on every CPU: codes are held to the GPU tests' bar, max(5e-5, 4 x spread_z), with equal
    iteration counts, the objective-only cases to max(1e-6, 4 x spread_f); float64 codes to 1e-6."""
    spec, g = CASES[name], load_case(cases, name)
    if spec["kwargs"].get("line_search", True):
        pytest.importorskip("scipy")
    x, w, z0 = case_inputs(spec)
    keep = x.clone(), w.clone(), z0.clone()
    z, info = iter_ridge_model.iterative_ridge(z0, x, w, alpha=spec["alpha"], **spec["kwargs"])
    z64, info64 = iter_ridge_model.iterative_ridge(z0, x, w, alpha=spec["alpha"], dtype=torch.float64, **spec["kwargs"])
    assert torch.equal(x, keep[0]) and torch.equal(w, keep[1]) and torch.equal(z0, keep[2])
    assert torch.isfinite(z).all() and info["iterations"] == len(g["f32"]) and info64["iterations"] == len(g["f64"])
    assert info["bad"] is None
    if spec["compare"] == "z":
        dz = float((z - torch.from_numpy(g["z32"])).abs().max())
        assert dz <= max(5e-5, 4.0 * float(g["spread_z"])), (name, dz)
        assert float((z64 - torch.from_numpy(g["z64"])).abs().max()) <= 1e-6
        assert info["status"] == ("converged" if spec.get("stops") else "maxiter")
    else:
        # (in the reference's order the model rounds each trial's objective to float32, and that noise moves Brent as it
        # moves the reference's own float32 run; spread_f was measured on the model that folds the objective in double)
        _, seeded = iter_ridge_model.iterative_ridge(z0, x, w, alpha=spec["alpha"], order_seed=1, **spec["kwargs"])
        f_rel = abs(seeded["fval"][-1] - float(g["f32"][-1])) / float(g["f32"][-1])
        assert f_rel <= max(1e-6, 4.0 * float(g["spread_f"])), (name, f_rel)
    assert abs(info64["fval"][-1] - float(g["f64"][-1])) <= 1e-6 * float(g["f64"][-1])
