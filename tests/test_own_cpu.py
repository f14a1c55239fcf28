"""orthant_wise_newton without a GPU: the Python surface equals the reference's, the C boundary declares and exports
the new symbols and its structs have the size of their ctypes mirrors, refusals come before any native call, the host
model (tests/own_model.py) reproduces the fixture recorded from the reference (bit for bit on the kind of CPU it was
recorded on, within the stored spread elsewhere), and every stored case satisfies the caps it was admitted under."""
import ctypes
import inspect
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import own_model
from own_cases import CASES, SPREAD_F_CAP, SPREAD_Z_CAP, admitted_f, case_inputs, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    return golden("own_cases")


def test_python_surface():
    import lasso_amd.linear.solvers.orthant_wise_newton  # noqa: F401  (the module; absent before this solver)
    from lasso_amd.linear.solvers import orthant_wise_newton
    import lasso_amd.linear  # noqa: F401
    direct = sys.modules["lasso_amd.linear.solvers.orthant_wise_newton"].orthant_wise_newton
    assert orthant_wise_newton is direct
    sig = inspect.signature(orthant_wise_newton)
    assert list(sig.parameters) == ["weight", "x", "z0", "alpha", "lr", "maxiter", "xtol", "line_search", "ls_options",
                                    "verbose", "return_info"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["alpha"], d["lr"], d["maxiter"], d["xtol"], d["line_search"], d["ls_options"], d["verbose"],
            d["return_info"]) == (1., 1., 20, 1e-5, "brent", None, 0, False)
    # not an algorithm= arm: sparse_encode's table is as it was
    se = sys.modules["lasso_amd.linear.sparse_encode"]
    assert set(se._OFF_PATH_ALGOS) == {"iter-ridge", "interior-point", "split-bregman", "own"}
    doc = orthant_wise_newton.__doc__
    assert "Deviations" in doc and "double" in doc and "k > d" in doc and "1e-4" in doc


def test_symbols_declared_and_exported():
    from lasso_amd import _native
    text = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()
    for name in ("lasso_own_workspace_bytes", "lasso_own_solve", "lasso_own_options", "lasso_own_result",
                 "LASSO_OWN_LS_NOT_CONVERGED", "LASSO_OWN_NONFINITE"):
        assert name in text, name
    assert "#define LASSO_HIP_ABI_VERSION 7" in text          # additive: the version stays
    raw = ctypes.CDLL(_native.lib_path())
    assert hasattr(raw, "lasso_own_workspace_bytes") and hasattr(raw, "lasso_own_solve")
    L = _native.lib()
    assert L.lasso_hip_abi_version() == 7
    small = L.lasso_own_workspace_bytes(64, 32, 128, _native.LASSO_F32)
    assert small >= (64 * 128 * 11 + 128 * 128 + 64 * 32) * 4    # z, v, d, eight candidates; Hinv; resid
    assert L.lasso_own_workspace_bytes(4096, 256, 1024, _native.LASSO_F32) > small
    assert L.lasso_own_workspace_bytes(0, 32, 128, _native.LASSO_F32) > 0
    assert L.lasso_own_workspace_bytes(64, 32, 4097, _native.LASSO_F32) == 0
    for dtype in (_native.LASSO_BF16, _native.LASSO_F64):
        assert L.lasso_own_workspace_bytes(64, 32, 128, dtype) == 0


def test_struct_sizes_match_the_header(tmp_path):
    from lasso_amd import _native as nat
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lasso_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(lasso_own_options), sizeof(lasso_own_trace), sizeof(lasso_own_result), '
                   '__builtin_offsetof(lasso_own_result, trace), __builtin_offsetof(lasso_own_trace, eval_count)); '
                   'return 0; }\n')
    exe = str(tmp_path / "sizes")
    build = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [ctypes.sizeof(nat.OwnOptions), ctypes.sizeof(nat.OwnTrace), ctypes.sizeof(nat.OwnResult),
                   nat.OwnResult.trace.offset, nat.OwnTrace.eval_count.offset]


def _solve_status(L, nat, n=4, d=3, k=5, dtype=None, ldx=None, ldw=None, ldz0=None, ldz=None, x=1, w=1, z0=1, z=1, ws=1,
                  alpha=0.1, opts=1, result=1, **fields):
    """lasso_own_solve with fake (never dereferenced) pointers: every refusal comes before the first HIP call"""
    p = lambda on: ctypes.c_void_p(0x1000 if on else 0)                                  # noqa: E731
    o = nat.OwnOptions(fields.get("maxiter", 3), fields.get("line_search", 0), fields.get("ls_maxiter", 500), 0, 1.0, 1e-5,
                       0.1, 0.95)
    r = nat.OwnResult()
    return L.lasso_own_solve(p(x), d if ldx is None else ldx, p(w), k if ldw is None else ldw, p(z0),
                             k if ldz0 is None else ldz0, p(z), k if ldz is None else ldz, n, d, k,
                             nat.LASSO_F32 if dtype is None else dtype, alpha, ctypes.byref(o) if opts else None,
                             ctypes.byref(r) if result else None, p(ws), 0, None)


def test_c_abi_refusals_need_no_device():
    from lasso_amd import _native as nat
    L = nat.lib()
    bad, unsup = nat.LASSO_ERR_BAD_ARG, nat.LASSO_ERR_UNSUPPORTED
    assert _solve_status(L, nat, dtype=nat.LASSO_F64) == unsup
    assert _solve_status(L, nat, dtype=nat.LASSO_BF16) == unsup
    assert _solve_status(L, nat, k=4097) == unsup
    for kw in (dict(x=0), dict(w=0), dict(z0=0), dict(z=0), dict(ws=0), dict(ldx=2), dict(ldw=4), dict(ldz0=4), dict(ldz=4),
               dict(n=-1), dict(d=0), dict(k=0), dict(alpha=-1.0), dict(alpha=float("nan")), dict(line_search=3),
               dict(line_search=-1), dict(maxiter=-1), dict(line_search=1, ls_maxiter=0), dict(opts=0), dict(result=0)):
        assert _solve_status(L, nat, **kw) == bad, kw
    assert _solve_status(L, nat, n=0, x=0, z0=0, z=0, ws=0) == nat.LASSO_OK           # nothing to do, nothing written
    # a well-formed call gets as far as the workspace check (0 bytes given), still without a launch
    for mode in (0, 1, 2):
        assert _solve_status(L, nat, line_search=mode) == nat.LASSO_ERR_WORKSPACE


def test_refusals_come_before_any_native_call(monkeypatch):
    from lasso_amd import _native
    from lasso_amd.linear.solvers import orthant_wise_newton

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_native, "lib", boom)
    monkeypatch.setattr(_native, "require_gpu", boom)
    w, x, z0 = torch.randn(16, 40), torch.randn(24, 16), torch.zeros(24, 40)
    with pytest.raises(ValueError, match="line_search must be one of {'brent', 'backtrack', 'none'}."):
        orthant_wise_newton(w, x, z0, line_search="armijo")
    with pytest.raises(TypeError, match="shrink"):
        orthant_wise_newton(w, x, z0, line_search="backtrack", ls_options=dict(shrink=0.5))
    with pytest.raises(AssertionError) as e:
        orthant_wise_newton(w, x, z0[0])                                 # assert z0.dim() == 2
    assert "native call" not in str(e.value)
    with pytest.raises(AssertionError) as e:
        orthant_wise_newton(w, x, torch.zeros(24, 39))
    assert "native call" not in str(e.value)
    for t in ((w.double(), x.double(), z0.double()), (w, x, z0.double())):
        with pytest.raises(NotImplementedError, match="float64"):
            orthant_wise_newton(*t)
    with pytest.raises(NotImplementedError, match="4096"):
        orthant_wise_newton(torch.randn(3, 4097), torch.randn(2, 3), torch.zeros(2, 4097))
    # and a well-formed call reaches the native layer
    with pytest.raises(AssertionError, match="native call"):
        orthant_wise_newton(w, x, z0.requires_grad_())


def test_no_gpu_is_a_native_error_not_a_cpu_result():
    from lasso_amd import _native
    from lasso_amd.linear.solvers import orthant_wise_newton
    if torch.cuda.is_available():        # a GPU is visible: tests/test_own_gpu.py covers the solve
        return
    with pytest.raises(_native.NativeError):
        orthant_wise_newton(torch.randn(3, 5), torch.randn(4, 3), torch.zeros(4, 5), maxiter=2)


def test_every_stored_case_satisfies_its_caps(cases):
    assert {key.split("/")[0] for key in cases.files} == set(CASES)
    for name, spec in CASES.items():
        g = load_case(cases, name)
        n, k = spec["n"], spec["k"]
        assert g["z32"].shape == (n, k) and g["z32"].dtype == np.float32
        assert g["z64"].shape == (n, k) and g["z64"].dtype == np.float64
        its = len(g["f32"])
        assert 1 <= its <= spec["kwargs"]["maxiter"] and len(g["t32"]) == len(g["ls32"]) == len(g["dz32"]) == its
        if spec["compare"] == "z":
            assert float(g["spread_z"]) <= SPREAD_Z_CAP, name                # (c)
        if spec["compare"] == "f":
            assert float(g["spread_f"]) <= SPREAD_F_CAP, name                # (d)
        for fn, bound, f in g["decisions32"]:                                # (a)
            assert abs(fn - bound) >= 1e-4 * abs(f), name
        xtol = spec["kwargs"].get("xtol", 1e-5)
        assert (np.abs(g["dz32"] - xtol) >= 0.01 * xtol).all(), name
    # the cases that are there for a path took it
    assert len(cases["bt_xtol/f32"]) < CASES["bt_xtol"]["kwargs"]["maxiter"]
    assert str(cases["bt_runout/warnings"]).count("line search did not converge.") == 3
    assert admitted_f(load_case(cases, "wide_brent")) and not admitted_f(load_case(cases, "wide_bt"))


@pytest.fixture(scope="module")
def recorded_on_this_kind_of_cpu():
    """True where this CPU rounds float32 products as the CPU the fixture was recorded on (the probe of
    tests/golden_runs.py: the first FISTA iterate of config 2 against the primary recording)."""
    import golden_runs
    from oracle import lasso_oracle as orc
    from recipes import LAMBDA_MAX_C2, recipe_xw
    X, W = recipe_xw(4096)
    z = orc.fista(X, X.new_zeros(4096, 1024), W, 0.5, lr=1.0 / LAMBDA_MAX_C2, maxiter=1, tol=0.0)[:64, :64].numpy()
    return golden_runs.same(z, golden_runs.load("g2_c2_fista", None)["z_block_M1"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_reproduces_fixture(cases, name, recorded_on_this_kind_of_cpu):
    """On the kind of CPU the fixture was recorded on the float32 model IS the reference: bit for bit, and within 1e-6
    in float64.  Another CPU's BLAS sums in another order -- it is "another correct float32 implementation", which is
    what spread_z / spread_f measured when the fixture was made: there the codes are held to the GPU tests' bar,
    max(5e-5, 4 x spread_z), with equal trial counts, and the objective-only cases to max(1e-6, 4 x spread_f)."""
    spec, g = CASES[name], load_case(cases, name)
    brent = spec["kwargs"]["line_search"] == "brent"
    if brent:
        pytest.importorskip("scipy")
    x, w, z0 = case_inputs(spec)
    keep = x.clone(), w.clone(), z0.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z, info = own_model.orthant_wise_newton(w, x, z0, alpha=spec["alpha"], **spec["kwargs"])
        z64, info64 = own_model.orthant_wise_newton(w, x, z0, alpha=spec["alpha"], dtype=torch.float64, **spec["kwargs"])
    assert torch.equal(x, keep[0]) and torch.equal(w, keep[1]) and torch.equal(z0, keep[2])
    assert len(info["warnings"]) == len([m for m in str(g["warnings"]).split("\n") if m])
    dz = float((z - torch.from_numpy(g["z32"])).abs().max())
    dz64 = float((z64 - torch.from_numpy(g["z64"])).abs().max())
    if recorded_on_this_kind_of_cpu:
        assert torch.equal(z, torch.from_numpy(g["z32"])), dz
        assert info["ls_iters"] == list(g["ls32"]) and info["t"] == list(g["t32"])
        assert dz64 <= 1e-6
        assert info64["ls_iters"] == list(g["ls64"])
        return
    f_rel = abs(info["objective"][-1] - float(g["f32"][-1])) / float(g["f32"][-1])
    f64_rel = abs(info64["objective"][-1] - float(g["f64"][-1])) / float(g["f64"][-1])
    if spec["compare"] == "z":
        assert dz <= max(5e-5, 4.0 * float(g["spread_z"])), (name, dz)
        if not brent:
            assert info["ls_iters"] == list(g["ls32"]) and info64["ls_iters"] == list(g["ls64"])
            assert dz64 <= 1e-6, (name, dz64)
    elif admitted_f(g):
        assert f_rel <= max(1e-6, 4.0 * float(g["spread_f"])), (name, f_rel)
    assert f64_rel <= 1e-6 or not admitted_f(g), (name, f64_rel)
    assert torch.isfinite(z).all() and info["iterations"] == len(g["f32"])
