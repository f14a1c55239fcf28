"""iterative_ridge_bfgs without a GPU: the Python surface equals the reference's, the C boundary declares and exports the
new symbols and its structs have the size of their ctypes mirrors, refusals come before any native call, the workspace
holds its two n k^2 regions, the host model (tests/irbfgs_model.py) reproduces the fixture recorded from the reference
(bit for bit on the kind of CPU it was recorded on, within the stored spread elsewhere), and every stored case satisfies
the caps it was admitted under."""
import ctypes
import inspect
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import irbfgs_model
from irbfgs_cases import (CASES, NONFINITE, SPREAD_F_CAP, SPREAD_Z_CAP, admitted_f, case_inputs, classes, load_case,
                          poisoned_inputs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    return golden("irbfgs_cases")


def test_python_surface():
    from lasso_amd.nonlinear import iterative_ridge_bfgs, owlqn, rss
    module = sys.modules["lasso_amd.nonlinear.iterative_ridge_bfgs"]   # (the function shadows its module, as in the reference)
    assert module.iterative_ridge_bfgs is iterative_ridge_bfgs and module.rss is rss
    assert sys.modules["lasso_amd.nonlinear.owlqn"].owlqn is owlqn
    sig = inspect.signature(iterative_ridge_bfgs)
    # the reference's names, order and defaults (lasso/nonlinear/iterative_ridge_bfgs.py:46-48), plus return_info
    assert list(sig.parameters) == ["f", "x0", "alpha", "lr", "xtol", "tikhonov", "eps", "line_search", "maxiter", "verbose",
                                    "return_info"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["alpha"], d["lr"], d["xtol"], d["tikhonov"], d["eps"], d["line_search"], d["maxiter"], d["verbose"],
            d["return_info"]) == (1.0, 1.0, 1e-5, 1e-4, None, True, None, 0, False)
    doc = iterative_ridge_bfgs.__doc__
    assert "Deviations" in doc and "double" in doc and "symmetric" in doc and "[n,k,k]" in doc


def test_symbols_declared_and_exported():
    from lasso_amd import _native
    text = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()
    for name in ("lasso_irbfgs_workspace_bytes", "lasso_irbfgs_solve", "lasso_irbfgs_update", "lasso_irbfgs_options",
                 "lasso_irbfgs_result", "lasso_irbfgs_trace", "LASSO_IRBFGS_CONVERGED", "LASSO_IRBFGS_NONFINITE"):
        assert name in text, name
    assert "#define LASSO_HIP_ABI_VERSION 7" in text          # additive: the version stays
    raw = ctypes.CDLL(_native.lib_path())
    for name in ("lasso_irbfgs_workspace_bytes", "lasso_irbfgs_solve", "lasso_irbfgs_update"):
        assert hasattr(raw, name), name
    assert _native.lib().lasso_hip_abi_version() == 7


def test_workspace_sizes():
    from lasso_amd import _native as nat
    L = nat.lib()
    f32 = nat.LASSO_F32
    n, d, k = 64, 32, 128
    size = L.lasso_irbfgs_workspace_bytes(n, d, k, f32)
    # B and the systems; six [n,k] vectors, two [n,d], W^T; the batch solver's own scratch
    floor = (2 * n * k * k + 6 * n * k + 2 * n * d + d * k) * 4 + L.lasso_batch_solve_workspace_bytes(n, k, f32) - 256
    assert floor <= size <= floor + (1 << 20)
    assert L.lasso_irbfgs_workspace_bytes(2 * n, d, k, f32) > 2 * size - (1 << 20)
    assert L.lasso_irbfgs_workspace_bytes(0, d, k, f32) > 0
    cap = L.lasso_batch_solve_tier_cap(f32, 2)
    assert cap == nat.IRBFGS_MAX_K == 1024
    assert L.lasso_irbfgs_workspace_bytes(2, d, cap, f32) > 0
    assert L.lasso_irbfgs_workspace_bytes(2, d, cap + 1, f32) == 0
    for bad in ((-1, d, k), (n, 0, k), (n, d, 0)):
        assert L.lasso_irbfgs_workspace_bytes(*bad, f32) == 0
    for dtype in (nat.LASSO_BF16, nat.LASSO_F64):
        assert L.lasso_irbfgs_workspace_bytes(n, d, k, dtype) == 0


def test_struct_sizes_match_the_header(tmp_path):
    from lasso_amd import _native as nat
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lasso_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(lasso_irbfgs_options), sizeof(lasso_irbfgs_trace), sizeof(lasso_irbfgs_result), '
                   '__builtin_offsetof(lasso_irbfgs_result, trace), __builtin_offsetof(lasso_irbfgs_trace, eval_count), '
                   '__builtin_offsetof(lasso_irbfgs_options, reserved), __builtin_offsetof(lasso_irbfgs_trace, lu), '
                   '__builtin_offsetof(lasso_irbfgs_result, row_bytes)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    build = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [ctypes.sizeof(nat.IrbfgsOptions), ctypes.sizeof(nat.IrbfgsTrace), ctypes.sizeof(nat.IrbfgsResult),
                   nat.IrbfgsResult.trace.offset, nat.IrbfgsTrace.eval_count.offset, nat.IrbfgsOptions.reserved.offset,
                   nat.IrbfgsTrace.lu.offset, nat.IrbfgsResult.row_bytes.offset]


def _solve_status(L, nat, n=4, d=3, k=5, dtype=None, ldx=None, ldw=None, ldz0=None, ldz=None, x=1, w=1, z0=1, z=1, ws=1,
                  alpha=0.1, opts=1, result=1, **fields):
    """lasso_irbfgs_solve with fake (never dereferenced) pointers: every refusal comes before the first HIP call"""
    p = lambda on: ctypes.c_void_p(0x1000 if on else 0)                                  # noqa: E731
    o = nat.IrbfgsOptions(fields.get("maxiter", 3), fields.get("line_search", 1), fields.get("lr", 1.0),
                          fields.get("xtol", 1e-5), fields.get("tikhonov", 1e-4), fields.get("eps", 1e-7),
                          fields.get("reserved", 0))
    r = nat.IrbfgsResult()
    return L.lasso_irbfgs_solve(p(x), d if ldx is None else ldx, p(w), k if ldw is None else ldw, p(z0),
                                k if ldz0 is None else ldz0, p(z), k if ldz is None else ldz, n, d, k,
                                nat.LASSO_F32 if dtype is None else dtype, alpha, ctypes.byref(o) if opts else None,
                                ctypes.byref(r) if result else None, p(ws), 0, None)


def _update_status(L, nat, n=4, k=5, dtype=None, alpha=0.1, tikhonov=1e-4, eps=1e-7, mode=1, wgs=0, null=None):
    p = [ctypes.c_void_p(0x1000)] * 8
    if null is not None:
        p = list(p)
        p[null] = ctypes.c_void_p(0)
    return L.lasso_irbfgs_update(*p, n, k, nat.LASSO_F32 if dtype is None else dtype, alpha, tikhonov, eps, mode, 0, wgs, None)


def test_c_abi_refusals_need_no_device():
    from lasso_amd import _native as nat
    L = nat.lib()
    bad, unsup = nat.LASSO_ERR_BAD_ARG, nat.LASSO_ERR_UNSUPPORTED
    assert _solve_status(L, nat, dtype=nat.LASSO_F64) == unsup
    assert _solve_status(L, nat, dtype=nat.LASSO_BF16) == unsup
    assert _solve_status(L, nat, k=1025) == unsup
    for kw in (dict(x=0), dict(w=0), dict(z0=0), dict(z=0), dict(ws=0), dict(ldx=2), dict(ldw=4), dict(ldz0=4), dict(ldz=4),
               dict(n=-1), dict(d=0), dict(k=0), dict(alpha=-1.0), dict(alpha=float("nan")), dict(line_search=2),
               dict(line_search=-1), dict(maxiter=-1), dict(lr=-1.0), dict(xtol=-1.0), dict(tikhonov=-1.0), dict(eps=-1.0),
               dict(eps=float("nan")), dict(reserved=1), dict(reserved=4), dict(opts=0), dict(result=0)):
        assert _solve_status(L, nat, **kw) == bad, kw
    assert _solve_status(L, nat, n=0, x=0, z0=0, z=0, ws=0) == nat.LASSO_OK           # nothing to do, nothing written
    # a well-formed call gets as far as the workspace check (0 bytes given), still without a launch
    for mode in (0, 1):
        assert _solve_status(L, nat, line_search=mode) == nat.LASSO_ERR_WORKSPACE
    assert _solve_status(L, nat, k=1024, reserved=2) == nat.LASSO_ERR_WORKSPACE
    # the row kernel's entry
    assert _update_status(L, nat, dtype=nat.LASSO_F64) == unsup and _update_status(L, nat, k=1025) == unsup
    for kw in (dict(n=-1), dict(k=0), dict(alpha=-1.0), dict(tikhonov=-1.0), dict(eps=float("nan")), dict(mode=3), dict(mode=-1),
               dict(wgs=-1)) + tuple(dict(null=i) for i in range(8)):
        assert _update_status(L, nat, **kw) == bad, kw
    assert _update_status(L, nat, n=0, null=0) == nat.LASSO_OK


def test_refusals_come_before_any_native_call(monkeypatch):
    from lasso_amd import _native
    from lasso_amd.nonlinear import iterative_ridge_bfgs, rss

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_native, "lib", boom)
    monkeypatch.setattr(_native, "require_gpu", boom)
    w, x, z0 = torch.randn(16, 40), torch.randn(24, 16), torch.ones(24, 40)
    fun = rss(x, w)
    with pytest.raises(NotImplementedError, match=r"only rss\(x, weight\) objectives run on the HIP path"):
        iterative_ridge_bfgs(lambda z: 0.5 * (z @ w.T - x).pow(2).sum(), z0)
    with pytest.raises(NotImplementedError, match=r"only rss\(x, weight\) objectives"):
        iterative_ridge_bfgs((x, w), z0)
    with pytest.raises(AssertionError) as e:
        iterative_ridge_bfgs(fun, z0[0])                                 # assert x0.dim() == 2
    assert "native call" not in str(e.value)
    with pytest.raises(AssertionError) as e:
        iterative_ridge_bfgs(fun, torch.zeros(24, 39))
    assert "native call" not in str(e.value)
    with pytest.raises(RuntimeError, match="2-D tensors"):
        iterative_ridge_bfgs(rss(x[0], w), z0)
    for f, z in ((rss(x.double(), w.double()), z0.double()), (fun, z0.double()), (rss(x, w.double()), z0)):
        with pytest.raises(NotImplementedError, match="float64"):
            iterative_ridge_bfgs(f, z)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        iterative_ridge_bfgs(rss(x.bfloat16(), w.bfloat16()), z0.bfloat16())
    with pytest.raises(NotImplementedError, match="1024"):
        iterative_ridge_bfgs(rss(torch.randn(2, 3), torch.randn(3, 1025)), torch.zeros(2, 1025))
    for kw in (dict(maxiter=-1), dict(alpha=-1.0), dict(tikhonov=-1.0), dict(eps=-1.0), dict(xtol=-1.0), dict(lr=-1.0)):
        with pytest.raises(ValueError):
            iterative_ridge_bfgs(fun, z0, **kw)
    # no rows and no iterations need no device: a copy of x0, silently
    out, info = iterative_ridge_bfgs(fun, z0, maxiter=0, verbose=2, return_info=True)
    assert torch.equal(out, z0) and out.data_ptr() != z0.data_ptr() and info["iterations"] == 0
    assert iterative_ridge_bfgs(rss(x[:0], w), z0[:0]).shape == (0, 40)
    # and a well-formed call reaches the native layer -- k at the cap included
    with pytest.raises(AssertionError, match="native call"):
        iterative_ridge_bfgs(rss(x, w.requires_grad_()), z0)
    with pytest.raises(AssertionError, match="native call"):
        iterative_ridge_bfgs(rss(torch.randn(2, 3), torch.randn(3, 1024)), torch.zeros(2, 1024))


def test_no_gpu_is_a_native_error_not_a_cpu_result():
    from lasso_amd import _native
    from lasso_amd.nonlinear import iterative_ridge_bfgs, rss
    if torch.cuda.is_available():        # a GPU is visible: tests/test_irbfgs_gpu.py covers the solve
        return
    with pytest.raises(_native.NativeError):
        iterative_ridge_bfgs(rss(torch.randn(4, 3), torch.randn(3, 5)), torch.ones(4, 5), maxiter=2)


def test_every_stored_case_satisfies_its_caps(cases):
    assert {key.split("/")[0] for key in cases.files} == set(CASES) | set(NONFINITE)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "irbfgs_cases.npz")) <= \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "owlqn_cases.npz"))
    for name, spec in CASES.items():
        g = load_case(cases, name)
        n, k = spec["n"], spec["k"]
        kw = spec["kwargs"]
        assert g["z32"].shape == (n, k) and g["z32"].dtype == np.float32
        assert g["z64"].shape == (n, k) and g["z64"].dtype == np.float64
        its = len(g["f32"])
        assert its <= kw["maxiter"] and len(g["t32"]) == len(g["ls32"]) == len(g["dx32"]) == len(g["invalid_rows"]) == its
        assert str(g["warnings"]) == ""                                      # no case took the LU route
        # fixed steps and one Brent iteration are compared by their codes
        if not kw["line_search"] or kw["maxiter"] == 1:
            assert spec["compare"] == "z", name
        if spec["compare"] == "z":
            assert float(g["spread_z"]) <= SPREAD_Z_CAP, name                # (c)
        if spec["compare"] == "f":
            assert float(g["spread_f"]) <= SPREAD_F_CAP, name                # (d)
        a = np.abs(g["curv32"])                                              # (a)
        assert ((a >= 10 * irbfgs_model.CURV_MIN) | (a <= irbfgs_model.CURV_MIN / 10)).all(), name
        xtol = kw.get("xtol", 1e-5)
        assert (np.abs(g["dx32"] - xtol) >= 0.01 * xtol).all(), name
        # a frozen zero of the start is an exact zero of the result
        z0 = case_inputs(spec)[2]
        assert (g["z32"][(z0 == 0).numpy()] == 0).all() and (g["z64"][(z0 == 0).numpy()] == 0).all()
    # the cases that are there for a path took it
    assert len(cases["all_zero/f32"]) == 1 and float(cases["all_zero/dx32"][0]) == 0.0
    assert not cases["all_zero/z32"].any()
    assert 1 < len(cases["xtol_early/f32"]) < CASES["xtol_early"]["kwargs"]["maxiter"]
    assert len(cases["iter0/f32"]) == 0 and len(cases["brent1_wave/f32"]) == 1
    assert list(cases["fixed4_lds70/invalid_rows"]) == [1, 1, 1, 1]          # the all-zero row: s = y = 0 at every update
    assert list(cases["dense_start/invalid_rows"]) == [0, 0, 0, 0]
    assert list(cases["xtol_early/invalid_rows"])[-1] == -1                  # no update follows the iteration that stops
    for name, shape in (("wave", 16), ("lds33", 33), ("lds70", 70), ("general", 288)):
        assert CASES["fixed4_" + name]["k"] == shape
    # the non-finite cases: one iteration, the poisoned row NaN except its frozen zeros, the others finite
    for name, entry in NONFINITE.items():
        g = load_case(cases, name)
        _, _, z0 = poisoned_inputs(entry)
        row = entry["poison"][1]
        assert int(g["iterations"]) == 1
        z = torch.from_numpy(g["z32"])
        others = [r for r in range(z.shape[0]) if r != row]
        assert torch.isfinite(z[others]).all() and torch.isnan(z[row][z0[row] != 0]).all()
        assert torch.equal(z[row][z0[row] == 0], z0[row][z0[row] == 0])
    assert "Cholesky factorization failed" in str(cases["nan_z0/warnings"])
    assert str(cases["nan_x/warnings"]) == "" and str(cases["inf_z0/warnings"]) == ""


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
    max(5e-5, 4 x spread_z), and the objective-only cases to max(1e-6, 4 x spread_f)."""
    spec, g = CASES[name], load_case(cases, name)
    if spec["kwargs"]["line_search"]:
        pytest.importorskip("scipy")
    x, w, z0 = case_inputs(spec)
    keep = x.clone(), w.clone(), z0.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z, info = irbfgs_model.iterative_ridge_bfgs(w, x, z0, alpha=spec["alpha"], **spec["kwargs"])
        z64, info64 = irbfgs_model.iterative_ridge_bfgs(w, x, z0, alpha=spec["alpha"], dtype=torch.float64, **spec["kwargs"])
    assert torch.equal(x, keep[0]) and torch.equal(w, keep[1]) and torch.equal(z0, keep[2])
    assert info["warnings"] == [] and info["iterations"] == len(g["f32"]) and torch.isfinite(z).all()
    assert info["invalid_rows"] == list(g["invalid_rows"])
    irbfgs_model.assert_robust(info)
    dz = float((z - torch.from_numpy(g["z32"])).abs().max())
    dz64 = float((z64 - torch.from_numpy(g["z64"])).abs().max())
    if recorded_on_this_kind_of_cpu:
        assert torch.equal(z, torch.from_numpy(g["z32"])), dz
        assert info["t"] == list(g["t32"]) and info["ls_iters"] == list(g["ls32"])
        assert dz64 <= 1e-6
        return
    if info["iterations"] == 0:
        assert torch.equal(z, z0)
        return
    if spec["compare"] == "z":
        assert dz <= max(5e-5, 4.0 * float(g["spread_z"])), (name, dz)
    elif admitted_f(g):
        f_rel = abs(info["objective"][-1] - float(g["f32"][-1])) / float(g["f32"][-1])
        assert f_rel <= max(1e-6, 4.0 * float(g["spread_f"])), (name, f_rel)


@pytest.mark.parametrize("name", sorted(NONFINITE))
def test_model_reproduces_the_class_pattern(cases, name):
    entry, g = NONFINITE[name], load_case(cases, name)
    if entry["case"]["kwargs"]["line_search"]:
        pytest.importorskip("scipy")
    x, w, z0 = poisoned_inputs(entry)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z, info = irbfgs_model.iterative_ridge_bfgs(w, x, z0, alpha=entry["case"]["alpha"], **entry["case"]["kwargs"])
    assert info["iterations"] == 1 and torch.equal(classes(z), classes(g["z32"]))
    assert info["warnings"] == [m for m in str(g["warnings"]).split("\n") if m]


def test_the_seeded_model_keeps_b_symmetric():
    """the symmetric form of the update is bitwise symmetric; the reference's baddbmm form is not"""
    spec = CASES["fixed4_lds33"]
    x, w, z0 = case_inputs(spec)
    m = irbfgs_model.Model(w, x, spec["alpha"])
    _, g0, _ = m.evaluate(z0)
    z1 = z0 - 0.01 * g0 * (z0 != 0)
    _, g1, _ = m.evaluate(z1)
    sym, ref = irbfgs_model.Hessians(z0, g0, True), irbfgs_model.Hessians(z0, g0, False)
    sym.update(z1, g1)
    ref.update(z1, g1)
    assert torch.equal(sym.B, sym.B.transpose(1, 2))
    assert not torch.equal(ref.B, ref.B.transpose(1, 2))
    scale = float(ref.B.abs().max())
    assert float((sym.B - ref.B).abs().max()) <= 1e-5 * scale
