"""interior_point without a GPU: the Python surface equals the reference's plus return_info, the C boundary declares and
exports the new symbols and its structs have the size of their ctypes mirrors, the workspace is linear in n, refusals
come before any native call, the host model (tests/interior_point_model.py) reproduces the fixture recorded from the
reference, and every stored case satisfies the caps it was admitted under."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import interior_point_model
from interior_point_cases import (CASES, RECORDS, SPREAD_F_CAP, SPREAD_Z_CAP, case_inputs, lasso_objective, load_case,
                                  rtol_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    return golden("interior_point_cases")


def test_python_surface():
    import lasso_amd.linear.solvers.interior_point  # noqa: F401  (the module; absent before this solver)
    from lasso_amd.linear.solvers import interior_point
    import lasso_amd.linear  # noqa: F401
    direct = sys.modules["lasso_amd.linear.solvers.interior_point"].interior_point
    assert interior_point is direct
    sig = inspect.signature(interior_point)
    assert list(sig.parameters) == ["x", "weight", "z0", "alpha", "maxiter", "barrier_init", "tol", "eps", "verbose",
                                    "return_info"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["z0"], d["alpha"], d["maxiter"], d["barrier_init"], d["tol"], d["eps"], d["verbose"], d["return_info"]) == \
        (None, 1.0, 20, 0.1, 1e-2, 1e-5, False, False)
    # not an algorithm= arm: sparse_encode's table is as it was, and 'interior-point' still raises
    se = sys.modules["lasso_amd.linear.sparse_encode"]
    assert set(se._OFF_PATH_ALGOS) == {"iter-ridge", "interior-point", "split-bregman", "own"}
    with pytest.raises(NotImplementedError, match="interior-point"):
        se.sparse_encode(torch.randn(4, 3), torch.randn(3, 5), algorithm="interior-point")
    # every solver the reference exports has a name here
    import lasso_amd.linear.solvers as solvers
    for name in ("ista", "coord_descent", "coord_descent_mod", "gpsr_basic", "orthant_wise_newton", "iterative_ridge",
                 "split_bregman", "interior_point"):
        assert callable(getattr(solvers, name)), name


def test_symbols_declared_and_exported():
    from lasso_amd import _native
    text = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()
    for name in ("lasso_interior_point_workspace_bytes", "lasso_interior_point_solve", "lasso_interior_point_rows",
                 "lasso_interior_point_options", "lasso_interior_point_trace", "lasso_interior_point_result",
                 "LASSO_INTERIOR_POINT_CONVERGED", "LASSO_INTERIOR_POINT_MAXITER", "LASSO_INTERIOR_POINT_BAD_START"):
        assert name in text, name
    assert "#define LASSO_HIP_ABI_VERSION 7" in text          # additive: the version stays
    raw = ctypes.CDLL(_native.lib_path())
    for name in ("lasso_interior_point_workspace_bytes", "lasso_interior_point_solve", "lasso_interior_point_rows"):
        assert hasattr(raw, name), name
    L = _native.lib()
    assert L.lasso_hip_abi_version() == 7
    assert L.lasso_interior_point_solve.argtypes is not None and L.lasso_interior_point_rows.argtypes is not None


def test_workspace_is_monotone_and_linear_in_n():
    from lasso_amd import _native
    L = _native.lib()
    ws = lambda n, d, k, dt=_native.LASSO_F32: L.lasso_interior_point_workspace_bytes(n, d, k, dt)  # noqa: E731
    sizes = [ws(n, 64, 256) for n in (0, 1, 64, 256, 4096, 65536)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert ws(64, 32, 128) >= (2 * 64 * 2 * 128 + 64 * 32) * 4                     # z, s [n][2k]; lambda [n][d]
    assert ws(64, 257, 128) == 0 and ws(64, 32, 4097) == 0 and ws(64, 256, 4096) > 0
    for dtype in (_native.LASSO_BF16, _native.LASSO_F64):
        assert ws(64, 32, 128, dtype) == 0
    # linear in n: the same bytes per row whatever n is, nine [n][k] and five [n][d] float arrays plus the row's figures
    for d, k in ((64, 256), (256, 1024), (256, 4096)):
        per_row = (9 * k + 5 * d + 1) * 4 + 64
        step = ws(8192, d, k) - ws(4096, d, k)
        assert step == ws(4096, d, k) - ws(0, d, k)
        assert 4096 * per_row <= step <= 4096 * (per_row + 256)
    # never n d^2, let alone the reference's n 2k d: 8.6 GB at this shape
    assert ws(4096, 256, 1024) < 4096 * 256 * 256 * 4 // 4
    assert ws(4096, 256, 1024) < 4096 * 2048 * 256 * 4 // 40


def test_struct_sizes_match_the_header(tmp_path):
    from lasso_amd import _native as nat
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lasso_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(lasso_interior_point_options), sizeof(lasso_interior_point_trace), '
                   'sizeof(lasso_interior_point_result), __builtin_offsetof(lasso_interior_point_options, reserved), '
                   '__builtin_offsetof(lasso_interior_point_result, trace), '
                   '__builtin_offsetof(lasso_interior_point_trace, gap)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    build = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [ctypes.sizeof(nat.InteriorPointOptions), ctypes.sizeof(nat.InteriorPointTrace),
                   ctypes.sizeof(nat.InteriorPointResult), nat.InteriorPointOptions.reserved.offset,
                   nat.InteriorPointResult.trace.offset, nat.InteriorPointTrace.gap.offset]


def _solve_status(L, nat, n=4, d=3, k=5, dtype=None, ldx=None, ldw=None, ldz0=None, ldz=None, x=1, w=1, z0=1, z=1, ws=1,
                  alpha=0.1, opts=1, result=1, **fields):
    """lasso_interior_point_solve with fake (never dereferenced) pointers: every refusal comes before the first HIP call"""
    p = lambda on: ctypes.c_void_p(0x1000 if on else 0)                                  # noqa: E731
    o = nat.InteriorPointOptions(fields.get("maxiter", 3), 0, fields.get("barrier_init", 0.1), fields.get("tol", 1e-2),
                                 fields.get("eps", 1e-5), fields.get("reserved", 0))
    r = nat.InteriorPointResult()
    return L.lasso_interior_point_solve(p(x), d if ldx is None else ldx, p(w), k if ldw is None else ldw, p(z0),
                                        k if ldz0 is None else ldz0, p(z), k if ldz is None else ldz, n, d, k,
                                        nat.LASSO_F32 if dtype is None else dtype, alpha, ctypes.byref(o) if opts else None,
                                        ctypes.byref(r) if result else None, p(ws), 0, None)


def _rows_status(L, nat, n=4, d=3, k=5, dtype=None, ldw=None, ldc=None, ldb=None, ldy=None, w=1, c=1, b=1, y=1):
    p = lambda on: ctypes.c_void_p(0x1000 if on else 0)                                  # noqa: E731
    return L.lasso_interior_point_rows(p(w), k if ldw is None else ldw, p(c), k if ldc is None else ldc, p(b),
                                       d if ldb is None else ldb, p(y), d if ldy is None else ldy, n, d, k,
                                       nat.LASSO_F32 if dtype is None else dtype, None)


def test_c_abi_refusals_need_no_device():
    from lasso_amd import _native as nat
    L = nat.lib()
    bad, unsup = nat.LASSO_ERR_BAD_ARG, nat.LASSO_ERR_UNSUPPORTED
    assert _solve_status(L, nat, dtype=nat.LASSO_F64) == unsup
    assert _solve_status(L, nat, dtype=nat.LASSO_BF16) == unsup
    assert _solve_status(L, nat, d=257) == unsup
    assert _solve_status(L, nat, k=4097) == unsup
    for kw in (dict(x=0), dict(w=0), dict(z0=0), dict(z=0), dict(ws=0), dict(ldx=2), dict(ldw=4), dict(ldz0=4), dict(ldz=4),
               dict(n=-1), dict(d=0), dict(k=0), dict(alpha=-1.0), dict(alpha=float("nan")), dict(maxiter=-1),
               dict(eps=-1.0), dict(eps=float("nan")), dict(tol=float("nan")), dict(barrier_init=float("nan")),
               dict(reserved=1), dict(reserved=1 << 40), dict(opts=0), dict(result=0)):
        assert _solve_status(L, nat, **kw) == bad, kw
    assert _solve_status(L, nat, n=0, x=0, z0=0, z=0, ws=0) == nat.LASSO_OK           # nothing to do, nothing written
    # a well-formed call gets as far as the workspace check (0 bytes given), still without a launch
    assert _solve_status(L, nat) == nat.LASSO_ERR_WORKSPACE
    assert _solve_status(L, nat, d=256, k=4096, tol=0.0, maxiter=0) == nat.LASSO_ERR_WORKSPACE
    # the row kernel's entry point
    assert _rows_status(L, nat, dtype=nat.LASSO_F64) == unsup
    assert _rows_status(L, nat, d=257) == unsup and _rows_status(L, nat, k=4097) == unsup
    for kw in (dict(w=0), dict(c=0), dict(b=0), dict(y=0), dict(ldw=4), dict(ldc=4), dict(ldb=2), dict(ldy=2), dict(n=-1),
               dict(d=0), dict(k=0)):
        assert _rows_status(L, nat, **kw) == bad, kw
    assert _rows_status(L, nat, n=0, w=0, c=0, b=0, y=0) == nat.LASSO_OK


def test_refusals_come_before_any_native_call(monkeypatch):
    from lasso_amd import _native
    from lasso_amd.linear.solvers import interior_point

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_native, "lib", boom)
    monkeypatch.setattr(_native, "require_gpu", boom)
    w, x, z0 = torch.randn(16, 40), torch.randn(24, 16), torch.ones(24, 40)
    for args in ((x[0], w, z0), (x, w[0], z0), (x, w, z0[0]), (x, w, torch.ones(23, 40)), (x, w, torch.ones(24, 39)),
                 (x, torch.randn(15, 40), None)):                           # the reference's asserts
        with pytest.raises(AssertionError) as e:
            interior_point(args[0], args[1], z0=args[2])
        assert "native call" not in str(e.value)
    for t in ((x.double(), w.double(), z0.double()), (x, w, z0.double()), (x.double(), w, None)):
        with pytest.raises(NotImplementedError, match="float64"):
            interior_point(t[0], t[1], z0=t[2])
    with pytest.raises(NotImplementedError, match="bfloat16"):
        interior_point(x.bfloat16(), w.bfloat16(), z0=z0.bfloat16())
    with pytest.raises(NotImplementedError, match="float16"):
        interior_point(x.half(), w.half())
    with pytest.raises(NotImplementedError, match="256"):
        interior_point(torch.randn(2, 257), torch.randn(257, 8))
    with pytest.raises(NotImplementedError, match="4096"):
        interior_point(torch.randn(2, 3), torch.randn(3, 4097), z0=torch.ones(2, 4097))
    for which in range(3):
        t = [x.clone(), w.clone(), z0.clone()]
        t[which].requires_grad_()
        with pytest.raises(NotImplementedError, match="autograd"):
            interior_point(t[0], t[1], z0=t[2])
    # n = 0: an empty result and False, with no native call
    z, ok = interior_point(x[:0], w, z0=z0[:0])
    assert z.shape == (0, 40) and ok is False
    z, ok, info = interior_point(x[:0], w, return_info=True)
    assert z.shape == (0, 40) and ok is False and info["iterations"] == 0
    # a well-formed call reaches the native layer; so does one whose inputs require grad outside grad mode
    with pytest.raises(AssertionError, match="native call"):
        interior_point(x, w, z0=z0)
    with torch.no_grad(), pytest.raises(AssertionError, match="native call"):
        interior_point(x, w.requires_grad_(), z0=z0)


def test_no_gpu_is_a_native_error_not_a_cpu_result():
    from lasso_amd import _native
    from lasso_amd.linear.solvers import interior_point
    if torch.cuda.is_available():        # a GPU is visible: tests/test_interior_point_gpu.py covers the solve
        return
    with pytest.raises(_native.NativeError):
        interior_point(torch.randn(4, 3), torch.randn(3, 5), z0=torch.ones(4, 5), maxiter=2)


def test_every_stored_case_satisfies_its_caps(cases):
    assert {key.split("/")[0] for key in cases.files} == set(CASES)
    for name, spec in CASES.items():
        g = load_case(cases, name)
        n, k = spec["n"], spec["k"]
        assert g["z32"].shape == (n, k) and g["z32"].dtype == np.float32
        assert g["z64"].shape == (n, k) and g["z64"].dtype == np.float64
        its = len(g["obj32"])
        assert 1 <= its <= spec["kwargs"].get("maxiter", 20) and len(g["obj64"]) == its
        assert all(len(g[key + "32"]) == its for key in RECORDS)
        assert bool(g["success"]) == bool(spec.get("stops")) and (its < spec["kwargs"].get("maxiter", 20)) == bool(g["success"])
        if spec["compare"] == "z":
            assert float(g["spread_z"]) <= SPREAD_Z_CAP, name
            assert float(g["model_gap64"]) <= 1e-7, name
        if spec["compare"] == "f":
            assert float(g["spread_f"]) <= SPREAD_F_CAP, name
        tol = float(g["tol"])
        assert tol == spec["kwargs"].get("tol", 1e-2)
        if tol > 0:                                                          # (a): no stop decision rounding could flip
            for suffix in ("32", "64"):
                worst = np.max(np.stack([g[key + suffix] for key in ("prim", "dual", "gap")]), axis=0)
                assert ((worst > 1.01 * tol) | (worst < 0.99 * tol)).all(), name
                assert (worst[:-1] > 1.01 * tol).all() and (worst[-1] < 0.99 * tol) == bool(g["success"]), name
    # the cases that are there for a path took it
    assert len(cases["stop_odd/obj32"]) == 4 and len(cases["stop_d256/obj32"]) == 5
    assert CASES["d256"]["d"] == 256 and CASES["d33"]["d"] == 33 and CASES["odd"]["k"] % 4 and CASES["odd"]["d"] % 4


def test_float32_model_within_64_ulp_of_the_reference(cases):
    """Certification (b) as stored: where codes are compared, the float32 model in the reference's order is within 64 ulp
    of max |z| of the reference's float32 codes and the float64 model within 1e-7 of its float64 codes; the model in the
    HIP path's order (halves merged first) is within 1e-7 of the float64 codes too, which holds the formulation itself."""
    for name, spec in CASES.items():
        g = load_case(cases, name)
        bar = 64 * float(np.finfo(np.float32).eps) * max(1.0, float(np.abs(g["z32"]).max()))
        assert float(g["model_bar32"]) == bar
        if spec["compare"] == "z":
            assert float(g["model_gap32"]) <= bar, (name, float(g["model_gap32"]), bar)
            assert float(g["model_gap64"]) <= 1e-7 and float(g["model_gap64_path"]) <= 1e-7, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_in_the_paths_order(cases, name):
    """order_seed: the halves merged first (c = d+ + d-, z+ - z-), every contraction and every system permuted.  In
    float64 that is the reference's float64 run to 1e-6; in float32 it is "another correct implementation", inside the
    bars the GPU tests hold the kernels to."""
    spec, g = CASES[name], load_case(cases, name)
    x, w, z0 = case_inputs(spec)
    z64, ok64, i64 = interior_point_model.interior_point(x, w, z0, alpha=spec["alpha"], dtype=torch.float64, order_seed=3,
                                                         **spec["kwargs"])
    z32, ok32, i32 = interior_point_model.interior_point(x, w, z0, alpha=spec["alpha"], order_seed=3, **spec["kwargs"])
    assert i64["iterations"] == i32["iterations"] == len(g["obj32"]) and ok64 == ok32 == bool(g["success"])
    if spec["compare"] == "z":
        assert float((z64 - torch.from_numpy(g["z64"])).abs().max()) <= 1e-6
        assert float((z32 - torch.from_numpy(g["z32"])).abs().max()) <= max(5e-5, 4.0 * float(g["spread_z"]))
    else:
        for z, key in ((z64, "lasso64"), (z32, "lasso32")):
            f_rel = abs(lasso_objective(z, x, w, spec["alpha"]) - float(g[key])) / float(g[key])
            assert f_rel <= max(1e-6, 4.0 * float(g["spread_f"])), (name, key, f_rel)


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_reproduces_fixture(cases, name):
    """In the reference's order the model reproduces the recorded run on the CPU that recorded it; another CPU's BLAS may
    sum otherwise, and then it is "another correct float32 implementation": codes are held to the GPU tests' bar, max(5e-5, 4 x spread_z), with equal iteration counts and success, the
    objective-only cases to max(1e-6, 4 x spread_f); float64 codes to 1e-6; the per-iteration records to their bars."""
    spec, g = CASES[name], load_case(cases, name)
    x, w, z0 = case_inputs(spec)
    keep = x.clone(), w.clone(), z0.clone()
    z, ok, info = interior_point_model.interior_point(x, w, z0, alpha=spec["alpha"], **spec["kwargs"])
    z64, ok64, info64 = interior_point_model.interior_point(x, w, z0, alpha=spec["alpha"], dtype=torch.float64, **spec["kwargs"])
    assert torch.equal(x, keep[0]) and torch.equal(w, keep[1]) and torch.equal(z0, keep[2])
    assert torch.isfinite(z).all() and info["iterations"] == len(g["obj32"]) and info64["iterations"] == len(g["obj64"])
    assert ok == ok64 == bool(g["success"])
    if spec["compare"] == "z":
        dz = float((z - torch.from_numpy(g["z32"])).abs().max())
        assert dz <= max(5e-5, 4.0 * float(g["spread_z"])), (name, dz)
        assert float((z64 - torch.from_numpy(g["z64"])).abs().max()) <= 1e-6
    else:
        f_rel = abs(lasso_objective(z, x, w, spec["alpha"]) - float(g["lasso32"])) / float(g["lasso32"])
        assert f_rel <= max(1e-6, 4.0 * float(g["spread_f"])), (name, f_rel)
    assert abs(lasso_objective(z64, x, w, spec["alpha"]) - float(g["lasso64"])) <= 1e-6 * float(g["lasso64"])
    for key, got in (("obj", info["obj"]), ("prim", info["prim_feas"]), ("dual", info["dual_feas"]), ("gap", info["gap"])):
        rel = float(np.max(np.abs(np.array(got) - g[key + "32"]) / np.abs(g[key + "32"])))
        assert rel <= rtol_of(g, key), (name, key, rel)
