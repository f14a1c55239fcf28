"""split_bregman without a GPU: the Python surface equals the reference's, the C boundary declares and exports the new
symbols and its structs have the size of their ctypes mirrors, every refusal and ValueError comes before any native
call, the host model (tests/split_bregman_model.py) reproduces the fixture recorded from the reference (bit for bit on
the kind of CPU it was recorded on, within the stored spread elsewhere), and every stored case satisfies the conditions
it was certified under."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import split_bregman_model as model
from split_bregman_cases import CASES, SPREAD_Z_CAP, bar_z, case_inputs, load_case, rtol_update

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    return golden("split_bregman_cases")


def test_python_surface():
    import lasso_amd.linear.solvers.split_bregman  # noqa: F401  (the module; absent before this solver)
    from lasso_amd.linear.solvers import split_bregman
    import lasso_amd.linear  # noqa: F401
    assert split_bregman is sys.modules["lasso_amd.linear.solvers.split_bregman"].split_bregman
    sig = inspect.signature(split_bregman)
    assert list(sig.parameters) == ["A", "y", "x0", "alpha", "lambd", "maxiter", "niter_inner", "tol", "tau", "verbose",
                                    "return_info"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["x0"], d["alpha"], d["lambd"], d["maxiter"], d["niter_inner"], d["tol"], d["tau"], d["verbose"],
            d["return_info"]) == (None, 1.0, 1.0, 20, 5, 1e-10, 1., False, False)
    # not an algorithm= arm: sparse_encode's table is as it was
    se = sys.modules["lasso_amd.linear.sparse_encode"]
    assert set(se._OFF_PATH_ALGOS) == {"iter-ridge", "interior-point", "split-bregman", "own"}
    doc = split_bregman.__doc__
    for word in ("itn", "maxiter - 1", "not the shrunk", "x0", "ValueError", "never stop", "iter %3d - cost: %0.4f",
                 "LinAlgError", "NaN", "requires_grad", "4096", "Out of scope", "Woodbury"):
        assert word in doc, word


def test_sparse_encode_arm_still_raises():
    from lasso_amd.linear import sparse_encode
    with pytest.raises(NotImplementedError):
        sparse_encode(torch.randn(4, 3), torch.randn(3, 5), 0.1, algorithm="split-bregman")


def test_symbols_declared_and_exported():
    from lasso_amd import _native
    text = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()
    for name in ("lasso_split_bregman_workspace_bytes", "lasso_split_bregman_solve", "lasso_split_bregman_options",
                 "lasso_split_bregman_trace", "lasso_split_bregman_result"):
        assert name in text, name
    assert "the Split Bregman solver is lasso_split_bregman_solve" in text          # the capability list
    assert "#define LASSO_HIP_ABI_VERSION 7" in text          # additive: the version stays
    raw = ctypes.CDLL(_native.lib_path())
    assert hasattr(raw, "lasso_split_bregman_workspace_bytes") and hasattr(raw, "lasso_split_bregman_solve")
    L = _native.lib()
    assert L.lasso_hip_abi_version() == 7
    small = L.lasso_split_bregman_workspace_bytes(64, 32, 128, _native.LASSO_F32)
    assert small >= (64 * 128 * 5 + 128 * 128) * 4            # Aty, two T, B, X; Hinv
    assert L.lasso_split_bregman_workspace_bytes(4096, 256, 1024, _native.LASSO_F32) > small
    assert L.lasso_split_bregman_workspace_bytes(0, 32, 128, _native.LASSO_F32) > 0
    assert L.lasso_split_bregman_workspace_bytes(64, 32, 4097, _native.LASSO_F32) == 0
    for dtype in (_native.LASSO_BF16, _native.LASSO_F64):
        assert L.lasso_split_bregman_workspace_bytes(64, 32, 128, dtype) == 0


def test_struct_sizes_match_the_header(tmp_path):
    from lasso_amd import _native as nat
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lasso_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(lasso_split_bregman_options), sizeof(lasso_split_bregman_trace), '
                   'sizeof(lasso_split_bregman_result), __builtin_offsetof(lasso_split_bregman_options, lambd), '
                   '__builtin_offsetof(lasso_split_bregman_trace, cost), '
                   '__builtin_offsetof(lasso_split_bregman_result, trace)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    build = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [ctypes.sizeof(nat.SplitBregmanOptions), ctypes.sizeof(nat.SplitBregmanTrace),
                   ctypes.sizeof(nat.SplitBregmanResult), nat.SplitBregmanOptions.lambd.offset,
                   nat.SplitBregmanTrace.cost.offset, nat.SplitBregmanResult.trace.offset]


def _solve_status(L, nat, n=4, d=3, k=5, dtype=None, ldx=None, ldw=None, ldx0=None, ldz=None, x=1, w=1, x0=1, z=1, ws=1,
                  alpha=0.1, opts=1, result=1, maxiter=3, niter_inner=2, reserved=0, lambd=1.0, tol=1e-10, tau=1.0):
    """lasso_split_bregman_solve with fake (never dereferenced) pointers: every refusal comes before the first HIP call"""
    p = lambda on: ctypes.c_void_p(0x1000 if on else 0)                                  # noqa: E731
    o = nat.SplitBregmanOptions(maxiter, niter_inner, reserved, 0, lambd, tol, tau)
    r = nat.SplitBregmanResult()
    return L.lasso_split_bregman_solve(p(x), d if ldx is None else ldx, p(w), k if ldw is None else ldw, p(x0),
                                       k if ldx0 is None else ldx0, p(z), k if ldz is None else ldz, n, d, k,
                                       nat.LASSO_F32 if dtype is None else dtype, alpha, ctypes.byref(o) if opts else None,
                                       ctypes.byref(r) if result else None, p(ws), 0, None)


def test_c_abi_refusals_need_no_device():
    from lasso_amd import _native as nat
    L = nat.lib()
    bad, unsup, nan = nat.LASSO_ERR_BAD_ARG, nat.LASSO_ERR_UNSUPPORTED, float("nan")
    assert _solve_status(L, nat, dtype=nat.LASSO_F64) == unsup
    assert _solve_status(L, nat, dtype=nat.LASSO_BF16) == unsup
    assert _solve_status(L, nat, k=4097) == unsup
    for kw in (dict(x=0), dict(w=0), dict(z=0), dict(ws=0), dict(ldx=2), dict(ldw=4), dict(ldx0=4), dict(ldz=4),
               dict(n=-1), dict(d=0), dict(k=0), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=nan), dict(lambd=0.0),
               dict(lambd=-1.0), dict(lambd=nan), dict(tol=nan), dict(tau=nan), dict(maxiter=0), dict(niter_inner=0),
               dict(reserved=2), dict(reserved=-2), dict(opts=0), dict(result=0)):
        assert _solve_status(L, nat, **kw) == bad, kw
    assert _solve_status(L, nat, n=0, x=0, x0=0, z=0, ws=0) == nat.LASSO_OK           # nothing to do, nothing written
    # a well-formed call gets as far as the workspace check (0 bytes given), still without a launch: x0 may be null,
    # a negative tol and bit 0 of reserved are legal
    for kw in (dict(), dict(x0=0, ldx0=0), dict(tol=-1.0), dict(reserved=1)):
        assert _solve_status(L, nat, **kw) == nat.LASSO_ERR_WORKSPACE, kw


def test_refusals_come_before_any_native_call(monkeypatch):
    from lasso_amd import _native
    from lasso_amd.linear.solvers import split_bregman

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_native, "lib", boom)
    monkeypatch.setattr(_native, "require_gpu", boom)
    A, y, x0 = torch.randn(16, 40), torch.randn(24, 16), torch.zeros(24, 40)
    nan = float("nan")
    for kw in (dict(maxiter=0), dict(maxiter=-3), dict(niter_inner=0), dict(alpha=0.0), dict(alpha=-1.0), dict(lambd=0.0),
               dict(lambd=-2.0), dict(alpha=nan), dict(lambd=nan), dict(tau=nan), dict(tol=nan)):
        with pytest.raises(ValueError, match="split_bregman"):
            split_bregman(A, y, x0, **kw)
    for bad in ((A, y[0]), (A[0], y), (A, torch.randn(24, 15)), (A, y, torch.zeros(24, 39)), (A, y, torch.zeros(23, 40))):
        with pytest.raises(AssertionError) as e:                 # the reference's asserts
            split_bregman(*bad)
        assert "native call" not in str(e.value)
    for t in ((A.double(), y.double(), x0.double()), (A, y, x0.double()), (A.double(), y)):
        with pytest.raises(NotImplementedError, match="float64"):
            split_bregman(*t)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        split_bregman(A.bfloat16(), y.bfloat16())
    with pytest.raises(NotImplementedError, match="float16"):
        split_bregman(A.half(), y.half())
    with pytest.raises(NotImplementedError, match="4096"):
        split_bregman(torch.randn(3, 4097), torch.randn(2, 3))
    for t in ((A.clone().requires_grad_(), y, x0), (A, y.clone().requires_grad_()), (A, y, x0.clone().requires_grad_())):
        with pytest.raises(NotImplementedError, match="requires_grad"):
            split_bregman(*t)
    # and a well-formed call reaches the native layer: a negative tol is legal, and so is requires_grad without grad mode
    with pytest.raises(AssertionError, match="native call"):
        split_bregman(A, y, x0, tol=-1.0)
    with torch.no_grad(), pytest.raises(AssertionError, match="native call"):
        split_bregman(A.clone().requires_grad_(), y)


def test_no_gpu_is_a_native_error_not_a_cpu_result():
    from lasso_amd import _native
    from lasso_amd.linear.solvers import split_bregman
    if torch.cuda.is_available():        # a GPU is visible: tests/test_split_bregman_gpu.py covers the solve
        return
    with pytest.raises(_native.NativeError):
        split_bregman(torch.randn(3, 5), torch.randn(4, 3), maxiter=2)


def test_every_stored_case_is_certified(cases):
    assert {key.split("/")[0] for key in cases.files} == set(CASES)
    for name, spec in CASES.items():
        g = load_case(cases, name)
        n, k = spec["n"], spec["k"]
        kw = spec["kwargs"]
        maxiter, tol = kw.get("maxiter", 20), kw.get("tol", 1e-10)
        assert g["x32"].shape == (n, k) and g["x32"].dtype == np.float32
        assert g["x64"].shape == (n, k) and g["x64"].dtype == np.float64
        its = int(g["iterations"])
        assert 1 <= its <= maxiter and len(g["update32"]) == len(g["update64"]) == its
        assert int(g["itn"]) == (its if bool(g["stopped"]) else maxiter - 1)
        assert bool(g["stopped"]) == (its < maxiter)
        assert float(g["spread_z"]) <= SPREAD_Z_CAP and np.isfinite(float(g["spread_update"])), name
        assert bar_z(g) <= 1e-2
        for u in list(g["update32"]) + list(g["update64"]):
            assert abs(u - tol) >= 0.01 * tol, name
        assert float(g["model_gap"]) == 0.0, name            # the model was the reference bit for bit when it was recorded
    # the cases that are there for a path took it
    assert bool(cases["tol_1em2/stopped"]) and 1 < int(cases["tol_1em2/itn"]) < 200
    assert cases["tol_1em2/update32"][-1] <= 1e-2 < cases["tol_1em2/update32"][-2]
    assert int(cases["maxiter_1/itn"]) == 0 and int(cases["maxiter_1/iterations"]) == 1
    assert not (cases["n37_d19_k70/x32"] == 0).any()          # x is the linear solve's X: dense


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
    """On the kind of CPU the fixture was recorded on the float32 model IS the reference: bit for bit, and within 1e-9
    in float64.  Another CPU's BLAS sums in another order -- it is "another correct float32 implementation", which is
    what spread_z / spread_update measured when the fixture was made: there x is held to the GPU tests' bar,
    max(5e-5, 4 x spread_z), with the same iteration count, and the updates to max(1e-5, 4 x spread_update)."""
    spec, g = CASES[name], load_case(cases, name)
    A, y, x0 = case_inputs(spec)
    keep = A.clone(), y.clone(), None if x0 is None else x0.clone()
    x, itn, info = model.split_bregman(A, y, x0, alpha=spec["alpha"], **spec["kwargs"])
    x64, itn64, info64 = model.split_bregman(A, y, x0, alpha=spec["alpha"], dtype=torch.float64, **spec["kwargs"])
    assert torch.equal(A, keep[0]) and torch.equal(y, keep[1]) and (x0 is None or torch.equal(x0, keep[2]))
    assert itn == itn64 == int(g["itn"]) and info["iterations"] == int(g["iterations"])
    assert info["stopped"] == bool(g["stopped"])
    dx = float((x - torch.from_numpy(g["x32"])).abs().max())
    dx64 = float((x64 - torch.from_numpy(g["x64"])).abs().max())
    if recorded_on_this_kind_of_cpu:
        assert torch.equal(x, torch.from_numpy(g["x32"])), dx
        assert info["update"] == list(g["update32"])
        assert dx64 <= 1e-9
        return
    assert dx <= bar_z(g), (name, dx)
    assert dx64 <= 1e-6, (name, dx64)
    rel = float(np.max(np.abs(np.array(info["update"]) - g["update32"]) / g["update32"]))
    assert rel <= rtol_update(g), (name, rel)


def test_model_x0_only_moves_the_first_update():
    """the property the GPU test asserts of the kernels, on the model: x0 enters through Xold of iteration 0 alone"""
    spec = CASES["n37_d19_k70"]
    A, y, _ = case_inputs(spec)
    g = torch.Generator().manual_seed(11)
    xa, ia, fa = model.split_bregman(A, y, torch.randn(37, 70, generator=g), alpha=0.3, maxiter=4)
    xb, ib, fb = model.split_bregman(A, y, torch.randn(37, 70, generator=g), alpha=0.3, maxiter=4)
    assert torch.equal(xa, xb) and fa["update"][1:] == fb["update"][1:] and fa["update"][0] != fb["update"][0]
