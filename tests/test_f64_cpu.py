"""float64 on the HIP path, the part that needs no GPU: the built library's ABI surface for LASSO_F64, the refusal
to fall back to the CPU, and the float64 fixture of the real reference against the oracle."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lasso_hip.h")


def _lib():
    from lasso_amd import _native as nat
    return nat, nat.lib()


def test_abi_version_is_unchanged_and_f64_is_additive():
    nat, L = _lib()
    assert L.lasso_hip_abi_version() == 7 and nat.ABI_VERSION == 7
    assert nat.LASSO_F64 == 2
    text = open(HEADER).read()
    assert re.search(r"#define\s+LASSO_HIP_ABI_VERSION\s+7\b", text)
    assert re.search(r"LASSO_F64\s*=\s*2\b", text)


def test_every_header_symbol_is_exported():
    nat, _ = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lasso_[a-z0-9_]+)\s*\(", text))
    declared.discard("lasso_allreduce_fn")
    assert {"lasso_fista_solve_f64", "lasso_objective_f64", "lasso_objective_f64_workspace_bytes"} <= declared
    out = subprocess.check_output(["nm", "-D", "--defined-only", nat.lib_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not (declared - exported), sorted(declared - exported)


def test_workspace_holds_the_double_state_and_the_kernel_is_named():
    nat, L = _lib()
    n, d, k = 4096, 256, 1024
    nbytes = L.lasso_fista_workspace_bytes(n, d, k, nat.LASSO_F64, 100, 0.0, 0, 0)
    assert nbytes >= 8 * (n * k + n * d)            # the momentum point and the residual, in double
    # the stop rule's checkpoints and the line search's candidate need room as well
    assert L.lasso_fista_workspace_bytes(n, d, k, nat.LASSO_F64, 100, 1e-5, 0, 0) >= 8 * (3 * n * k + n * d)
    assert L.lasso_fista_workspace_bytes(n, d, k, nat.LASSO_F64, 100, 0.0, 0, 1) >= 8 * (3 * n * k + n * d)
    for backtrack in (0, 1):
        name = L.lasso_fista_kernel_name(n, d, k, nat.LASSO_F64, backtrack).decode()
        assert "f64" in name, name
    # beyond the fused shapes too: the float64 path is the general GEMM for any d, k
    assert L.lasso_fista_workspace_bytes(128, 512, 4096, nat.LASSO_F64, 10, 0.0, 0, 0) >= 8 * (128 * 4096 + 128 * 512)
    assert L.lasso_objective_f64_workspace_bytes(n, d, k) >= 8 * n * d
    # the fp32 answers are what they were (the dtype argument picks the float64 sizes, nothing else moved)
    assert 0 < L.lasso_fista_workspace_bytes(n, d, k, nat.LASSO_F32, 100, 0.0, 0, 0) < nbytes


def test_no_cpu_fallback_for_float64():
    from lasso_amd import _native as nat
    from lasso_amd.linear import sparse_encode, lasso_loss
    from lasso_amd.linear.lipschitz import lipschitz_constant
    from lasso_amd.linear.solvers import ista
    from lasso_amd.linear.solvers.ista import _DT
    assert _DT[torch.float64] == nat.LASSO_F64          # float64 reaches the native layer, it is not refused in Python
    x = torch.randn(5, 8, dtype=torch.float64)
    w = torch.randn(8, 12, dtype=torch.float64)
    z0 = torch.zeros(5, 12, dtype=torch.float64)
    if not torch.cuda.is_available():        # fails loudly (NativeError), not NotImplementedError and not a CPU result
        with pytest.raises(nat.NativeError):
            ista(x, z0, w, 0.3, lr=0.1)
        with pytest.raises(nat.NativeError):
            sparse_encode(x, w, alpha=0.3)
        with pytest.raises(nat.NativeError):
            lipschitz_constant(w)
        with pytest.raises(nat.NativeError):
            lasso_loss(x, z0, w)


def test_f64_entry_points_check_their_arguments_not_the_dtype():
    """host side, before any HIP call: the entry points of the float64 list answer LASSO_ERR_BAD_ARG to a bad shape or
    a null pointer with LASSO_F64 (they used to answer LASSO_ERR_UNSUPPORTED to the dtype itself); one outside the list
    still refuses the dtype"""
    nat, L = _lib()
    F64, BAD, UNS = nat.LASSO_F64, nat.LASSO_ERR_BAD_ARG, nat.LASSO_ERR_UNSUPPORTED
    none = None
    assert L.lasso_fista_solve(none, 8, none, 12, none, 0, none, 12, 5, 0, 12, F64, 0.3, 0.1, 1, 3, 0.0, 0, 0, 1.5,
                               none, none, none, none, none, none, none, 0, none) == BAD           # d = 0
    assert L.lasso_fista_solve_f64(none, 8, none, 12, none, 0, none, 12, 5, 8, 12, 0.3, 0.1, 1, 3, 0.0, 0, 0, 1.5,
                                   none, none, none, none, none, none, none, 0, none) == BAD       # null pointers
    assert L.lasso_fista_solve_f64(none, 8, none, 12, none, 0, none, 12, 5, 8, 12, 0.3, 0.1, 1, 3, 0.0, nat.SOLVE_ASYNC,
                                   0, 1.5, none, none, none, none, none, none, none, 0, none) == UNS
    assert L.lasso_lipschitz(none, 12, 8, 12, F64, none, none, 0, none) == BAD
    assert L.lasso_objective(none, 8, none, 12, none, 12, 5, 8, 12, F64, 0.7, none, none, none, 0, none) == BAD
    assert L.lasso_objective_throttled(none, 8, none, 12, none, 12, 5, 8, 12, F64, 0.7, none, none, 0, none, 0,
                                       none) == BAD
    assert L.lasso_objective_f64(none, 8, none, 12, none, 12, 5, 8, 12, 0.7, none, none, none, 0, none) == BAD
    assert L.lasso_init_transpose(5, 8, 12, F64, none, 8, none, 12, none, 12, none, 0, none) == BAD
    assert L.lasso_gram_accumulate(none, 12, none, 8, 5, 8, 12, F64, none, none, none, 0, none) == UNS
    assert L.lasso_fista_prepare(none, 12, 8, 12, F64, 4, none, 0, none) == UNS


def test_oracle_reproduces_the_references_float64_codes(golden_this_cpu):
    """tests/golden/f64_cases.npz holds float64 codes of the REAL reference (generate_golden_f64.py).  The oracle runs
    the same ATen ops in the same order, so it gives them bit for bit, as the fp32 fixtures are pinned: against the
    recorded run of the kind of CPU this is (tests/golden_runs.py; further runs: generate_golden_f64.py --run NAME),
    else against the primary recording.  Only the primary run has been recorded so far: on another kind of CPU (the
    recorded fp32 run `cpu2`, for one: its float64 GEMM leaves the oracle 2.0e-15 from the primary recording in the first
    case) the test fails until the reference has been recorded there."""
    import warnings
    from oracle import lasso_oracle as orc
    from golden_f64 import CASES, case_inputs, case_step
    g = golden_this_cpu("f64_cases")
    for tag, case in CASES.items():
        lr = float(g[tag + "_lr"])
        assert abs(lr - case_step(case)) <= 1e-12 * lr
        X, W, z0, kw = case_inputs(case, lr=lr)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            z = orc.fista(X, z0, W, case["alpha"], **kw)
        ref = torch.from_numpy(g[tag + "_z"])
        assert z.dtype is torch.float64 and ref.dtype is torch.float64
        assert torch.equal(z, ref), (
            "%s: the oracle differs from the reference's recorded float64 code by %g (recorded run: %s); on a kind of "
            "CPU without a recorded run, record one with generate_golden_f64.py --run"
            % (tag, (z - ref).abs().max().item(), golden_this_cpu.run or "primary"))
