"""The float64 convolutional path's ABI surface, the part that needs no GPU: the new entry points are declared,
exported and prototyped, the _f64 byte counts exceed their fp32 forms, and geometry, null pointers and the workspace
size are judged on the host before any HIP call."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lasso_hip.h")

NEW = ["lasso_conv_ista_solve_f64", "lasso_conv_objective_f64", "lasso_conv_lip_bound_f64",
       "lasso_conv_ista_workspace_bytes_f64", "lasso_conv_ista_trace_bytes_f64",
       "lasso_conv_ista_backward_workspace_bytes_f64", "lasso_conv_lip_workspace_bytes_f64"]

# N, C, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw: 3 x 3 kernel, stride 1, padding 1
GOOD = (3, 2, 12, 10, 24, 12, 10, 3, 3, 1, 1, 1, 1)
BAD_GEOM = (3, 2, 12, 11, 24, 12, 10, 3, 3, 1, 1, 1, 1)      # W does not match Wz


def _lib():
    from lasso_amd import _native as nat
    return nat, nat.lib()


def test_new_symbols_are_declared_exported_and_prototyped():
    nat, L = _lib()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lasso_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", nat.lib_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is not None, name      # prototyped in _native, not ctypes' defaults
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert "dtype" not in decl, name
    for name, slot in [("lasso_conv_ista_solve_f64", "double* last_delta_out"),
                       ("lasso_conv_objective_f64", "double* loss_dev"), ("lasso_conv_lip_bound_f64", "double* l_out")]:
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert slot in decl and "float*" not in decl, name
    # additive: the ABI version has not moved
    assert L.lasso_hip_abi_version() == 7 and nat.ABI_VERSION == 7
    assert re.search(r"#define\s+LASSO_HIP_ABI_VERSION\s+7\b", open(HEADER).read())


def test_f64_byte_counts_exceed_their_fp32_forms():
    _, L = _lib()
    # bench.py's three conv cases and a stride-2 geometry.  (On problems of a few hundred code pixels the comparison
    # says nothing: the fp32 count carries the fused kernel's tables and 256 KiB of partial sums, fixed sizes that the
    # double path does not have.)
    geoms = [(256, 1, 32, 32, 64, 26, 26, 7, 7, 1, 1, 0, 0), (64, 3, 64, 64, 128, 64, 64, 5, 5, 1, 1, 2, 2),
             (32, 16, 64, 64, 256, 64, 64, 3, 3, 1, 1, 1, 1), (8, 2, 79, 47, 48, 40, 24, 3, 3, 2, 2, 1, 1)]
    for g in geoms:
        assert L.lasso_conv_ista_workspace_bytes_f64(*g) > L.lasso_conv_ista_workspace_bytes(*g) > 0, g
        assert L.lasso_conv_ista_backward_workspace_bytes_f64(*g) > L.lasso_conv_ista_backward_workspace_bytes(*g) > 0, g
        for T in (0, 5):
            assert L.lasso_conv_ista_trace_bytes_f64(*g, T) == 2 * L.lasso_conv_ista_trace_bytes(*g, T) > 0, (g, T)
    for K, C, ks, sample in [(6, 2, 3, 50), (5, 9, 5, 50), (40, 3, 7, 50), (300, 400, 3, 2)]:
        assert L.lasso_conv_lip_workspace_bytes_f64(K, C, ks, sample) > L.lasso_conv_lip_workspace_bytes(K, C, ks, sample) > 0
    # a geometry that does not fit says 0, as the fp32 forms do
    assert L.lasso_conv_ista_workspace_bytes_f64(*BAD_GEOM) == 0
    assert L.lasso_conv_ista_backward_workspace_bytes_f64(*BAD_GEOM) == 0
    assert L.lasso_conv_ista_trace_bytes_f64(*BAD_GEOM, 3) == 0 and L.lasso_conv_ista_trace_bytes_f64(*GOOD, -1) == 0


def _calls(L, nat, geom, p, ws, ws_bytes):
    """every float64 route through the conv entry points with the pointers `p` / workspace `ws`"""
    F64 = nat.LASSO_F64
    return {
        "solve_f64": L.lasso_conv_ista_solve_f64(p, p, p, p, *geom, 0.1, 0.2, 1, 5, 0.0, None, None, ws, ws_bytes, None),
        "solve": L.lasso_conv_ista_solve(p, p, p, p, *geom, F64, 0.1, 0.2, 1, 5, 0.0, None, None, ws, ws_bytes, None),
        "objective_f64": L.lasso_conv_objective_f64(p, p, p, *geom, 0.1, p, ws, ws_bytes, None),
        "objective": L.lasso_conv_objective(p, p, p, *geom, F64, 0.1, p, ws, ws_bytes, None),
        "run_traced": L.lasso_conv_ista_run_traced(p, p, p, p, *geom, F64, 0.1, 0.2, 1, 5, p, ws, ws_bytes, None),
        "backward": L.lasso_conv_ista_backward(p, p, p, p, *geom, F64, 0.2, 1, 5, p, p, p, ws, ws_bytes, None),
    }


def test_arguments_are_judged_on_the_host():
    nat, L = _lib()
    one = 0x1000                       # a non-null address that is never dereferenced: the checks come first
    for name, status in _calls(L, nat, BAD_GEOM, one, one, 1 << 30).items():
        assert status == nat.LASSO_ERR_BAD_ARG, name
    for name, status in _calls(L, nat, BAD_GEOM, None, None, 0).items():
        assert status == nat.LASSO_ERR_BAD_ARG, name
    for name, status in _calls(L, nat, GOOD, None, None, 0).items():          # null required pointers
        assert status == nat.LASSO_ERR_BAD_ARG, name
    for name, status in _calls(L, nat, GOOD, None, one, 1 << 30).items():
        assert status == nat.LASSO_ERR_BAD_ARG, name
    for name, status in _calls(L, nat, GOOD, one, one, 0).items():            # a good geometry, no workspace
        assert status == nat.LASSO_ERR_WORKSPACE, name
    # one byte short is short
    need = L.lasso_conv_ista_workspace_bytes_f64(*GOOD)
    assert L.lasso_conv_ista_solve_f64(one, one, one, one, *GOOD, 0.1, 0.2, 1, 5, 0.0, None, None, one, need - 1,
                                       None) == nat.LASSO_ERR_WORKSPACE
    # the bound
    assert L.lasso_conv_lip_bound_f64(None, 6, 2, 3, 1, 50, 0, None, one, 1 << 20, None) == nat.LASSO_ERR_BAD_ARG
    assert L.lasso_conv_lip_bound_f64(one, 6, 2, 4, 1, 50, 0, None, one, 1 << 20, None) == nat.LASSO_ERR_BAD_ARG   # even kernel
    assert L.lasso_conv_lip_bound_f64(one, 6, 2, 3, 1, 50, 0, None, one, 0, None) == nat.LASSO_ERR_WORKSPACE
    # other dtypes stay refused
    assert L.lasso_conv_ista_solve(one, one, one, one, *GOOD, nat.LASSO_BF16, 0.1, 0.2, 1, 5, 0.0, None, None, one,
                                   1 << 30, None) == nat.LASSO_ERR_UNSUPPORTED


def test_no_cpu_result_without_a_gpu(monkeypatch):
    """What a box without a GPU answers (forced here, so that the test says the same on every box)."""
    from lasso_amd import _native as nat
    from lasso_amd.conv2d import ista_conv2d, lip_bound_conv2d
    from lasso_amd.conv2d.ista import conv_loss
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    g = torch.Generator().manual_seed(0)
    w = torch.randn(4, 2, 3, 3, generator=g, dtype=torch.float64)
    x = torch.randn(2, 2, 5, 5, generator=g, dtype=torch.float64)
    z0 = torch.zeros(2, 4, 5, 5, dtype=torch.float64)
    with pytest.raises(nat.NativeError):
        ista_conv2d(x, z0, w, 0.1, padding=1, lr=0.1)
    with pytest.raises(nat.NativeError):
        conv_loss(x, z0, w, 0.1, padding=1)
    with pytest.raises(nat.NativeError):
        lip_bound_conv2d(w, 1)
