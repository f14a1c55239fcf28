"""The float64 M-step's ABI surface, the part that needs no GPU: the new entry points are declared, exported and
prototyped, check their arguments on the host before any HIP call, and size their workspaces as documented; the ABI
version has not moved."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lasso_hip.h")

NEW = ["lasso_gram_f64_workspace_bytes", "lasso_gram_accumulate_f64", "lasso_dict_sweep_f64_workspace_bytes",
       "lasso_dict_sweep_f64", "lasso_dict_fill_degenerate_f64", "lasso_zero_columns_f64",
       "lasso_ridge_f64_workspace_bytes", "lasso_ridge_solve_f64"]


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
    # double matrices, no dtype argument: the declarations take double*, and no `int dtype`
    for name in NEW:
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert "dtype" not in decl, name
        if not name.endswith("_workspace_bytes"):
            assert "double*" in decl and "float*" not in decl, name
    assert L.lasso_hip_abi_version() == 7 and nat.ABI_VERSION == 7
    assert re.search(r"#define\s+LASSO_HIP_ABI_VERSION\s+7\b", open(HEADER).read())


def test_bad_arguments_are_refused_on_the_host():
    nat, L = _lib()
    BAD = nat.LASSO_ERR_BAD_ARG
    none = None
    one = 0x1000                       # a non-null address that is never dereferenced: the size checks come first
    # null pointers
    assert L.lasso_gram_accumulate_f64(none, 12, none, 8, 5, 8, 12, none, none, none, 0, none) == BAD
    assert L.lasso_dict_sweep_f64(none, none, none, 12, 8, 12, 1e-10, 0, none, none, none, 0, none) == BAD
    assert L.lasso_dict_fill_degenerate_f64(none, 12, 8, 12, none, none, 1, 8, 0, none) == BAD
    assert L.lasso_zero_columns_f64(none, 12, 5, 12, none, none) == BAD
    assert L.lasso_ridge_solve_f64(none, none, none, 12, 8, 12, 0.1, none, none, 0, none) == BAD
    # zero sizes (n, d, k in turn), a leading dimension below the row length
    for n, d, k in [(0, 8, 12), (5, 0, 12), (5, 8, 0)]:
        assert L.lasso_gram_accumulate_f64(one, 12, one, 8, n, d, k, one, one, none, 0, none) == BAD, (n, d, k)
    assert L.lasso_gram_accumulate_f64(one, 11, one, 8, 5, 8, 12, one, one, none, 0, none) == BAD
    for d, k in [(0, 12), (8, 0)]:
        assert L.lasso_dict_sweep_f64(one, one, one, 12, d, k, 1e-10, 0, one, none, one, 1 << 20, none) == BAD, (d, k)
        assert L.lasso_dict_fill_degenerate_f64(one, 12, d, k, one, one, 1, 8, 0, none) == BAD, (d, k)
        assert L.lasso_ridge_solve_f64(one, one, one, 12, d, k, 0.1, none, one, 1 << 20, none) == BAD, (d, k)
    assert L.lasso_dict_fill_degenerate_f64(one, 12, 8, 12, one, one, 0, 8, 0, none) == BAD           # no pool rows
    for n, k in [(0, 12), (5, 0)]:
        assert L.lasso_zero_columns_f64(one, 12, n, k, one, none) == BAD, (n, k)
    # beyond the limits: unsupported, and the workspace queries say 0
    UNS = nat.LASSO_ERR_UNSUPPORTED
    assert L.lasso_dict_sweep_f64(one, one, one, 4097, 8, 4097, 1e-10, 0, one, none, one, 1 << 20, none) == UNS
    assert L.lasso_dict_sweep_f64(one, one, one, 12, 1025, 12, 1e-10, 0, one, none, one, 1 << 20, none) == UNS
    assert L.lasso_ridge_solve_f64(one, one, one, 4097, 8, 4097, 0.1, none, one, 1 << 20, none) == UNS
    assert L.lasso_dict_sweep_f64_workspace_bytes(1025, 12) == 0 and L.lasso_dict_sweep_f64_workspace_bytes(8, 4097) == 0
    # a workspace that is too small
    assert L.lasso_dict_sweep_f64(one, one, one, 12, 8, 12, 1e-10, 0, one, none, one, 16, none) == nat.LASSO_ERR_WORKSPACE
    assert L.lasso_ridge_solve_f64(one, one, one, 12, 8, 12, 0.1, none, one, 16, none) == nat.LASSO_ERR_WORKSPACE


def test_workspace_queries():
    nat, L = _lib()
    for n, d, k in [(4096, 256, 1024), (37, 10, 50), (300, 300, 520)]:
        assert L.lasso_gram_f64_workspace_bytes(n, d, k) >= 8 * (k * k + k * d)          # at least one split's slabs
        assert L.lasso_dict_sweep_f64_workspace_bytes(d, k) >= 8 * k * d                 # U = B - A D^T
        assert L.lasso_ridge_f64_workspace_bytes(d, k) >= 8 * (k + d) * k                # [A + lam I ; B^T]
    assert L.lasso_ridge_f64_workspace_bytes(256, 4096) > 0
    assert L.lasso_ridge_f64_workspace_bytes(256, 4097) == 0
    assert L.lasso_gram_f64_workspace_bytes(0, 8, 12) == 0
