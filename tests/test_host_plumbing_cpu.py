"""The host plumbing every feature shares, the part that needs no GPU: _native.DT / one_dtype / pick_device, and the
error channel of the C ABI (lasso::fail): the float64 and GPSR drivers report through it directly, and the texts that
come back through lasso_hip_last_error are the ones these bad arguments have always produced."""
import ctypes as C

import pytest
import torch


def test_one_dtype():
    from lasso_amd import _native as nat
    f64 = torch.zeros(2, 2, dtype=torch.float64)
    f32 = torch.zeros(2, 2)
    bf16 = torch.zeros(2, 2, dtype=torch.bfloat16)
    assert nat.one_dtype("op", f64) is True and nat.one_dtype("op", f64, f64, f64) is True
    assert nat.one_dtype("op", f32) is False and nat.one_dtype("op", f32, bf16) is False     # none is float64
    assert nat.one_dtype("op", f64, None, f64) is True and nat.one_dtype("op", None, f32) is False
    assert nat.one_dtype("op") is False and nat.one_dtype("op", None) is False
    with pytest.raises(RuntimeError) as e:
        nat.one_dtype("gram", f64, f32, None, f64)
    assert str(e.value) == "gram: expected tensors of one dtype, got torch.float64, torch.float32, torch.float64"
    with pytest.raises(RuntimeError):
        nat.one_dtype("dict_learning", f32, f64)


def test_dtype_table():
    from lasso_amd import _native as nat
    from lasso_amd.linear.solvers.ista import _DT
    assert _DT is nat.DT
    assert nat.DT == {torch.float32: nat.LASSO_F32, torch.bfloat16: nat.LASSO_BF16, torch.float64: nat.LASSO_F64}


def test_pick_device_of_cpu_tensors_is_the_current_hip_device(monkeypatch):
    from lasso_amd import _native as nat
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 3)
    x, w = torch.zeros(2, 2), torch.zeros(2, 2, dtype=torch.float64)
    assert nat.pick_device(x, w) == torch.device("cuda", 3)
    assert nat.pick_device(x, None, w) == torch.device("cuda", 3)
    assert nat.pick_device() == torch.device("cuda", 3)


def test_no_gpu_is_reported_before_a_device_is_picked():
    from lasso_amd import _native as nat
    from lasso_amd.linear import lasso_loss, update_dict_ridge
    x, z, w = torch.randn(5, 8), torch.randn(5, 12), torch.randn(8, 12)
    if not torch.cuda.is_available():        # NativeError, not whatever torch.cuda.current_device() raises
        with pytest.raises(nat.NativeError):
            lasso_loss(x, z, w)
        with pytest.raises(nat.NativeError):
            update_dict_ridge(x, z)


# (call, status, text) of host-side failures -- all of them before any HIP call, so the pointers are never read
_P = 4096


def _failures(nat, L):
    p, none = C.c_void_p(_P), None
    o = nat.GpsrOptions()
    o.lambda_backtrack, o.maxiter = 0.5, 3
    r = nat.GpsrResult()
    tail = (none, none, none, none, none, none, p, 16, none)
    return [
        # float64 drivers (gemm_f64.hip), reached through both entry points
        (lambda: L.lasso_fista_solve_f64(p, 8, p, 12, none, 0, p, 12, 5, 8, 12, 0.3, 0.1, 1, 3, 0.0, 0, 0, 1.5, *tail),
         nat.LASSO_ERR_WORKSPACE, "workspace 16 < 9728 bytes"),
        (lambda: L.lasso_fista_solve_f64(p, 8, p, 12, none, 0, p, 12, 5, 8, 12, 0.3, 0.1, 1, 3, 0.0, 0, 1, 1.5, *tail),
         nat.LASSO_ERR_WORKSPACE, "workspace 16 < 51968 bytes"),
        (lambda: L.lasso_fista_solve(p, 8, p, 12, none, 0, p, 12, 5, 8, 12, nat.LASSO_F64, 0.3, 0.1, 1, 3, 0.0, 0, 0, 1.5, *tail),
         nat.LASSO_ERR_WORKSPACE, "workspace 16 < 9728 bytes"),
        (lambda: L.lasso_objective_f64(p, 8, p, 12, p, 12, 5, 8, 12, 0.7, p, none, p, 16, none),
         nat.LASSO_ERR_WORKSPACE, "need 17152 bytes"),
        (lambda: L.lasso_objective(p, 8, p, 12, p, 12, 5, 8, 12, nat.LASSO_F64, 0.7, p, none, p, 16, none),
         nat.LASSO_ERR_WORKSPACE, "need 17152 bytes"),
        # GPSR driver (gpsr.hip)
        (lambda: L.lasso_gpsr_solve(p, 1 << 23, p, 12, none, 0, p, 12, 5, 8, 12, nat.LASSO_F32, 0.3, C.byref(o), C.byref(r), p,
                            1 << 40, none),
         nat.LASSO_ERR_UNSUPPORTED, "row pitch beyond the 32-bit offsets of a 64-row block"),
        (lambda: L.lasso_gpsr_solve(p, 8, p, 12, none, 0, p, 12, 5, 8, 12, nat.LASSO_F32, 0.3, C.byref(o), C.byref(r), p, 16, none),
         nat.LASSO_ERR_WORKSPACE, "need 333056 bytes"),
        # the C-ABI layer itself, and the regions behind the solver's workspace (lr = LASSO_LR_AUTO)
        (lambda: L.lasso_fista_solve_f64(none, 8, none, 12, none, 0, none, 12, 5, 0, 12, 0.3, 0.1, 1, 3, 0.0, 0, 0, 1.5, none, none,
                                 none, none, none, none, none, 0, none),
         nat.LASSO_ERR_BAD_ARG, "bad shape n=5 d=0 k=12"),
        (lambda: L.lasso_fista_solve_f64(none, 8, none, 12, none, 0, none, 12, 5, 8, 12, 0.3, 0.1, 1, 3, 0.0, nat.SOLVE_ASYNC, 0,
                                 1.5, none, none, none, none, none, none, none, 0, none),
         nat.LASSO_ERR_UNSUPPORTED, "LASSO_F64: asynchronous and sharded solves are fp32 only"),
        (lambda: L.lasso_fista_solve(p, 8, p, 12, none, 0, p, 12, 5, 8, 12, nat.LASSO_F32, 0.3, nat.LR_AUTO, 1, 3, 0.0, 0, 0, 1.5,
                             *tail),
         nat.LASSO_ERR_WORKSPACE, "workspace 16 < 13579264 bytes"),
        (lambda: L.lasso_fista_solve_f64(p, 8, p, 12, none, 0, p, 12, 5, 8, 12, 0.3, nat.LR_AUTO, 1, 3, 0.0, 0, 0, 1.5, *tail),
         nat.LASSO_ERR_WORKSPACE, "workspace 16 < 183040 bytes"),
        (lambda: L.lasso_fista_solve(p, 2100, p, 2100, none, 0, p, 2100, 5, 2100, 2100, nat.LASSO_F32, 0.3, nat.LR_AUTO, 1, 3, 0.0,
                             0, 0, 1.5, *tail),
         nat.LASSO_ERR_UNSUPPORTED, "lr = LASSO_LR_AUTO: min(d,k) > 2048"),
        (lambda: L.lasso_fista_solve_f64(p, 2100, p, 2100, none, 0, p, 2100, 5, 2100, 2100, 0.3, nat.LR_AUTO, 1, 3, 0.0, 0, 0,
                                 1.5, *tail),
         nat.LASSO_ERR_UNSUPPORTED, "lr = LASSO_LR_AUTO: min(d,k) > 2048"),
    ]


def test_error_texts_come_back_through_last_error():
    from lasso_amd import _native as nat
    L = nat.lib()
    for call, status, text in _failures(nat, L):
        assert call() == status
        assert L.lasso_hip_last_error().decode() == text
