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
    ] + _layout_failures(nat, L)


def _layout_failures(nat, L):
    """include/lasso_hip.h's layout contract, the part that refuses: a leading dimension smaller than the row length, for
    every entry point that takes one, and the alignment rules of lasso_mstep_pipe_* (q: a base aligned to the element
    only).  n, d, k = 5, 8, 12; the pipelined M-step at d = 256, k = 512."""
    p, q, none, big = C.c_void_p(_P), C.c_void_p(_P + 4), None, 1 << 40
    F32, F64 = nat.LASSO_F32, nat.LASSO_F64
    n, d, k = 5, 8, 12
    tail = (none, none, none, none, none, none, p, big, none)
    o = nat.GpsrOptions()
    o.lambda_backtrack, o.maxiter = 0.5, 3
    r = nat.GpsrResult()
    cb = nat.ALLREDUCE_FN(lambda ctx, sums, count: 0)
    lam = C.c_double()
    small, row, small64 = "leading dimension too small", "leading dimension smaller than the row length", "bad argument"
    ab, abd, dd = ("[A | B] must be 16-byte aligned, pitch a multiple of 4",
                   "[A | B] and the dictionary must be 16-byte aligned, pitches multiples of 4",
                   "the dictionary must be 16-byte aligned, pitch a multiple of 4")
    zx = "Z and X must be 16-byte aligned, pitches multiples of 4"

    def solve(ldx, ldw, ldz0, ldz, lr=0.1):
        return lambda: L.lasso_fista_solve(p, ldx, p, ldw, p if ldz0 else none, ldz0, p, ldz, n, d, k, F32, 0.3, lr, 1, 3, 0.0, 0,
                                           0, 1.5, *tail)

    def solve64(ldx, ldw, ldz0, ldz):
        return lambda: L.lasso_fista_solve_f64(p, ldx, p, ldw, p if ldz0 else none, ldz0, p, ldz, n, d, k, 0.3, 0.1, 1, 3, 0.0,
                                               0, 0, 1.5, *tail)

    def run(ldx, ldz_in, ldy_in, ldz_out, ldy_out, dk=(d, k)):
        return lambda: L.lasso_fista_run(p, ldx, p, ldz_in, p if ldy_in else none, ldy_in, p, ldz_out, p if ldy_out else none,
                                         ldy_out, n, dk[0], dk[1], F32, 0.3, 0.1, 1, 0, 1, 3, 0, none, p, big, none)

    def sharded(ldx, ldw, ldz0, ldz):
        return lambda: L.lasso_fista_solve_sharded(p, ldx, p, ldw, p if ldz0 else none, ldz0, p, ldz, n, n, d, k, F32, 0.3, 0.1, 1,
                                                   3, 0.0, 1.5, cb, none, none, none, none, none, none, p, big, none)

    def objective(ldx, ldw, ldz):
        return lambda: L.lasso_objective(p, ldx, p, ldw, p, ldz, n, d, k, F32, 0.7, p, none, p, big, none)

    def cd_solve(ldx, ldw, ldz0, ldz):
        return lambda: L.lasso_cd_solve(p, ldx, p, ldw, p if ldz0 else none, ldz0, p, ldz, n, d, k, F32, 0.3, 5, 1e-6, none, none,
                                        p, big, none)

    def gpsr(ldx, ldw, ldz0, ldz):
        return lambda: L.lasso_gpsr_solve(p, ldx, p, ldw, p if ldz0 else none, ldz0, p, ldz, n, d, k, F32, 0.3, C.byref(o),
                                          C.byref(r), p, big, none)

    def pipe_gram(z, ldz, x, ldx, abp, ldab):
        return lambda: L.lasso_mstep_pipe_gram(z, ldz, x, ldx, 4096, 256, 512, F32, abp, ldab, 0, p, big, none)

    def pipe_rows(abp, ldab, dp, ldd):
        return lambda: L.lasso_mstep_pipe_rows(abp, ldab, dp, ldd, 4096, 256, 512, F32, 0, 1, p, big, none)

    def pipe_sweep(abp, ldab, dp, ldd):
        return lambda: L.lasso_mstep_pipe_sweep(abp, ldab, dp, ldd, 4096, 256, 512, F32, 1e-10, 0, p, p, big, none)

    bad = nat.LASSO_ERR_BAD_ARG
    return [(call, bad, text) for call, text in [
        # ---- leading dimension too small
        (solve(d - 1, k, 0, k), row), (solve(d, k - 1, 0, k), row), (solve(d, k, k - 1, k), row), (solve(d, k, 0, k - 1), row),
        (solve(d, k - 1, 0, k, nat.LR_AUTO), small64),
        (solve64(d - 1, k, 0, k), small), (solve64(d, k - 1, 0, k), small), (solve64(d, k, k - 1, k), small),
        (solve64(d, k, 0, k - 1), small),
        (sharded(d - 1, k, 0, k), small), (sharded(d, k - 1, 0, k), small), (sharded(d, k, k - 1, k), small),
        (sharded(d, k, 0, k - 1), small),
        (lambda: L.lasso_fista_prepare(p, k - 1, d, k, F32, 3, p, big, none), "ldw < k or maxiter < 0"),
        (run(d - 1, k, 0, k, 0), row), (run(d, k - 1, 0, k, 0), row), (run(d, k, k - 1, k, 0), row), (run(d, k, 0, k - 1, 0), row),
        (run(d, k, 0, k, k - 1), row),
        (run(299, 1100, 0, 1100, 0, (300, 1100)), row), (run(300, 1099, 0, 1100, 0, (300, 1100)), row),
        (run(300, 1100, 1099, 1100, 0, (300, 1100)), row), (run(300, 1100, 0, 1099, 0, (300, 1100)), row),
        (run(300, 1100, 0, 1100, 1099, (300, 1100)), row),
        (lambda: L.lasso_lipschitz(p, k - 1, d, k, F32, C.byref(lam), p, big, none), small64),
        (lambda: L.lasso_lipschitz(p, k - 1, d, k, F64, C.byref(lam), p, big, none), small64),
        (objective(d - 1, k, k), small), (objective(d, k - 1, k), small), (objective(d, k, k - 1), small),
        (lambda: L.lasso_objective_throttled(p, d, p, k - 1, p, k, n, d, k, F32, 0.7, p, none, 2, p, big, none), small),
        (lambda: L.lasso_objective(p, d, p, k, p, k - 1, n, d, k, F64, 0.7, p, none, p, big, none), small),
        (lambda: L.lasso_objective_f64(p, d - 1, p, k, p, k, n, d, k, 0.7, p, none, p, big, none), small),
        (lambda: L.lasso_gram_accumulate(p, k - 1, p, d, n, d, k, F32, p, p, none, 0, none), small64),
        (lambda: L.lasso_gram_accumulate(p, k, p, d - 1, n, d, k, F32, p, p, none, 0, none), small64),
        (lambda: L.lasso_gram_accumulate_signal(p, k, p, d - 1, n, d, k, F32, p, p, none, 0, p, 1, none), small64),
        (lambda: L.lasso_gram_accumulate_f64(p, k - 1, p, d, n, d, k, p, p, none, 0, none), small64),
        (lambda: L.lasso_gram_accumulate_f64(p, k, p, d - 1, n, d, k, p, p, none, 0, none), small64),
        (lambda: L.lasso_dict_sweep(p, p, p, k - 1, d, k, F32, 1e-10, 0, none, 0, 0, 0, p, none, p, big, none), small64),
        (lambda: L.lasso_dict_sweep(p, p, p, k, d, k, F32, 1e-10, 0, p, 2, d - 1, 0, p, none, p, big, none), "bad pool"),
        (lambda: L.lasso_dict_sweep_async(p, p, p, k - 1, d, k, F32, 1e-10, 0, none, 0, 0, 0, p, p, p, big, none), small64),
        (lambda: L.lasso_dict_sweep_async_to(p, p, p, k - 1, q, k, d, k, F32, 1e-10, 0, none, 0, 0, 0, p, p, none, 0, p, big,
                                             none), small64),
        (lambda: L.lasso_dict_sweep_async_to(p, p, p, k, C.c_void_p(_P + (1 << 20)), k - 1, d, k, F32, 1e-10, 0, none, 0, 0, 0, p,
                                             p, none, 0, p, big, none), small64),
        (lambda: L.lasso_dict_sweep_f64(p, p, p, k - 1, d, k, 1e-10, 0, p, none, p, big, none), small64),
        (lambda: L.lasso_dict_fill_degenerate(p, k - 1, d, k, F32, p, p, 2, d, 0, none), small64),
        (lambda: L.lasso_dict_fill_degenerate(p, k, d, k, F32, p, p, 2, d - 1, 0, none), small64),
        (lambda: L.lasso_dict_fill_degenerate_f64(p, k - 1, d, k, p, p, 2, d, 0, none), small64),
        (lambda: L.lasso_dict_fill_degenerate_f64(p, k, d, k, p, p, 2, d - 1, 0, none), small64),
        (lambda: L.lasso_zero_columns(p, k - 1, n, k, F32, p, none), small64),
        (lambda: L.lasso_zero_columns_f64(p, k - 1, n, k, p, none), small64),
        (lambda: L.lasso_ridge_solve(p, p, p, k - 1, d, k, F32, 0.1, none, p, big, none), small64),
        (lambda: L.lasso_ridge_solve_f64(p, p, p, k - 1, d, k, 0.1, none, p, big, none), small64),
        (lambda: L.lasso_init_transpose(n, d, k, F32, p, d - 1, p, k, p, k, p, big, none), small),
        (lambda: L.lasso_init_transpose(n, d, k, F32, p, d, p, k - 1, p, k, p, big, none), small),
        (lambda: L.lasso_init_transpose(n, d, k, F32, p, d, p, k, p, k - 1, p, big, none), small),
        (lambda: L.lasso_init_transpose(n, d, k, F64, p, d - 1, p, k, p, k, p, big, none), small),
        (lambda: L.lasso_cd_prepare(p, d - 1, p, k, none, 0, n, d, k, F32, p, big, none), small),
        (lambda: L.lasso_cd_prepare(p, d, p, k - 1, none, 0, n, d, k, F32, p, big, none), small),
        (lambda: L.lasso_cd_prepare(p, d, p, k, p, k - 1, n, d, k, F32, p, big, none), small),
        (lambda: L.lasso_cd_finish(p, k - 1, none, 0, n, d, k, 0.3, p, big, none), small),
        (lambda: L.lasso_cd_finish(p, k, p, k - 1, n, d, k, 0.3, p, big, none), small),
        (cd_solve(d - 1, k, 0, k), small), (cd_solve(d, k - 1, 0, k), small), (cd_solve(d, k, k - 1, k), small),
        (cd_solve(d, k, 0, k - 1), small),          # (refused before lasso_cd_prepare's launches, not by lasso_cd_finish)
        (gpsr(d - 1, k, 0, k), small), (gpsr(d, k - 1, 0, k), small), (gpsr(d, k, k - 1, k), small), (gpsr(d, k, 0, k - 1), small),
        (lambda: L.lasso_fista_backward(p, d - 1, p, k, p, p, n, d, k, F32, 0.1, 1, 3, p, p, p, p, big, none), small64),
        (lambda: L.lasso_fista_backward_steps(p, d, p, k - 1, p, p, n, d, k, F32, 0.1, none, 1, 3, p, p, p, p, big, none), small64),
        (lambda: L.lasso_patches_extract(p, p, 3 * 4 * 4 - 1, none, 2, 3, 8, 8, 4, 4, 2, 2, 1, none), small64),
        (lambda: L.lasso_patches_reconstruct(p, 3 * 4 * 4 - 1, none, p, 2, 3, 8, 8, 4, 4, 2, 2, none), small64),
        (pipe_gram(p, 511, p, 256, p, 768), small64), (pipe_gram(p, 512, p, 255, p, 768), small64),
        (pipe_gram(p, 512, p, 256, p, 767), small64),
        (pipe_rows(p, 767, p, 512), small64), (pipe_rows(p, 768, p, 511), small64),
        (pipe_sweep(p, 767, p, 512), small64), (pipe_sweep(p, 768, p, 511), small64),
        (lambda: L.lasso_mstep_pipe_finish(p, 511, 4096, 256, 512, F32, 1e-10, 0, p, none, 0, p, big, none), small64),
        # ---- lasso_mstep_pipe_*: 16-byte aligned bases, pitches multiples of 4 -- refused before the shape is looked at
        (pipe_gram(p, 512, p, 256, p, 771), ab), (pipe_gram(p, 512, p, 256, q, 772), ab),
        (pipe_gram(p, 515, p, 256, p, 768), zx), (pipe_gram(p, 512, p, 259, p, 768), zx),
        (pipe_gram(q, 516, p, 256, p, 768), zx), (pipe_gram(p, 512, q, 260, p, 768), zx),
        (pipe_rows(p, 771, p, 512), abd), (pipe_rows(q, 772, p, 512), abd), (pipe_rows(p, 768, p, 515), abd),
        (pipe_rows(p, 768, q, 516), abd),
        (pipe_sweep(p, 768, p, 515), dd), (pipe_sweep(p, 768, q, 516), dd),
    ]]


def test_error_texts_come_back_through_last_error():
    from lasso_amd import _native as nat
    L = nat.lib()
    for call, status, text in _failures(nat, L):
        assert call() == status
        assert L.lasso_hip_last_error().decode() == text
