"""ctypes binding of liblasso_hip.so (the C ABI of include/lasso_hip.h).

This is the binding a maintainer of the reference would add next to
lasso/linear/solvers/ista.py; see INTEGRATION.md.  The library is built in-tree
by ``__graft_entry__.build()`` / ``make -C pytorch-lasso_amd/csrc``.
"""
import collections
import ctypes as C
import os
import threading
import warnings

import torch

LASSO_OK, LASSO_ERR_BAD_ARG, LASSO_ERR_UNSUPPORTED = 0, 1, 2
LASSO_ERR_WORKSPACE, LASSO_ERR_HIP, LASSO_WARN_LINESEARCH = 3, 4, 5
LASSO_PENDING, LASSO_WARN_ABORTED, LASSO_PENDING_MAPPED, LASSO_PENDING_DEFERRED = 6, 7, 8, 9
LASSO_F32, LASSO_BF16, LASSO_F64 = 0, 1, 2
STOP_GLOBAL, STOP_NONE, STOP_GLOBAL_CHUNKED = 0, 1, 2
ABI_VERSION = 7
KERNEL_AUTO, KERNEL_TILE, KERNEL_SPLITK = 0, 0x100, 0x200
SOLVE_ASYNC = 0x4000
SOLVE_ONE_CHUNK = 0x10000
SOLVE_SHARDED = 0x8000
SOLVE_STATUS_MAPPED = 0x20000       # iters_out = four words of pinned (device-writable) host memory
SOLVE_DEFER_VERDICT = 0x40000       # the verdict's launch is left to lasso_fista_solve_verdict_deferred (another stream)
LR_AUTO = -1.0
GPSR_ZERO_SOLUTION, GPSR_TAU_FACTOR_CHANGED, GPSR_LINESEARCH_FAILED = 1, 2, 4
GPSR_DEBIAS_NO_NONZEROS, GPSR_DEBIAS_TOO_MANY = 8, 16
OWN_BRENT, OWN_BACKTRACK, OWN_NONE = 0, 1, 2
OWN_LS_NOT_CONVERGED, OWN_NONFINITE = 1, 2
OWLQN_MAX_PAIRS = 1535                                                # most pairs lasso_owlqn_solve holds
GLM_BERNOULLI = 1                                                     # lasso_owlqn_glm_solve's family
ACT_IDENTITY, ACT_SIGMOID, ACT_TANH, ACT_RELU = 0, 1, 2, 3               # LASSO_ACT_*: lasso_ista_nl_solve's activation
IRBFGS_CONVERGED, IRBFGS_NONFINITE = 1, 2
IRBFGS_MAX_K = 1024                                                   # lasso_batch_solve_tier_cap(LASSO_F32, general)
IRBFGS_TIME_ROWS = 2                                                  # bit 1 of lasso_irbfgs_options.reserved
ITER_RIDGE_CONVERGED, ITER_RIDGE_NAN, ITER_RIDGE_MAXITER = 0, 1, 2
INTERIOR_POINT_CONVERGED, INTERIOR_POINT_MAXITER, INTERIOR_POINT_BAD_START = 0, 1, 2
CG_ABS_TOL, CG_REL_TOL, CG_CURV_CONVERGED, CG_CURV_NEGATIVE, CG_MAXITER = 0, 1, 2, 3, 4
CG_FORMS = ('fused', 'unfused', 'conv-implicit', 'conv-patches')      # LASSO_CG_FORM_*
LIP_STATUS = ('converged', 'breakdown', 'maxiter', 'nonfinite')         # LASSO_LIP_*
LIP_SPACES = ('image', 'code')                                        # LASSO_LIP_SPACE_*
CG_PLAIN_FORM = 1                                                     # bit 0 of lasso_cg_options.reserved
FORCE_BLOCKS_128 = 8                                                  # LASSO_FORCE_BLOCKS_128, a bit of options.reserved

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class NativeError(RuntimeError):
    """The HIP extension is missing, or a native call failed."""


_LIB_PATH = os.path.join(_HERE, "liblasso_hip.so")


def lib_path():
    return _LIB_PATH


class GpsrOptions(C.Structure):
    """lasso_gpsr_options (include/lasso_hip.h)"""
    _fields_ = [(name, C.c_int32) for name in ('stop_criterion', 'maxiter', 'miniter', 'init', 'continuation', 'debias',
                                               'cont_steps', 'maxiter_debias', 'miniter_debias', 'reserved')] + \
               [(name, C.c_double) for name in ('tol', 'mu', 'lambda_backtrack', 'first_tau_factor', 'tol_debias')]


class GpsrTrace(C.Structure):
    """lasso_gpsr_trace: host arrays of the caller"""
    _pf, _pi = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    _fields_ = [('capacity', C.c_int32), ('lambda_', _pf), ('lambda0', _pf), ('trials', _pi), ('objective', _pf),
                ('criterion', _pf), ('nz', _pi), ('step_capacity', C.c_int32), ('step_tau', C.POINTER(C.c_double)),
                ('step_f0', _pf), ('step_nz0', _pi), ('step_end', _pi), ('db_capacity', C.c_int32), ('db_rr', _pf),
                ('db_conv', _pf)]


class GpsrResult(C.Structure):
    """lasso_gpsr_result"""
    _fields_ = [('n_iter', C.c_int32), ('flags', C.c_int32), ('steps', C.c_int32), ('db_iters', C.c_int32),
                ('objective', C.c_double), ('main_objective', C.c_double), ('main_rr', C.c_float), ('main_l1', C.c_float),
                ('main_nz', C.c_int32), ('db_rr', C.c_float), ('db_l1', C.c_float), ('db_nz', C.c_int32),
                ('trace', C.POINTER(GpsrTrace))]


class OwnOptions(C.Structure):
    """lasso_own_options"""
    _fields_ = [(name, C.c_int32) for name in ('maxiter', 'line_search', 'ls_maxiter', 'reserved')] + \
               [(name, C.c_double) for name in ('lr', 'xtol', 'ls_tol', 'ls_decay')]


class OwnTrace(C.Structure):
    """lasso_own_trace: host arrays of the caller"""
    _pd, _pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _fields_ = [('capacity', C.c_int32), ('eval_capacity', C.c_int32), ('t', _pd), ('ls_iters', _pi), ('f', _pd),
                ('delta_z', _pd), ('eval_iter', _pi), ('eval_t', _pd), ('eval_f', _pd), ('eval_count', C.c_int64)]


class OwnResult(C.Structure):
    """lasso_own_result"""
    _fields_ = [('n_iter', C.c_int32), ('flags', C.c_int32), ('f0', C.c_double), ('f_final', C.c_double),
                ('cholesky_info', C.c_int32), ('ls_failures', C.c_int32), ('trace', C.POINTER(OwnTrace))]


class OwlqnOptions(C.Structure):
    """lasso_owlqn_options"""
    _fields_ = [(name, C.c_int32) for name in ('maxiter', 'line_search', 'ls_maxiter', 'history_size')] + \
               [(name, C.c_double) for name in ('lr', 'xtol', 'ls_tol', 'ls_decay')] + [('reserved', C.c_int64)]


class OwlqnTrace(C.Structure):
    """lasso_owlqn_trace: host arrays of the caller"""
    _pd, _pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _fields_ = [('capacity', C.c_int32), ('eval_capacity', C.c_int32), ('t', _pd), ('ls_iters', _pi), ('f', _pd),
                ('delta_x', _pd), ('pairs', _pi), ('skipped', _pi), ('h_diag', _pd), ('eval_iter', _pi), ('eval_t', _pd),
                ('eval_f', _pd), ('eval_count', C.c_int64)]


class OwlqnResult(C.Structure):
    """lasso_owlqn_result"""
    _fields_ = [('n_iter', C.c_int32), ('flags', C.c_int32), ('f0', C.c_double), ('f_final', C.c_double),
                ('ls_failures', C.c_int32), ('reserved', C.c_int32), ('trace', C.POINTER(OwlqnTrace)),
                ('direction_ms', C.c_double), ('direction_bytes', C.c_double)]


class IstaNlOptions(C.Structure):
    """lasso_ista_nl_options"""
    _fields_ = [(name, C.c_int32) for name in ('maxiter', 'fast', 'lr_auto', 'power_iters')] + \
               [('lr', C.c_double), ('tol', C.c_double), ('reserved', C.c_int64)]


class IstaNlTrace(C.Structure):
    """lasso_ista_nl_trace: host arrays of the caller"""
    _fields_ = [('capacity', C.c_int32), ('loss', C.c_int32), ('deltas', C.POINTER(C.c_double)), ('f', C.POINTER(C.c_double))]


class IstaNlResult(C.Structure):
    """lasso_ista_nl_result"""
    _fields_ = [('n_iter', C.c_int32), ('stopped', C.c_int32), ('last_delta', C.c_double), ('f0', C.c_double),
                ('f_final', C.c_double), ('l_dev', C.c_void_p)]


class IrbfgsOptions(C.Structure):
    """lasso_irbfgs_options"""
    _fields_ = [('maxiter', C.c_int32), ('line_search', C.c_int32), ('lr', C.c_double), ('xtol', C.c_double),
                ('tikhonov', C.c_double), ('eps', C.c_double), ('reserved', C.c_int64)]


class IrbfgsTrace(C.Structure):
    """lasso_irbfgs_trace: host arrays of the caller"""
    _pd, _pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _fields_ = [('capacity', C.c_int32), ('eval_capacity', C.c_int32), ('t', _pd), ('ls_iters', _pi), ('f', _pd),
                ('delta_x', _pd), ('invalid_rows', _pi), ('lu', _pi), ('eval_iter', _pi), ('eval_t', _pd),
                ('eval_f', _pd), ('eval_count', C.c_int64)]


class IrbfgsResult(C.Structure):
    """lasso_irbfgs_result"""
    _fields_ = [('n_iter', C.c_int32), ('flags', C.c_int32), ('f0', C.c_double), ('f_final', C.c_double),
                ('lu_count', C.c_int32), ('reserved', C.c_int32), ('bad_row', C.c_int64),
                ('trace', C.POINTER(IrbfgsTrace)), ('row_ms', C.c_double), ('row_bytes', C.c_double),
                ('solve_ms', C.c_double)]


class IterRidgeOptions(C.Structure):
    """lasso_iter_ridge_options"""
    _fields_ = [('maxiter', C.c_int32), ('line_search', C.c_int32), ('tol', C.c_double), ('tikhonov', C.c_double),
                ('eps', C.c_double), ('reserved', C.c_int64)]


class IterRidgeTrace(C.Structure):
    """lasso_iter_ridge_trace: host arrays of the caller"""
    _pd, _pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _fields_ = [('capacity', C.c_int32), ('eval_capacity', C.c_int32), ('f', _pd), ('update', _pd), ('t', _pd),
                ('ls_evals', _pi), ('support_max', _pi), ('support_mean', _pd), ('eval_iter', _pi), ('eval_t', _pd),
                ('eval_f', _pd), ('eval_count', C.c_int64)]


class IterRidgeResult(C.Structure):
    """lasso_iter_ridge_result"""
    _fields_ = [('n_iter', C.c_int32), ('status', C.c_int32), ('f0', C.c_double), ('f_final', C.c_double),
                ('bad_row', C.c_int64), ('bad_minor', C.c_int32), ('pad_', C.c_int32),
                ('trace', C.POINTER(IterRidgeTrace))]


class InteriorPointOptions(C.Structure):
    """lasso_interior_point_options"""
    _fields_ = [('maxiter', C.c_int32), ('pad_', C.c_int32), ('barrier_init', C.c_double), ('tol', C.c_double),
                ('eps', C.c_double), ('reserved', C.c_int64)]


class InteriorPointTrace(C.Structure):
    """lasso_interior_point_trace: host arrays of the caller"""
    _pd = C.POINTER(C.c_double)
    _fields_ = [('capacity', C.c_int32), ('pad_', C.c_int32), ('obj', _pd), ('prim_feas', _pd), ('dual_feas', _pd),
                ('gap', _pd)]


class InteriorPointResult(C.Structure):
    """lasso_interior_point_result"""
    _fields_ = [('n_iter', C.c_int32), ('status', C.c_int32), ('obj0', C.c_double),
                ('trace', C.POINTER(InteriorPointTrace))]


class SplitBregmanOptions(C.Structure):
    """lasso_split_bregman_options"""
    _fields_ = [(name, C.c_int32) for name in ('maxiter', 'niter_inner', 'reserved', 'pad_')] + \
               [(name, C.c_double) for name in ('lambd', 'tol', 'tau')]


class SplitBregmanTrace(C.Structure):
    """lasso_split_bregman_trace: host arrays of the caller"""
    _fields_ = [('capacity', C.c_int32), ('pad_', C.c_int32), ('update', C.POINTER(C.c_double)),
                ('cost', C.POINTER(C.c_double))]


class SplitBregmanResult(C.Structure):
    """lasso_split_bregman_result"""
    _fields_ = [('n_iter', C.c_int32), ('itn', C.c_int32), ('stopped', C.c_int32), ('cholesky_info', C.c_int32),
                ('trace', C.POINTER(SplitBregmanTrace))]


class CgOptions(C.Structure):
    """lasso_cg_options"""
    _fields_ = [('maxiter', C.c_int32), ('reserved', C.c_int32), ('tol', C.c_double), ('rtol', C.c_double),
                ('tik', C.c_double)]


class CgTrace(C.Structure):
    """lasso_cg_trace: host arrays of the caller"""
    _pd = C.POINTER(C.c_double)
    _fields_ = [('capacity', C.c_int32), ('pad_', C.c_int32), ('r_abs', _pd), ('curv_sum', _pd), ('rs', _pd)]


class CgResult(C.Structure):
    """lasso_cg_result"""
    _fields_ = [('n_iter', C.c_int32), ('status', C.c_int32), ('host_reads', C.c_int32), ('form', C.c_int32),
                ('termcond', C.c_double), ('trace', C.POINTER(CgTrace))]


class ConvLipOptions(C.Structure):
    """lasso_conv_lip_options"""
    _fields_ = [('maxiter', C.c_int32), ('reserved', C.c_int32), ('tol', C.c_double)]


class ConvLipResult(C.Structure):
    """lasso_conv_lip_result; history: a host array of the caller"""
    _fields_ = [('theta', C.c_double), ('residual', C.c_double), ('dim', C.c_int64), ('steps', C.c_int32),
                ('matvecs', C.c_int32), ('host_reads', C.c_int32), ('space', C.c_int32), ('status', C.c_int32),
                ('restarts', C.c_int32), ('history_capacity', C.c_int32), ('pad_', C.c_int32),
                ('history', C.POINTER(C.c_double))]


# int (*lasso_allreduce_fn)(void* ctx, double* sums, int count)   (include/lasso_hip.h)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int)


def stop_budget(numel, tol):
    """ista.py:64,93: ``z0.numel() * tol`` rounded once to float32 (stop_budget<float>, csrc/stoprule_host.hpp)"""
    return C.c_float(float(numel) * tol).value


def use_library(path):
    """Bind a different build of the library (A/B builds of the kernels under tools/); must be
    called before the first native call."""
    global _LIB_PATH, _LIB
    _LIB_PATH, _LIB = path, None


def _declare(lib):
    i64, i32, dbl, vp, sz = C.c_int64, C.c_int, C.c_double, C.c_void_p, C.c_size_t
    lib.lasso_hip_abi_version.restype = i32
    lib.lasso_hip_status_string.restype = C.c_char_p
    lib.lasso_hip_status_string.argtypes = [i32]
    lib.lasso_hip_last_error.restype = C.c_char_p
    lib.lasso_hip_device_cus.argtypes = [C.POINTER(i32)]
    lib.lasso_debug_force_standby.restype = i32
    lib.lasso_debug_force_standby.argtypes = [i32]
    lib.lasso_fista_workspace_bytes.restype = sz
    lib.lasso_fista_workspace_bytes.argtypes = [i64, i64, i64, i32, i32, dbl, i32, i32]
    lib.lasso_fista_kernel_name.restype = C.c_char_p
    lib.lasso_fista_kernel_name.argtypes = [i64, i64, i64, i32, i32]
    lib.lasso_fista_solve.restype = i32
    lib.lasso_fista_solve.argtypes = [
        vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32,
        dbl, dbl, i32, i32, dbl, i32, i32, dbl, C.POINTER(C.c_int32), C.POINTER(C.c_float),
        C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
        vp, sz, vp]
    pdbl = C.POINTER(dbl)
    lib.lasso_fista_solve_f64.restype = i32
    lib.lasso_fista_solve_f64.argtypes = [
        vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64,
        dbl, dbl, i32, i32, dbl, i32, i32, dbl, C.POINTER(C.c_int32), pdbl,
        C.POINTER(C.c_int32), pdbl, pdbl, pdbl, vp, sz, vp]
    lib.lasso_objective_f64_workspace_bytes.restype = sz
    lib.lasso_objective_f64_workspace_bytes.argtypes = [i64, i64, i64]
    lib.lasso_objective_f64.restype = i32
    lib.lasso_objective_f64.argtypes = [vp, i64, vp, i64, vp, i64, i64, i64, i64, dbl, vp, vp, vp, sz, vp]
    lib.lasso_fista_prepare.restype = i32
    lib.lasso_fista_prepare.argtypes = [vp, i64, i64, i64, i32, i32, vp, sz, vp]
    lib.lasso_fista_run.restype = i32
    lib.lasso_fista_run.argtypes = [
        vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32,
        dbl, dbl, i32, i32, i32, i32, i32, vp, vp, sz, vp]
    lib.lasso_lipschitz_workspace_bytes.restype = sz
    lib.lasso_lipschitz_workspace_bytes.argtypes = [i64, i64]
    lib.lasso_lipschitz.restype = i32
    lib.lasso_lipschitz.argtypes = [vp, i64, i64, i64, i32, C.POINTER(dbl), vp, sz, vp]
    lib.lasso_objective_workspace_bytes.restype = sz
    lib.lasso_objective_workspace_bytes.argtypes = [i64, i64, i64]
    lib.lasso_objective.restype = i32
    lib.lasso_objective.argtypes = [vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, dbl, vp, vp,
                                    vp, sz, vp]
    lib.lasso_objective_throttled.restype = i32
    lib.lasso_objective_throttled.argtypes = [vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, dbl, vp, vp, i32,
                                              vp, sz, vp]
    lib.lasso_gram_accumulate.restype = i32
    lib.lasso_gram_workspace_bytes.restype = sz
    lib.lasso_gram_workspace_bytes.argtypes = [i64, i64, i64]
    lib.lasso_gram_accumulate.argtypes = [vp, i64, vp, i64, i64, i64, i64, i32, vp, vp, vp, sz, vp]
    lib.lasso_gram_accumulate_signal.argtypes = [vp, i64, vp, i64, i64, i64, i64, i32, vp, vp, vp, sz, vp, i32, vp]
    lib.lasso_fista_solve_verdict_deferred.restype = i32
    lib.lasso_fista_solve_verdict_deferred.argtypes = [vp, vp, vp, i32, vp]
    lib.lasso_mstep_pipe_head_word.restype = vp
    lib.lasso_mstep_pipe_head_word.argtypes = [i64, i64, i64, vp, sz]
    lib.lasso_dict_sweep_workspace_bytes.restype = sz
    lib.lasso_dict_sweep_workspace_bytes.argtypes = [i64, i64]
    lib.lasso_dict_sweep.restype = i32
    lib.lasso_dict_sweep.argtypes = [vp, vp, vp, i64, i64, i64, i32, dbl, i32, vp, i64, i64,
                                     C.c_uint64, vp, C.POINTER(C.c_int32), vp, sz, vp]
    lib.lasso_dict_sweep_async.restype = i32
    lib.lasso_dict_sweep_async.argtypes = [vp, vp, vp, i64, i64, i64, i32, dbl, i32, vp, i64, i64,
                                           C.c_uint64, vp, vp, vp, sz, vp]
    lib.lasso_dict_sweep_async_to.restype = i32
    lib.lasso_dict_sweep_async_to.argtypes = [vp, vp, vp, i64, vp, i64, i64, i64, i32, dbl, i32, vp, i64, i64,
                                              C.c_uint64, vp, vp, vp, i32, vp, sz, vp]
    lib.lasso_stream_wait_word.restype = i32
    lib.lasso_stream_wait_word.argtypes = [vp, i32, i32, vp]
    lib.lasso_mstep_pipe_stages.restype = i32
    lib.lasso_mstep_pipe_stages.argtypes = [i64, i64, i64]
    lib.lasso_mstep_pipe_stage_rows.restype = i32
    lib.lasso_mstep_pipe_stage_rows.argtypes = [i64, i64, i64, i32, C.POINTER(i64), C.POINTER(i64)]
    lib.lasso_mstep_pipe_workspace_bytes.restype = sz
    lib.lasso_mstep_pipe_workspace_bytes.argtypes = [i64, i64, i64]
    lib.lasso_mstep_pipe_gram.restype = i32
    lib.lasso_mstep_pipe_gram.argtypes = [vp, i64, vp, i64, i64, i64, i64, i32, vp, i64, i32, vp, sz, vp]
    lib.lasso_mstep_pipe_wait.restype = i32
    lib.lasso_mstep_pipe_wait.argtypes = [i64, i64, i64, i32, vp, sz, vp]
    lib.lasso_mstep_pipe_rows.restype = i32
    lib.lasso_mstep_pipe_rows.argtypes = [vp, i64, vp, i64, i64, i64, i64, i32, i32, i32, vp, sz, vp]
    lib.lasso_mstep_pipe_sweep.restype = i32
    lib.lasso_mstep_pipe_sweep.argtypes = [vp, i64, vp, i64, i64, i64, i64, i32, dbl, i32, vp, vp, sz, vp]
    lib.lasso_mstep_pipe_finish.restype = i32
    lib.lasso_mstep_pipe_finish.argtypes = [vp, i64, i64, i64, i64, i32, dbl, i32, vp, vp, i32, vp, sz, vp]
    lib.lasso_mstep_pipe_signal.restype = i32
    lib.lasso_mstep_pipe_signal.argtypes = [i64, i64, i64, i32, vp, sz, vp]
    lib.lasso_fista_solve_verdict_mapped.restype = i32
    lib.lasso_fista_solve_verdict_mapped.argtypes = [i64, i64, i64, i64, i32, i32, dbl, vp, vp, vp, sz, vp]
    lib.lasso_dict_sweep_count.restype = vp
    lib.lasso_dict_sweep_count.argtypes = [i64, i64, vp, sz]
    lib.lasso_fista_solve_sharded.restype = i32
    lib.lasso_fista_solve_sharded.argtypes = [
        vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i64, i32, dbl, dbl, i32, i32, dbl, dbl,
        ALLREDUCE_FN, vp, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_float),
        C.POINTER(C.c_float), vp, sz, vp]
    lib.lasso_fista_solve_collect.restype = i32
    lib.lasso_fista_solve_collect.argtypes = [i64, i64, i64, i32, i32, dbl, vp, vp, sz, vp]
    lib.lasso_fista_solve_deltas.restype = vp
    lib.lasso_fista_solve_deltas.argtypes = [i64, i64, i64, i32, i32, dbl, vp, sz]
    lib.lasso_fista_solve_verdict.restype = i32
    lib.lasso_fista_solve_verdict.argtypes = [i64, i64, i64, i64, i32, i32, dbl, vp, vp, sz, vp]
    lib.lasso_fista_solve_finish.restype = i32
    lib.lasso_fista_solve_finish.argtypes = [i64, i64, i64, i32, i32, dbl, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                             vp, sz, vp]
    lib.lasso_init_transpose_workspace_bytes.restype = sz
    lib.lasso_init_transpose_workspace_bytes.argtypes = [i64, i64]
    lib.lasso_init_transpose.restype = i32
    lib.lasso_init_transpose.argtypes = [i64, i64, i64, i32, vp, i64, vp, i64, vp, i64, vp, sz, vp]
    lib.lasso_ridge_workspace_bytes.restype = sz
    lib.lasso_ridge_workspace_bytes.argtypes = [i64, i64]
    lib.lasso_ridge_solve.restype = i32
    lib.lasso_ridge_solve.argtypes = [vp, vp, vp, i64, i64, i64, i32, dbl, C.POINTER(C.c_int32), vp, sz, vp]
    lib.lasso_dict_fill_degenerate.restype = i32
    lib.lasso_dict_fill_degenerate.argtypes = [vp, i64, i64, i64, i32, vp, vp, i64, i64, i32, vp]
    lib.lasso_zero_columns.restype = i32
    lib.lasso_zero_columns.argtypes = [vp, i64, i64, i64, i32, vp, vp]
    pi32 = C.POINTER(C.c_int32)
    # float64 M-step: double matrices, no dtype argument
    lib.lasso_gram_f64_workspace_bytes.restype = sz
    lib.lasso_gram_f64_workspace_bytes.argtypes = [i64, i64, i64]
    lib.lasso_gram_accumulate_f64.restype = i32
    lib.lasso_gram_accumulate_f64.argtypes = [vp, i64, vp, i64, i64, i64, i64, vp, vp, vp, sz, vp]
    lib.lasso_dict_sweep_f64_workspace_bytes.restype = sz
    lib.lasso_dict_sweep_f64_workspace_bytes.argtypes = [i64, i64]
    lib.lasso_dict_sweep_f64.restype = i32
    lib.lasso_dict_sweep_f64.argtypes = [vp, vp, vp, i64, i64, i64, dbl, i32, vp, pi32, vp, sz, vp]
    lib.lasso_dict_fill_degenerate_f64.restype = i32
    lib.lasso_dict_fill_degenerate_f64.argtypes = [vp, i64, i64, i64, vp, vp, i64, i64, i32, vp]
    lib.lasso_zero_columns_f64.restype = i32
    lib.lasso_zero_columns_f64.argtypes = [vp, i64, i64, i64, vp, vp]
    lib.lasso_ridge_f64_workspace_bytes.restype = sz
    lib.lasso_ridge_f64_workspace_bytes.argtypes = [i64, i64]
    lib.lasso_ridge_solve_f64.restype = i32
    lib.lasso_ridge_solve_f64.argtypes = [vp, vp, vp, i64, i64, i64, dbl, pi32, vp, sz, vp]
    lib.lasso_cd_workspace_bytes.restype = sz
    lib.lasso_cd_workspace_bytes.argtypes = [i64, i64, i64, i32]
    lib.lasso_cd_prepare.restype = i32
    lib.lasso_cd_prepare.argtypes = [vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, vp, sz, vp]
    lib.lasso_cd_run.restype = i32
    lib.lasso_cd_run.argtypes = [i64, i64, i64, dbl, dbl, i32, pi32, pi32, vp, sz, vp]
    lib.lasso_cd_finish.restype = i32
    lib.lasso_cd_finish.argtypes = [vp, i64, vp, i64, i64, i64, i64, dbl, vp, sz, vp]
    geom = [i64, i64, i64, i64, i64, i64, i64, i32, i32, i32, i32, i32, i32]
    lib.lasso_conv_ista_workspace_bytes.restype = sz
    lib.lasso_conv_ista_workspace_bytes.argtypes = geom
    lib.lasso_conv_ista_kernel_name.restype = C.c_char_p
    lib.lasso_conv_ista_kernel_name.argtypes = geom
    lib.lasso_conv_ista_solve.restype = i32
    lib.lasso_conv_ista_solve.argtypes = [vp, vp, vp, vp] + geom + [i32, dbl, dbl, i32, i32, dbl, pi32,
                                                                    C.POINTER(C.c_float), vp, sz, vp]
    lib.lasso_conv_objective.restype = i32
    lib.lasso_conv_objective.argtypes = [vp, vp, vp] + geom + [i32, dbl, vp, vp, sz, vp]
    lib.lasso_conv_ista_trace_bytes.restype = sz
    lib.lasso_conv_ista_trace_bytes.argtypes = geom + [i32]
    lib.lasso_conv_ista_run_traced.restype = i32
    lib.lasso_conv_ista_run_traced.argtypes = [vp, vp, vp, vp] + geom + [i32, dbl, dbl, i32, i32, vp, vp, sz, vp]
    lib.lasso_conv_ista_backward_workspace_bytes.restype = sz
    lib.lasso_conv_ista_backward_workspace_bytes.argtypes = geom
    lib.lasso_conv_ista_backward.restype = i32
    lib.lasso_conv_ista_backward.argtypes = [vp, vp, vp, vp] + geom + [i32, dbl, i32, i32, vp, vp, vp, vp, sz, vp]
    lib.lasso_conv_lip_workspace_bytes.restype = sz
    lib.lasso_conv_lip_workspace_bytes.argtypes = [i64, i64, i32, i32]
    lib.lasso_conv_lip_bound.restype = i32
    lib.lasso_conv_lip_bound.argtypes = [vp, i64, i64, i32, i32, i32, i32, C.POINTER(dbl), vp, sz, vp]
    # float64 forms of the convolutional entry points (csrc/conv_f64.hip)
    lib.lasso_conv_ista_workspace_bytes_f64.restype = sz
    lib.lasso_conv_ista_workspace_bytes_f64.argtypes = geom
    lib.lasso_conv_ista_trace_bytes_f64.restype = sz
    lib.lasso_conv_ista_trace_bytes_f64.argtypes = geom + [i32]
    lib.lasso_conv_ista_backward_workspace_bytes_f64.restype = sz
    lib.lasso_conv_ista_backward_workspace_bytes_f64.argtypes = geom
    lib.lasso_conv_lip_workspace_bytes_f64.restype = sz
    lib.lasso_conv_lip_workspace_bytes_f64.argtypes = [i64, i64, i32, i32]
    lib.lasso_conv_ista_solve_f64.restype = i32
    lib.lasso_conv_ista_solve_f64.argtypes = [vp, vp, vp, vp] + geom + [dbl, dbl, i32, i32, dbl, pi32, pdbl, vp, sz, vp]
    lib.lasso_conv_objective_f64.restype = i32
    lib.lasso_conv_objective_f64.argtypes = [vp, vp, vp] + geom + [dbl, vp, vp, sz, vp]
    lib.lasso_conv_lip_bound_f64.restype = i32
    lib.lasso_conv_lip_bound_f64.argtypes = [vp, i64, i64, i32, i32, i32, i32, pdbl, vp, sz, vp]
    lib.lasso_fista_backward_workspace_bytes.restype = sz
    lib.lasso_fista_backward_workspace_bytes.argtypes = [i64, i64, i64]
    lib.lasso_fista_backward.restype = i32
    lib.lasso_fista_backward.argtypes = [vp, i64, vp, i64, vp, vp, i64, i64, i64, i32, dbl, i32, i32,
                                         vp, vp, vp, vp, sz, vp]
    lib.lasso_fista_backward_steps.restype = i32
    lib.lasso_fista_backward_steps.argtypes = [vp, i64, vp, i64, vp, vp, i64, i64, i64, i32, dbl, C.POINTER(C.c_float),
                                               i32, i32, vp, vp, vp, vp, sz, vp]
    lib.lasso_patches_extract.restype = i32
    lib.lasso_patches_extract.argtypes = [vp, vp, i64, vp, i64, i64, i64, i64, i32, i32, i32, i32, i32, vp]
    lib.lasso_patches_reconstruct.restype = i32
    lib.lasso_patches_reconstruct.argtypes = [vp, i64, vp, vp, i64, i64, i64, i64, i32, i32, i32, i32, vp]
    lib.lasso_gpsr_workspace_bytes.restype = sz
    lib.lasso_gpsr_workspace_bytes.argtypes = [i64, i64, i64, i32]
    lib.lasso_gpsr_solve.restype = i32
    lib.lasso_gpsr_solve.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, dbl,
                                     C.POINTER(GpsrOptions), C.POINTER(GpsrResult), vp, sz, vp]
    lib.lasso_conv_gpsr_workspace_bytes.restype = sz
    lib.lasso_conv_gpsr_workspace_bytes.argtypes = [i64] * 7 + [i32] * 6
    lib.lasso_conv_gpsr_form.restype = C.c_char_p
    lib.lasso_conv_gpsr_form.argtypes = [i64] * 7 + [i32] * 7
    lib.lasso_conv_gpsr_solve.restype = i32
    lib.lasso_conv_gpsr_solve.argtypes = [vp, vp, vp, vp] + [i64] * 7 + [i32] * 6 + [i32, dbl, C.POINTER(GpsrOptions),
                                                                                  C.POINTER(GpsrResult), vp, sz, vp]
    lib.lasso_own_workspace_bytes.restype = sz
    lib.lasso_own_workspace_bytes.argtypes = [i64, i64, i64, i32]
    lib.lasso_own_solve.restype = i32
    lib.lasso_own_solve.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, dbl,
                                    C.POINTER(OwnOptions), C.POINTER(OwnResult), vp, sz, vp]
    lib.lasso_owlqn_workspace_bytes.restype = sz
    lib.lasso_owlqn_workspace_bytes.argtypes = [i64, i64, i64, i32, i64]
    lib.lasso_owlqn_solve.restype = i32
    lib.lasso_owlqn_solve.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, dbl,
                                      C.POINTER(OwlqnOptions), C.POINTER(OwlqnResult), vp, sz, vp]
    lib.lasso_owlqn_glm_solve.restype = i32
    lib.lasso_owlqn_glm_solve.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, dbl, i32,
                                          C.POINTER(OwlqnOptions), C.POINTER(OwlqnResult), vp, sz, vp]
    lib.lasso_ista_nl_workspace_bytes.restype = sz
    lib.lasso_ista_nl_workspace_bytes.argtypes = [i64, i64, i64, i32, i32]
    lib.lasso_ista_nl_solve.restype = i32
    lib.lasso_ista_nl_solve.argtypes = [vp, i64, vp, i64, vp, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, dbl, i32,
                                        C.POINTER(IstaNlOptions), C.POINTER(IstaNlResult), C.POINTER(IstaNlTrace), vp, sz, vp]
    lib.lasso_irbfgs_workspace_bytes.restype = sz
    lib.lasso_irbfgs_workspace_bytes.argtypes = [i64, i64, i64, i32]
    lib.lasso_irbfgs_solve.restype = i32
    lib.lasso_irbfgs_solve.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, dbl,
                                       C.POINTER(IrbfgsOptions), C.POINTER(IrbfgsResult), vp, sz, vp]
    lib.lasso_irbfgs_update.restype = i32
    lib.lasso_irbfgs_update.argtypes = [vp] * 8 + [i64, i64, i32, dbl, dbl, dbl, i32, i32, i32, vp]
    lib.lasso_iter_ridge_workspace_bytes.restype = sz
    lib.lasso_iter_ridge_workspace_bytes.argtypes = [i64, i64, i64, i32]
    lib.lasso_iter_ridge_solve.restype = i32
    lib.lasso_iter_ridge_solve.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, dbl,
                                           C.POINTER(IterRidgeOptions), C.POINTER(IterRidgeResult), vp, sz, vp]
    lib.lasso_iter_ridge_rows.restype = i32
    lib.lasso_iter_ridge_rows.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i32, dbl, dbl, dbl,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, sz, vp]
    lib.lasso_split_bregman_workspace_bytes.restype = sz
    lib.lasso_split_bregman_workspace_bytes.argtypes = [i64, i64, i64, i32]
    lib.lasso_split_bregman_solve.restype = i32
    lib.lasso_split_bregman_solve.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, dbl,
                                              C.POINTER(SplitBregmanOptions), C.POINTER(SplitBregmanResult), vp, sz, vp]
    lib.lasso_interior_point_workspace_bytes.restype = sz
    lib.lasso_interior_point_workspace_bytes.argtypes = [i64, i64, i64, i32]
    lib.lasso_interior_point_solve.restype = i32
    lib.lasso_interior_point_solve.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, dbl,
                                               C.POINTER(InteriorPointOptions), C.POINTER(InteriorPointResult), vp, sz, vp]
    lib.lasso_interior_point_rows.restype = i32
    lib.lasso_interior_point_rows.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, vp]
    lib.lasso_cg_workspace_bytes.restype = sz
    lib.lasso_cg_workspace_bytes.argtypes = [i64, i64, i32]
    lib.lasso_cg_solve.restype = i32
    lib.lasso_cg_solve.argtypes = [vp, i64, vp, i64, vp, i64, i64, i64, i32, C.POINTER(CgOptions), C.POINTER(CgResult),
                                   vp, sz, vp]
    lib.lasso_conv_cg_workspace_bytes.restype = sz
    lib.lasso_conv_cg_workspace_bytes.argtypes = [i64] * 7 + [i32] * 6
    lib.lasso_conv_cg_solve.restype = i32
    lib.lasso_conv_cg_solve.argtypes = [vp, vp, vp] + [i64] * 7 + [i32] * 6 + [i32, C.POINTER(CgOptions),
                                                                             C.POINTER(CgResult), vp, sz, vp]
    lib.lasso_conv_lip_constant_workspace_bytes.restype = sz
    lib.lasso_conv_lip_constant_workspace_bytes.argtypes = [i64, i64, i32, i32, i64, i64] + [i32] * 7
    lib.lasso_conv_lip_constant.restype = i32
    lib.lasso_conv_lip_constant.argtypes = [vp, i64, i64, i32, i32, i64, i64] + [i32] * 6 + [
        C.POINTER(ConvLipOptions), C.POINTER(ConvLipResult), vp, sz, vp]
    lib.lasso_batch_solve_tier_cap.restype = i32
    lib.lasso_batch_solve_tier_cap.argtypes = [i32, i32]
    lib.lasso_solver_block_side.restype = i32
    lib.lasso_solver_block_side.argtypes = [i64, i64, i64]
    lib.lasso_batch_solve_workgroups.restype = i32
    lib.lasso_batch_solve_workgroups.argtypes = [i64, i64, i32]
    lib.lasso_batch_solve_workspace_bytes.restype = sz
    lib.lasso_batch_solve_workspace_bytes.argtypes = [i64, i64, i32]
    for fn in (lib.lasso_batch_chol_solve, lib.lasso_batch_lu_solve):     # result: lasso_batch_solve_result*
        fn.restype = i32
        fn.argtypes = [vp, i64, i64, vp, i64, vp, i64, i64, i64, i32, vp, vp, sz, vp]
    lib.lasso_cd_solve.restype = i32
    lib.lasso_cd_solve.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i64, i64, i32, dbl, i32,
                                   dbl, pi32, pi32, vp, sz, vp]
    lib.lasso_cd_mod_workspace_bytes.restype = sz
    lib.lasso_cd_mod_workspace_bytes.argtypes = [i64, i64, i64, i32]
    lib.lasso_cd_mod_solve.restype = i32
    lib.lasso_cd_mod_solve.argtypes = [vp, i64, vp, i64, vp, i64, i32, vp, vp, vp, i64, i64, i64, i32, dbl, i32,
                                       dbl, pi32, C.POINTER(C.c_int64), vp, sz, vp]


def lib():
    """Load the shared library; fail loudly if it is not built."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise NativeError(
                "lasso_amd: %s is missing -- build it with `python -c 'import "
                "__graft_entry__ as g; g.build()'` (there is no CPU fallback)" % path)
        try:
            handle = C.CDLL(path)
        except OSError as e:  # pragma: no cover
            raise NativeError("lasso_amd: cannot load %s: %s" % (path, e))
        _declare(handle)
        if handle.lasso_hip_abi_version() != ABI_VERSION:
            raise NativeError("lasso_amd: ABI version mismatch")
        _LIB = handle
    return _LIB


def check(status):
    if status == LASSO_OK:
        return
    L = lib()
    msg = "%s: %s" % (L.lasso_hip_status_string(status).decode(),
                      L.lasso_hip_last_error().decode())
    if status == LASSO_WARN_LINESEARCH:
        warnings.warn("backtracking line search failed. Reverting to initial step size")
        return
    if status == LASSO_ERR_BAD_ARG:
        raise ValueError(msg)
    if status == LASSO_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise NativeError(msg)


def require_gpu():
    if not torch.cuda.is_available():
        raise NativeError("lasso_amd: no HIP device visible (torch.cuda.is_available() is "
                          "False); this package has no CPU fallback")


DT = {torch.float32: LASSO_F32, torch.bfloat16: LASSO_BF16, torch.float64: LASSO_F64}


def one_dtype(what, *tensors):
    """True: every tensor is float64 (the double entry points); False: none is.  A mix raises before any launch
    (the reference's matmul raises there too).  None entries are ignored."""
    f64 = [t.dtype == torch.float64 for t in tensors if t is not None]
    if any(f64) and not all(f64):
        raise RuntimeError("%s: expected tensors of one dtype, got %s"
                           % (what, ", ".join(str(t.dtype) for t in tensors if t is not None)))
    return bool(f64) and all(f64)


def pick_device(*tensors):
    """The device a call runs on: that of the first tensor on a HIP device, else the current HIP device (tensors that
    live on the CPU are staged through it)."""
    for t in tensors:
        if t is not None and t.is_cuda:
            return t.device
    return torch.device('cuda', torch.cuda.current_device())


def stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class HostWords:
    """A few int32 words of pinned (device-writable) host memory whose LAST word a kernel sets to 1, released, after it
    has written the others (LASSO_SOLVE_STATUS_MAPPED, lasso_dict_sweep_async, lasso_mstep_pipe_finish).  ``arm()``
    zeroes that word before the launch; ``wait()`` polls it -- the result needs neither a copy launch nor an event
    record behind the kernel (an event record between two kernels of a stream costs ~5 us on that stream)."""

    def __init__(self, count):
        self.tensor = torch.zeros(count, dtype=torch.int32).pin_memory()
        self.view = self.tensor.numpy()              # shares the pinned pages

    def arm(self):
        self.view[-1] = 0
        return self.tensor.data_ptr()

    def ready(self):
        return self.view[-1] != 0

    def wait(self, timeout=120.0):
        import time
        view, spins, t0 = self.view, 0, None
        while view[-1] == 0:
            spins += 1
            if (spins & 0x3FFF) == 0:
                now = time.monotonic()
                if t0 is None:
                    t0 = now
                elif now - t0 > timeout:
                    raise NativeError("lasso_amd: no result from the GPU after %.0f s (kernel fault or hang)" % timeout)
        return view


_WS = collections.OrderedDict()       # key -> buffer, least recently used first
_WS_LOCK = threading.Lock()
_WS_MAX_ENTRIES = 64                   # (device, stream, thread, purpose) combinations kept
_WS_MAX_BYTES = 8 << 30                # ... and their total size; beyond either the oldest entries go


def _ws_evict(keep):
    total = sum(b.numel() for b in _WS.values())
    while len(_WS) > 1 and (len(_WS) > _WS_MAX_ENTRIES or total > _WS_MAX_BYTES):
        key = next(iter(_WS))
        if key == keep:                 # never the buffer being handed out
            _WS.move_to_end(key)
            key = next(iter(_WS))
            if key == keep:
                break
        total -= _WS.pop(key).numel()


def workspace(device, nbytes, tag='fista'):
    """A cached device scratch buffer (caller-owned memory of the C ABI).  One buffer per
    (device, HIP stream, host thread, purpose): calls enqueued on one stream are ordered, so
    they may share scratch; different streams or threads never do (the C library itself is
    re-entrant -- all state lives in the workspace the caller passes).  The cache is bounded
    (least recently used entries are dropped beyond `_WS_MAX_ENTRIES` keys or `_WS_MAX_BYTES`
    bytes): thread pools with churn or code that creates many streams do not pin one workspace
    set each for ever.  A dropped buffer goes back to torch's caching allocator, which keeps
    it alive for the kernels already enqueued on its stream."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream,
           threading.get_ident(), tag)
    with _WS_LOCK:
        buf = _WS.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
            _WS[key] = buf
        _WS.move_to_end(key)
        _ws_evict(key)
    return buf


def release_workspaces():
    """Drop every cached scratch buffer (e.g. after a one-off large problem)."""
    with _WS_LOCK:
        _WS.clear()
