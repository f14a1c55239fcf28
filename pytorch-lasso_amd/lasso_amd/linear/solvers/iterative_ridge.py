"""HIP-backed iterated ridge regression: the arguments, defaults, warning and prints of
``lasso.linear.solvers.iterative_ridge`` (reference iterative_ridge.py:11-141) on the kernels of csrc/iter_ridge.hip."""
import ctypes as C
import warnings

import torch

from ... import _native as nat

_MAX_K = 1024
_BRENT_MAXFUN = 500                                            # evaluations one bounded Brent search makes at most
# scipy.optimize's _status_message, which the reference prints
_STATUS = {nat.ITER_RIDGE_CONVERGED: ('converged', 'Optimization terminated successfully.'),
           nat.ITER_RIDGE_NAN: ('nan', 'NaN result encountered.'),
           nat.ITER_RIDGE_MAXITER: ('maxiter', 'Warning: Maximum number of iterations has been exceeded.')}


def iterative_ridge(z0, x, weight, alpha=1.0, tol=1e-5, tikhonov=1e-4, eps=None, maxiter=10, line_search=True, cg=False,
                    cg_options=None, verbose=False, return_info=False):
    """Iterated ridge regression (Schmidt 2005, section 2.5) for min_z 0.5 ||z W^T - x||^2 + alpha ||z||_1 over the
    whole batch.  z0 [n,k], x [n,d], weight [d,k] -> z [n,k] (a new tensor on the device of ``x``; no input is modified).

    The arguments, their order and defaults are the reference's (iterative_ridge.py:11-13) plus ``return_info``.  Each
    iteration solves, per row, ``(G[S,S] + diag(alpha / |z_S| + tikhonov)) z_S = (x W)_S`` on that row's support
    ``S = {j : |z_j| >= eps}`` (``eps`` defaults to the float32 machine epsilon); entries off the support keep their
    value.  The reference builds one masked k x k matrix per row and factors it at full size; the masked system and the
    compacted one have the same solution, and this path only ever factors the compacted one (its workspace is linear
    in n).  ``tol`` is scaled by ``z0.numel()``; the stop test ``sum |update| <= tol`` and the NaN test are one decision
    for the whole batch, once per iteration.  ``line_search=True`` minimises ``f(z + t (z_sol - z))`` over (0, 10) with
    scipy's bounded Brent method.  ``verbose`` prints the reference's lines (after the solve: the iterations run inside
    one native call).  ``return_info`` also returns ``dict(iterations, status, fval, update, t, ls_evals, support_max,
    support_mean, f0, evaluations)``: ``status`` is 'converged', 'nan' or 'maxiter'; per iteration the objective,
    sum |update|, the step, the Brent evaluations, and the largest and mean support of the new z; ``evaluations`` lists
    the ``(iteration, t, f)`` the search evaluated.

    Deviations from the reference, all on purpose:
      * The objective of a line-search trial is folded in double from three sums of the residual and of p W^T plus one
        pass over the code, and handed to Brent un-rounded; the reference rounds a float32 product of every trial.
        That rounding noise is what sends its own float32 and float64 runs to different steps.
      * A system that is not positive definite raises ``torch.linalg.LinAlgError`` naming the row and the leading
        minor.  The reference warns and falls back to a batched LU; this path has no LU.
      * ``tikhonov=0`` works here, because masked entries are not part of the system; the reference fails on it.
      * Hitting ``maxiter`` is reported in ``info['status']`` and printed under ``verbose``, as the reference does.

    Out of scope: ``cg=True`` raises NotImplementedError (the reference's inner conjugate gradient stops on a loose
    batch-wide tolerance and does not reproduce its own float64 codes); ``cg_options`` without ``cg`` is ignored, as in
    the reference.  Any non-float32 tensor and k > 1024 raise NotImplementedError.  There is no autograd (inputs that
    require grad are accepted, the result carries no graph), no ``algorithm='iter-ridge'`` arm of sparse_encode, and no
    row sharding over GPUs (the stop rule and the line search are batch-wide).  CPU tensors are staged through the
    device.  No CPU fallback."""
    if cg:
        raise NotImplementedError("lasso_amd: iterative_ridge is not implemented for cg=True (Cholesky only)")
    if x.dim() != 2 or weight.dim() != 2:
        raise RuntimeError("iterative_ridge expects 2-D x and weight")
    assert z0.dim() == 2
    d, k = weight.shape
    n = x.size(0)
    assert x.size(1) == d
    assert z0.shape == (n, k)
    for t in (weight, x, z0):
        if t.dtype != torch.float32:
            raise NotImplementedError("lasso_amd: iterative_ridge is not implemented for %s tensors" % t.dtype)
    if k > _MAX_K:
        raise NotImplementedError("lasso_amd: iterative_ridge is implemented for at most %d components (k = %d)"
                                  % (_MAX_K, k))
    maxiter = int(maxiter)
    if maxiter < 0 or alpha < 0 or tol < 0 or tikhonov < 0:
        raise ValueError("iterative_ridge: maxiter, alpha, tol and tikhonov must not be negative")
    if tikhonov < 1e-5:
        warnings.warn('small regularization value %0.4e may lead to '
                      'inprecise results.' % tikhonov)                       # iterative_ridge.py:53-55
    if eps is None:
        eps = torch.finfo(weight.dtype).eps
    nat.require_gpu()
    out_device = x.device
    dev = nat.pick_device(x, weight, z0)
    xg = x.detach().to(device=dev).contiguous()
    wg = weight.detach().to(device=dev).contiguous()
    z0g = z0.detach().to(device=dev).contiguous()
    z = torch.empty((n, k), dtype=torch.float32, device=dev)
    info = dict(iterations=0, status='maxiter' if maxiter == 0 or n == 0 else 'converged', fval=[], update=[], t=[],
                ls_evals=[], support_max=[], support_mean=[], f0=0.0, evaluations=[])
    if n > 0:
        cap = max(maxiter, 1)
        ecap = max(maxiter * _BRENT_MAXFUN, 1) if line_search else 1
        dbl, i32 = C.c_double * cap, C.c_int32 * cap
        f_arr, u_arr, t_arr, sm_arr = dbl(), dbl(), dbl(), dbl()
        ls_arr, sx_arr = i32(), i32()
        e_iter, e_t, e_f = (C.c_int32 * ecap)(), (C.c_double * ecap)(), (C.c_double * ecap)()
        trace = nat.IterRidgeTrace(cap, ecap, f_arr, u_arr, t_arr, ls_arr, sx_arr, sm_arr, e_iter, e_t, e_f, 0)
        options = nat.IterRidgeOptions(maxiter, 1 if line_search else 0, float(tol), float(tikhonov), float(eps), 0)
        res = nat.IterRidgeResult()
        res.trace = C.pointer(trace)
        L = nat.lib()
        with torch.cuda.device(dev):
            ws = nat.workspace(dev, L.lasso_iter_ridge_workspace_bytes(n, d, k, nat.LASSO_F32), "iter_ridge")
            status = L.lasso_iter_ridge_solve(
                nat.ptr(xg), xg.stride(0) if n > 1 else d, nat.ptr(wg), wg.stride(0) if d > 1 else k,
                nat.ptr(z0g), k, nat.ptr(z), k, n, d, k, nat.LASSO_F32, float(alpha),
                C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
        if status == nat.LASSO_ERR_BAD_ARG and res.bad_row >= 0:
            raise torch.linalg.LinAlgError(
                "iterative_ridge: the ridge system of row %d is not positive-definite (the leading minor of order %d of "
                "its support is not positive-definite, or not a number)." % (res.bad_row, res.bad_minor))
        nat.check(status)
        its = min(res.n_iter, cap)
        evs = min(trace.eval_count, ecap)
        name, msg = _STATUS[res.status]
        info = dict(iterations=res.n_iter, status=name, fval=list(f_arr[:its]), update=list(u_arr[:its]),
                    t=list(t_arr[:its]), ls_evals=list(ls_arr[:its]), support_max=list(sx_arr[:its]),
                    support_mean=list(sm_arr[:its]), f0=res.f0,
                    evaluations=[(e_iter[i], e_t[i], e_f[i]) for i in range(evs)])
        if verbose:
            print('initial fval: %0.4f' % res.f0)                                # :71
            for i in range(its):
                print('iter %3d - fval: %0.4f' % (i + 1, f_arr[i]))              # :121
            print(msg)                                                           # :137-139
            print("         Current function value: %f" % res.f_final)
            print("         Iterations: %d" % res.n_iter)
    else:
        z = z0g.clone()
    z = z.to(device=out_device)
    return (z, info) if return_info else z
