"""HIP-backed orthant-wise Newton: the arguments, defaults, warnings and prints of
``lasso.linear.solvers.orthant_wise_newton`` (reference orthant_wise_newton.py:33-160) on the kernels of csrc/own.hip."""
import ctypes as C
import warnings

import torch

from ... import _native as nat

_LINE_SEARCHES = {'brent': nat.OWN_BRENT, 'backtrack': nat.OWN_BACKTRACK, 'none': nat.OWN_NONE}
_LS_DEFAULTS = dict(tol=0.1, decay=0.95, maxiter=500)          # backtracking(), orthant_wise_newton.py:20
_BRENT_MAXFUN = 500                                            # evaluations one bounded Brent search makes at most
_MAX_K = 4096


def orthant_wise_newton(weight, x, z0, alpha=1., lr=1., maxiter=20, xtol=1e-5, line_search='brent', ls_options=None,
                        verbose=0, return_info=False):
    """Orthant-wise Newton for min_z 0.5 ||z W^T - x||^2 + alpha ||z||_1 over the whole batch, with the explicit
    Hessian W^T W + 1e-4 I.  weight [d,k], x [n,d], z0 [n,k] -> z [n,k] (a new tensor on the device of ``x``; no
    input is modified).

    The arguments and defaults are the reference's (orthant_wise_newton.py:33-35) plus ``return_info``.
    ``line_search``: 'brent' (bounded Brent on (0, 10)), 'backtrack' (``ls_options``: tol 0.1, decay 0.95, maxiter
    500; any other key raises TypeError) or 'none' (t = lr); anything else raises ValueError.  Every line search is
    one decision for the whole batch.  ``verbose`` prints the reference's lines (after the solve: the iterations run
    inside one native call), and 'line search did not converge.' is warned once per iteration whose backtracking ran
    out of trials.  ``return_info`` also returns ``dict(iterations, t, ls_iters, objective, delta_z, evaluations)``:
    per iteration the step, the number of line-search evaluations, the objective and ||dz||_2 of the new z, and the
    list of ``(iteration, t, f)`` the search evaluated.

    Deviations from the reference, both on purpose:
      * ``Hinv = (W^T W + 1e-4 I)^-1`` is computed in double (the library's float64 Gram and Cholesky) and rounded
        once to float32; the reference factors in float32.
      * The objective of a line-search trial is folded in double and handed to Brent un-rounded; the reference rounds
        it to float32 first, and that rounding noise is what sends its own float32 and float64 runs to different
        steps.  (The backtracking test keeps the reference's float32 operation order.)
    For k > d the Hessian equals the 1e-4 shift on a (k - d)-dimensional subspace, its condition number is of the
    order of 1e4 ||W||^2, and neither this path nor the reference reproduces its own float64 codes there: the
    objectives agree (to about 1e-5 relative), the codes do not.  After several Brent iterations the same holds for
    every shape: codes of two correct float32 implementations differ by 0.1 and more while their objectives agree.

    bfloat16 / float16 tensors are computed in float32 on their exact up-conversions and rounded once at the end;
    float64 tensors and k > 4096 raise NotImplementedError.  Like the reference (``@torch.no_grad()``), inputs that
    require grad are accepted and the result carries no graph.  A Hessian that is not positive definite raises
    ``torch.linalg.LinAlgError``.  A non-finite objective ends the solve with the last accepted z (a warning).
    CPU tensors are staged through the device.  No CPU fallback."""
    assert z0.dim() == 2
    verbose = int(verbose)
    if ls_options is None:
        ls_options = {}
    if line_search not in _LINE_SEARCHES:
        raise ValueError("line_search must be one of {'brent', 'backtrack', 'none'}.")
    for name in ls_options:
        if name not in _LS_DEFAULTS:
            raise TypeError("backtracking() got an unexpected keyword argument '%s'" % name)
    ls = dict(_LS_DEFAULTS, **ls_options)
    if x.dim() != 2 or weight.dim() != 2:
        raise RuntimeError("orthant_wise_newton expects 2-D x and weight")
    d, k = weight.shape
    n = x.size(0)
    assert x.size(1) == d
    assert z0.shape == (n, k)
    for t in (weight, x, z0):
        if t.dtype == torch.float64:
            raise NotImplementedError("lasso_amd: orthant_wise_newton is not implemented for torch.float64 tensors")
        if t.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise NotImplementedError("lasso_amd: orthant_wise_newton is not implemented for %s tensors" % t.dtype)
    if k > _MAX_K:
        raise NotImplementedError("lasso_amd: orthant_wise_newton is implemented for at most %d components (k = %d)"
                                  % (_MAX_K, k))
    maxiter = int(maxiter)
    if maxiter < 0 or int(ls['maxiter']) < 1 or alpha < 0:
        raise ValueError("orthant_wise_newton: maxiter >= 0, ls_options['maxiter'] >= 1 and alpha >= 0 are required")
    nat.require_gpu()
    out_device, out_dtype = x.device, x.dtype
    dev = nat.pick_device(x, weight, z0)
    xg = x.detach().to(device=dev, dtype=torch.float32).contiguous()
    wg = weight.detach().to(device=dev, dtype=torch.float32).contiguous()
    z0g = z0.detach().to(device=dev, dtype=torch.float32).contiguous()
    z = torch.empty((n, k), dtype=torch.float32, device=dev)
    info = dict(iterations=0, t=[], ls_iters=[], objective=[], delta_z=[], evaluations=[])
    if n > 0:
        mode = _LINE_SEARCHES[line_search]
        cap = max(maxiter, 1)
        per_iter = {nat.OWN_BRENT: _BRENT_MAXFUN, nat.OWN_BACKTRACK: int(ls['maxiter']), nat.OWN_NONE: 0}[mode]
        ecap = max(maxiter * per_iter, 1)
        t_arr, f_arr, dz_arr = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
        ls_arr = (C.c_int32 * cap)()
        e_iter, e_t, e_f = (C.c_int32 * ecap)(), (C.c_double * ecap)(), (C.c_double * ecap)()
        trace = nat.OwnTrace(cap, ecap, t_arr, ls_arr, f_arr, dz_arr, e_iter, e_t, e_f, 0)
        options = nat.OwnOptions(maxiter, mode, int(ls['maxiter']), 0, float(lr), float(xtol), float(ls['tol']),
                                 float(ls['decay']))
        res = nat.OwnResult()
        res.trace = C.pointer(trace)
        L = nat.lib()
        with torch.cuda.device(dev):
            ws = nat.workspace(dev, L.lasso_own_workspace_bytes(n, d, k, nat.LASSO_F32), "own")
            status = L.lasso_own_solve(
                nat.ptr(xg), xg.stride(0) if n > 1 else d, nat.ptr(wg), wg.stride(0) if d > 1 else k,
                nat.ptr(z0g), k, nat.ptr(z), k, n, d, k, nat.LASSO_F32, float(alpha),
                C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
        if status == nat.LASSO_ERR_BAD_ARG and res.cholesky_info != 0:
            raise torch.linalg.LinAlgError(
                "linalg.cholesky: The factorization could not be completed because the input is not positive-definite "
                "(the leading minor of order %d is not positive-definite)." % res.cholesky_info)
        nat.check(status)
        its = min(res.n_iter, cap)
        evs = min(trace.eval_count, ecap)
        info = dict(iterations=res.n_iter, t=list(t_arr[:its]), ls_iters=list(ls_arr[:its]), objective=list(f_arr[:its]),
                    delta_z=list(dz_arr[:its]), evaluations=[(e_iter[i], e_t[i], e_f[i]) for i in range(evs)])
        for _ in range(res.ls_failures):
            warnings.warn('line search did not converge.')                    # orthant_wise_newton.py:27
        if res.flags & nat.OWN_NONFINITE:
            warnings.warn('orthant_wise_newton: the objective is not finite; returning the last accepted iterate')
        if verbose:
            print('initial f: %0.4f' % res.f0)                                   # :93
            if verbose > 1:
                for i in range(its):
                    print('iter %3d - ls_iters: %3d - f: %0.4f - dz: %0.3e' % (i + 1, ls_arr[i], f_arr[i], dz_arr[i]))
            print("         Current function value: %f" % res.f_final)           # :157-158
            print("         Iterations: %d" % res.n_iter)
    else:
        z = z0g.clone()
    z = z.to(device=out_device, dtype=out_dtype)
    return (z, info) if return_info else z
