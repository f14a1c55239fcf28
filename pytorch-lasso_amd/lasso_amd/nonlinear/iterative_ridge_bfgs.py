"""HIP-backed BFGS iterated ridge: the arguments, defaults, warnings and prints of ``lasso.nonlinear.iterative_ridge_bfgs``
(reference lasso/nonlinear/iterative_ridge_bfgs.py:45-140) on the kernels of csrc/irbfgs.hip, for the objective
``rss(x, weight)``."""
import ctypes as C
import warnings

import torch

from .. import _native as nat
from .owlqn import rss

_BRENT_MAXFUN = 500                                            # evaluations one bounded Brent search makes at most


def iterative_ridge_bfgs(f, x0, alpha=1.0, lr=1.0, xtol=1e-5, tikhonov=1e-4, eps=None, line_search=True, maxiter=None,
                         verbose=0, return_info=False):
    """A BFGS analogue of iterated ridge for min_z f(z) + alpha ||z||_1 with ``f = rss(x, weight)``: x0 [n,k] -> z [n,k]
    (a new tensor on the device of ``x0``; no input is modified).  Any other ``f`` raises NotImplementedError: only
    ``rss(x, weight)`` objectives run on the HIP path.

        z = iterative_ridge_bfgs(rss(x, weight), z0, alpha=0.5)
        # reference: iterative_ridge_bfgs(lambda z: 0.5 * (z @ weight.T - x).pow(2).sum(), z0, alpha=0.5)

    The arguments and defaults are the reference's (iterative_ridge_bfgs.py:46-48) plus ``return_info``: ``maxiter``
    defaults to ``5 k``, ``eps`` to ``finfo(float32).eps``.  Every row keeps its own BFGS Hessian estimate B [k,k]
    (the identity at the start); one step size, one objective and one stop test ``||x_new - x||_2 <= xtol`` (absolute)
    serve the whole batch.  Per iteration: coordinates with ``|x| < eps`` are frozen; the direction solves, per row,
    B with the frozen rows and columns zeroed plus ``diag(alpha / |x| + tikhonov)`` against ``grad + alpha sign(x)``
    (``lasso_amd.linear.utils.batch_cholesky_solve``'s kernels: if any row's Cholesky fails, the reference's
    'Cholesky factorization failed. Reverting to LU decomposition...' is warned once for that iteration and the whole
    batch is solved by LU); the step is the bounded-Brent minimiser on (0, 10) (``line_search=True``) or
    ``clamp(lr / ||grad||_1, max=lr)`` in iteration 1 and ``lr`` later; then every row's B takes the BFGS update
    (rows with ``|y.s| <= 1e-10`` keep theirs; the first update scales every B by ``rho (y.y)``).  No update follows
    the iteration that stops.  ``verbose`` prints the reference's lines (after the solve: the iterations run inside one
    native call).  A non-finite objective ends the solve (a warning).  ``return_info`` also returns ``dict(iterations,
    t, ls_iters, objective, delta_x, invalid_rows, lu, evaluations)``: per iteration the step, the Brent evaluations,
    the objective and ||dx||_2 of the new iterate, the rows whose update was invalid (-1: no update followed the
    iteration) and whether the LU route ran; ``evaluations`` lists the ``(iteration, t, f)`` the search evaluated.

    Deviations from the reference, all on purpose:
      * The objective, y.s, y.y, B s and s^T B s are folded in double and rounded once; Brent sees the un-rounded double
        of the quadratic form 0.5 (|r|^2 - 2 t <r,q> + t^2 |q|^2) + alpha |x - t d|_1 with q = d W^T.
      * The update computes rho (y_i y_j) and (Bs_i Bs_j) / (s^T B s) as symmetric functions of (i, j), so B is bitwise
        symmetric; the reference's ``baddbmm(B, rho * y, y^T)`` is not (only its LU route can see that).
      * The update behind the last iteration (``maxiter`` reached) is not computed: nothing reads it.
      * A Brent search that meets a non-finite objective ends there instead of walking to its evaluation limit.
    The workspace holds TWO [n,k,k] float32 arrays (B, as the reference, and the emitted systems): split a large batch.

    float32 tensors only, all of one dtype (anything else raises NotImplementedError naming the dtype); k <= 1024
    (beyond: NotImplementedError naming the cap).  Like the reference (``@torch.no_grad()``), inputs that require grad
    are accepted and the result carries no graph.  CPU tensors are staged through the device.  No CPU fallback."""
    assert x0.dim() == 2
    verbose = int(verbose)
    if not isinstance(f, rss):
        raise NotImplementedError("lasso_amd: only rss(x, weight) objectives run on the HIP path (got %s)"
                                  % type(f).__name__)
    x, weight = f.x, f.weight
    if not (torch.is_tensor(x) and torch.is_tensor(weight)) or x.dim() != 2 or weight.dim() != 2:
        raise RuntimeError("iterative_ridge_bfgs: rss(x, weight) expects 2-D tensors x [n,d] and weight [d,k]")
    d, k = weight.shape
    n = x.size(0)
    assert x.size(1) == d
    assert x0.shape == (n, k)
    for t in (weight, x, x0):
        if t.dtype != torch.float32:
            raise NotImplementedError("lasso_amd: iterative_ridge_bfgs is not implemented for %s tensors" % t.dtype)
    if k > nat.IRBFGS_MAX_K:
        raise NotImplementedError("lasso_amd: iterative_ridge_bfgs handles k <= %d (got k = %d)" % (nat.IRBFGS_MAX_K, k))
    if maxiter is None:
        maxiter = k * 5
    if eps is None:
        eps = torch.finfo(torch.float32).eps
    maxiter = int(maxiter)
    if maxiter < 0 or alpha < 0 or lr < 0 or xtol < 0 or tikhonov < 0 or eps < 0:
        raise ValueError("iterative_ridge_bfgs: maxiter, alpha, lr, xtol, tikhonov and eps must not be negative")
    info = dict(iterations=0, t=[], ls_iters=[], objective=[], delta_x=[], invalid_rows=[], lu=[], evaluations=[])
    if n == 0 or maxiter == 0:
        z = x0.detach().clone()
        return (z, info) if return_info else z
    nat.require_gpu()
    out_device = x0.device
    dev = nat.pick_device(x0, x, weight)
    xg = x.detach().to(device=dev).contiguous()
    wg = weight.detach().to(device=dev).contiguous()
    z0g = x0.detach().to(device=dev).contiguous()
    z = torch.empty((n, k), dtype=torch.float32, device=dev)
    cap = maxiter
    ecap = max(maxiter * _BRENT_MAXFUN, 1) if line_search else 1
    t_arr, f_arr, dx_arr = ((C.c_double * cap)() for _ in range(3))
    ls_arr, inv_arr, lu_arr = ((C.c_int32 * cap)() for _ in range(3))
    e_iter, e_t, e_f = (C.c_int32 * ecap)(), (C.c_double * ecap)(), (C.c_double * ecap)()
    trace = nat.IrbfgsTrace(cap, ecap, t_arr, ls_arr, f_arr, dx_arr, inv_arr, lu_arr, e_iter, e_t, e_f, 0)
    options = nat.IrbfgsOptions(maxiter, 1 if line_search else 0, float(lr), float(xtol), float(tikhonov), float(eps), 0)
    res = nat.IrbfgsResult()
    res.trace = C.pointer(trace)
    L = nat.lib()
    with torch.cuda.device(dev):
        ws = nat.workspace(dev, L.lasso_irbfgs_workspace_bytes(n, d, k, nat.LASSO_F32), "iterative_ridge_bfgs")
        status = L.lasso_irbfgs_solve(
            nat.ptr(xg), xg.stride(0) if n > 1 else d, nat.ptr(wg), wg.stride(0) if d > 1 else k,
            nat.ptr(z0g), k, nat.ptr(z), k, n, d, k, nat.LASSO_F32, float(alpha),
            C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
    nat.check(status)
    its = min(res.n_iter, cap)
    evs = min(trace.eval_count, ecap)
    info = dict(iterations=res.n_iter, t=list(t_arr[:its]), ls_iters=list(ls_arr[:its]), objective=list(f_arr[:its]),
                delta_x=list(dx_arr[:its]), invalid_rows=list(inv_arr[:its]), lu=[bool(v) for v in lu_arr[:its]],
                evaluations=[(e_iter[i], e_t[i], e_f[i]) for i in range(evs)])
    for _ in range(res.lu_count):
        warnings.warn('Cholesky factorization failed. Reverting to LU decomposition...')      # linear/utils.py:55
    if res.flags & nat.IRBFGS_NONFINITE:
        warnings.warn('iterative_ridge_bfgs: the objective is not finite; the solve ends with this iterate')
    if verbose:
        print('initial loss: %0.4f' % res.f0)                                       # :93
        if verbose > 1:
            for i in range(its):
                print('iter %3d - loss: %0.4f - dx: %0.4e' % (i + 1, f_arr[i], dx_arr[i]))   # :126
        print("         Current function value: %f" % res.f_final)                 # :137-138
        print("         Iterations: %d" % res.n_iter)
    z = z.to(device=out_device)
    return (z, info) if return_info else z
