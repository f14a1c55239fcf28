"""HIP-backed interior-point lasso solver: the arguments, defaults, assertion and prints of
``lasso.linear.solvers.interior_point`` (reference interior_point.py:93-225) on the kernels of csrc/interior_point.hip."""
import ctypes as C

import torch

from ... import _native as nat

_MAX_D = 256
_MAX_K = 4096
# scipy's ReportBase with the reference's BasicReport columns (interior_point.py:11-14), written out
_WIDTHS = (7, 15, 12, 12, 10)
_HEADER = "|" + "|".join("{:^%d}" % wd for wd in _WIDTHS) + "|"
_ROW = "|{:^7}|{:^+15.4e}|{:^12.2e}|{:^12.2e}|{:^10.2e}|"


def interior_point(x, weight, z0=None, alpha=1.0, maxiter=20, barrier_init=0.1, tol=1e-2, eps=1e-5, verbose=False,
                   return_info=False):
    """Interior-point method (Schmidt 2005, section 2.3; Chen, Donoho and Saunders 2001) for
    min_z 0.5 ||z W^T - x||^2 + alpha ||z||_1 over the whole batch.  x [n,d], weight [d,k], z0 [n,k] -> (zf [n,k],
    success): zf is a new tensor on the device of ``x`` (no input is modified), success a Python bool.

    The arguments, their order and defaults are the reference's (interior_point.py:93-94) plus ``return_info``.  The
    code is split into non-negative halves z = z+ - z- with a log barrier of weight mu (``barrier_init`` at first).
    Each iteration forms the KKT residuals, solves per row the d x d system ``(I + W diag(c) W^T) dlambda = rhs`` with
    ``c = z+/s+ + z-/s-`` (1/s is taken as 0 where ``|s| < eps``), takes damped steps ``0.99 min(1, smallest ratio)``,
    shrinks mu and clamps z and s at 0.  The reference carries the dictionary twice, [W, -W], and builds an [n, 2k, d]
    intermediate and an [n, d, d] batch for that system; this path keeps one W and its workspace is linear in n.  The
    stop test is one decision for the whole batch: the means over rows of prim_feas, dual_feas and gap all ``< tol``.
    ``z0=None`` takes the ridge code.  The start must be interior (z > 0, s > 0, -alpha < lambda W < alpha); otherwise
    ``AssertionError``, as in the reference (an all-zero row of z0 is such a start).  ``verbose`` prints the reference's
    lines (after the solve: the iterations run inside one native call).  ``return_info`` also returns
    ``dict(iterations, obj0, obj, prim_feas, dual_feas, gap)`` with one entry per iteration.

    Bad data: a NaN in a row of ``x`` makes that row's codes NaN and leaves every other row as it is; a NaN mean never
    stops the loop, so ``maxiter`` iterations run and success is False.  A system whose pivot is not positive is not
    repaired: that row's codes are NaN.

    Out of scope: any non-float32 tensor, ``d > 256`` and ``k > 4096`` raise NotImplementedError, and so do inputs that
    require grad under grad mode (there is no autograd).  There is no ``algorithm='interior-point'`` arm of
    sparse_encode and no row sharding over GPUs (the stop rule is a batch mean).  CPU tensors are staged through the
    device.  No CPU fallback."""
    assert torch.is_tensor(x) and x.dim() == 2
    assert torch.is_tensor(weight) and weight.dim() == 2
    n, d = x.shape
    if z0 is not None:
        assert torch.is_tensor(z0) and z0.dim() == 2
        n1, k = z0.shape
        assert n1 == n
        assert weight.shape == (d, k)
    else:
        d1, k = weight.shape
        assert d1 == d
    for t in (x, weight, z0):
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError("lasso_amd: interior_point is not implemented for %s tensors" % t.dtype)
    if d > _MAX_D:
        raise NotImplementedError("lasso_amd: interior_point is implemented for an input size of at most %d (d = %d)"
                                  % (_MAX_D, d))
    if k > _MAX_K:
        raise NotImplementedError("lasso_amd: interior_point is implemented for at most %d components (k = %d)"
                                  % (_MAX_K, k))
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, z0)):
        raise NotImplementedError("lasso_amd: interior_point has no autograd; detach the inputs or use torch.no_grad()")
    maxiter = int(maxiter)
    if maxiter < 0:
        raise ValueError("interior_point: maxiter must not be negative")
    info = dict(iterations=0, obj0=0.0, obj=[], prim_feas=[], dual_feas=[], gap=[])
    if n == 0:
        z = x.new_zeros((0, k))
        return (z, False, info) if return_info else (z, False)
    nat.require_gpu()
    out_device = x.device
    dev = nat.pick_device(x, weight) if z0 is None else nat.pick_device(x, weight, z0)
    xg = x.detach().to(device=dev).contiguous()
    wg = weight.detach().to(device=dev).contiguous()
    if z0 is None:
        from ..sparse_encode import _ridge_init
        z0g = _ridge_init(xg, wg, alpha)                     # the reference's ridge(x.T, weight, alpha).T
    else:
        z0g = z0.detach()
    z0g = z0g.to(device=dev).contiguous()
    z = torch.empty((n, k), dtype=torch.float32, device=dev)
    cap = max(maxiter, 1)
    dbl = C.c_double * cap
    obj, prim, dual, gap = dbl(), dbl(), dbl(), dbl()
    trace = nat.InteriorPointTrace(cap, 0, obj, prim, dual, gap)
    options = nat.InteriorPointOptions(maxiter, 0, float(barrier_init), float(tol), float(eps), 0)
    res = nat.InteriorPointResult()
    res.trace = C.pointer(trace)
    L = nat.lib()
    with torch.cuda.device(dev):
        ws = nat.workspace(dev, L.lasso_interior_point_workspace_bytes(n, d, k, nat.LASSO_F32), "interior_point")
        status = L.lasso_interior_point_solve(
            nat.ptr(xg), xg.stride(0) if n > 1 else d, nat.ptr(wg), wg.stride(0) if d > 1 else k,
            nat.ptr(z0g), k, nat.ptr(z), k, n, d, k, nat.LASSO_F32, float(alpha),
            C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
    if status == nat.LASSO_ERR_BAD_ARG and res.status == nat.INTERIOR_POINT_BAD_START:
        # interior_point.py:65-67
        raise AssertionError("interior_point: the start is not interior (z > 0, s > 0, -alpha < lambda W < alpha)")
    nat.check(status)
    its = min(res.n_iter, cap)
    success = res.status == nat.INTERIOR_POINT_CONVERGED
    info = dict(iterations=res.n_iter, obj0=res.obj0, obj=list(obj[:its]), prim_feas=list(prim[:its]),
                dual_feas=list(dual[:its]), gap=list(gap[:its]))
    if verbose:
        print('initial obj func: %0.4e\n' % res.obj0)                        # :146
        print(_HEADER.format("niter", "obj func", "prim feas", "dual feas", "gap"))
        print(_HEADER.format(*('-' * wd for wd in _WIDTHS)))
        for i in range(its):
            print(_ROW.format(i + 1, obj[i], prim[i], dual[i], gap[i]))    # :216
    z = z.to(device=out_device)
    return (z, success, info) if return_info else (z, success)
