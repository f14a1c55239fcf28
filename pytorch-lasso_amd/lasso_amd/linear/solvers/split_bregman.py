"""HIP-backed Split Bregman: the arguments, defaults and prints of ``lasso.linear.solvers.split_bregman`` (reference
split_bregman.py:5-86) on the kernels of csrc/split_bregman.hip."""
import ctypes as C
import math

import torch

from ... import _native as nat

_MAX_K = 4096


def split_bregman(A, y, x0=None, alpha=1.0, lambd=1.0, maxiter=20, niter_inner=5, tol=1e-10, tau=1., verbose=False,
                  return_info=False):
    """Split Bregman for min_x 0.5 ||x A^T - y||^2 + alpha ||x||_1 over the whole batch.  A [d,k], y [n,d], x0 [n,k] or
    None (zeros) -> ``(x, itn)``: x [n,k] float32, a new tensor on the device of ``y`` (no input is modified), and the
    outer iteration number upon termination.

    The arguments, their order and defaults are the reference's (split_bregman.py:5-6) plus ``return_info``.  The
    algorithm is the reference's on row-major [n,k] state: once per solve ``H = A^T A / alpha + lambd I``,
    ``Hinv = H^-1``, ``Aty = (y A) / alpha``, ``B = D = 0``; every outer iteration saves ``Xold = X``, runs
    ``niter_inner`` times ``X = (Aty + lambd (D - B)) Hinv^T; D = softshrink(X + B, 1 / lambd)``, then
    ``B += tau (X - D)`` and ``update = ||X - Xold||_F``.  The loop breaks at the top of an iteration once
    ``update <= tol``; ``update`` starts at +inf, so the first iteration always runs.

    Behaviour, decision by decision:
      * ``itn`` is the reference's: the index of the iteration at whose top the stop fired, which equals the number of
        outer iterations executed; ``maxiter - 1`` if the stop never fired.  ``return_info`` also returns
        ``dict(iterations, stopped, update)``: the outer iterations executed, whether the stop fired, and the executed
        iterations' ``update`` values as doubles; under ``verbose`` also ``cost``, the list of their costs.
      * The returned ``x`` is the linear solve's ``X``, not the shrunk ``D``: it is dense and in general has no exact
        zeros.  That is the reference's behaviour (:84).
      * ``x0`` only enters through ``Xold`` of the first iteration (the first inner iteration overwrites ``X`` from
        ``Aty`` alone): two solves that differ only in ``x0`` return bitwise the same ``x`` unless
        ``tol >= ||X_1 - x0||``; only ``update[0]`` differs.
      * ``maxiter < 1`` raises ValueError (the reference fails with UnboundLocalError at 0: it has no value there);
        ``niter_inner < 1`` raises ValueError (a deliberate narrowing: the reference tolerates 0, where nothing is ever
        solved); ``alpha <= 0``, ``lambd <= 0`` or a NaN among ``alpha``, ``lambd``, ``tau``, ``tol`` raises ValueError.
      * ``tol < 0`` is legal and means "never stop": a norm is never <= a negative number.  Such a solve makes no host
        read until it finishes (one per 1024 outer iterations beyond that many).
      * ``verbose`` prints the reference's line ``'iter %3d - cost: %0.4f'`` per executed outer iteration (:80-82),
        after the solve from the trace (the iterations run inside one native call); the cost is
        ``0.5 |X A^T - y|^2 + alpha |X|_1`` folded in double.
      * A failed factorisation of ``H`` (possible only with a non-finite ``A``) raises ``torch.linalg.LinAlgError``, the
        type the reference's ``torch.linalg.cholesky`` raises.
      * A NaN or Inf in ``y`` is an ordinary operand: that row of ``x`` comes back non-finite, ``update`` is NaN, the stop
        never fires (``NaN <= tol`` is false) and ``maxiter`` iterations run, without a warning; the other rows come back
        bitwise as they do for a batch of the same shape without the bad value.
      * Deviation on purpose: ``Hinv`` is computed in double (the library's float64 Gram and Cholesky) and rounded once
        to float32; the reference factors in float32.  ``update`` and the cost are folded in double in a fixed order:
        two solves of the same arguments are bitwise equal.
      * Refusals, all before any native call: any non-float32 tensor raises NotImplementedError naming the dtype;
        ``k > 4096`` raises NotImplementedError; an input that requires grad under grad mode raises
        NotImplementedError ("requires_grad"); shape mismatches are the reference's asserts.

    Out of scope: the ``algorithm='split-bregman'`` arm of sparse_encode (it keeps raising NotImplementedError) and
    dict_learning with it; float64, bfloat16 and float16 tensors; autograd; ``k > 4096``; row sharding over GPUs (the
    stop rule is batch-wide); a Woodbury form for d < k (two n x k x d products instead of one n x k x k product, but
    another rounding against the reference).  CPU tensors are staged through the device.  No CPU fallback."""
    assert y.dim() == 2
    assert A.dim() == 2
    assert y.shape[1] == A.shape[0]
    d, k = A.shape
    n = y.shape[0]
    if x0 is not None:
        assert x0.shape == (n, k)
    tensors = [t for t in (A, y, x0) if t is not None]
    for t in tensors:
        if t.dtype != torch.float32:
            raise NotImplementedError("lasso_amd: split_bregman is not implemented for %s tensors" % t.dtype)
    if k > _MAX_K:
        raise NotImplementedError("lasso_amd: split_bregman is implemented for at most %d components (k = %d)"
                                  % (_MAX_K, k))
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise NotImplementedError("lasso_amd: split_bregman does not build an autograd graph; inputs that "
                                  "require grad (requires_grad=True) are not supported -- detach them")
    maxiter, niter_inner = int(maxiter), int(niter_inner)
    alpha, lambd, tau, tol = float(alpha), float(lambd), float(tau), float(tol)
    if maxiter < 1 or niter_inner < 1:
        raise ValueError("split_bregman: maxiter >= 1 and niter_inner >= 1 are required")
    if any(math.isnan(v) for v in (alpha, lambd, tau, tol)) or alpha <= 0 or lambd <= 0:
        raise ValueError("split_bregman: alpha > 0 and lambd > 0 are required, and alpha, lambd, tau, tol must be numbers")
    nat.require_gpu()
    out_device = y.device
    dev = nat.pick_device(y, A, x0)
    yg = y.detach().to(device=dev).contiguous()
    wg = A.detach().to(device=dev).contiguous()
    x0g = None if x0 is None else x0.detach().to(device=dev).contiguous()
    x = torch.empty((n, k), dtype=torch.float32, device=dev)
    if n > 0:
        upd, cost = (C.c_double * maxiter)(), (C.c_double * maxiter)()
        trace = nat.SplitBregmanTrace(maxiter, 0, upd, cost if verbose else None)
        options = nat.SplitBregmanOptions(maxiter, niter_inner, 0, 0, lambd, tol, tau)
        res = nat.SplitBregmanResult()
        res.trace = C.pointer(trace)
        L = nat.lib()
        with torch.cuda.device(dev):
            ws = nat.workspace(dev, L.lasso_split_bregman_workspace_bytes(n, d, k, nat.LASSO_F32), "split_bregman")
            status = L.lasso_split_bregman_solve(
                nat.ptr(yg), yg.stride(0) if n > 1 else d, nat.ptr(wg), wg.stride(0) if d > 1 else k,
                nat.ptr(x0g), k, nat.ptr(x), k, n, d, k, nat.LASSO_F32, alpha,
                C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
        if status == nat.LASSO_ERR_BAD_ARG and res.cholesky_info != 0:
            raise torch.linalg.LinAlgError(
                "linalg.cholesky: The factorization could not be completed because the input is not positive-definite "
                "(the leading minor of order %d is not positive-definite)." % res.cholesky_info)
        nat.check(status)
        its, itn, stopped = res.n_iter, res.itn, bool(res.stopped)
        info = dict(iterations=its, stopped=stopped, update=list(upd[:its]))
        if verbose:
            info['cost'] = list(cost[:its])
    else:
        # no rows: every update is the norm of nothing, 0.0, and the stop fires at the top of iteration 1 unless tol < 0
        stopped = tol >= 0 and maxiter > 1
        its = 1 if stopped else maxiter
        itn = 1 if stopped else maxiter - 1
        info = dict(iterations=its, stopped=stopped, update=[0.0] * its)
        if verbose:
            info['cost'] = [0.0] * its
    if verbose:
        for i, c in enumerate(info['cost']):
            print('iter %3d - cost: %0.4f' % (i, c))                             # :80-82
    x = x.to(device=out_device)
    return (x, itn, info) if return_info else (x, itn)
