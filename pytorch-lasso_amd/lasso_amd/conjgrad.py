"""HIP-backed conjugate gradients: ``cg``, ``batch_cg`` and ``batch_cg_conv2d`` of ``lasso.conjgrad`` (reference
conjgrad.py:60-107) with the reference's names, argument order and defaults, on the kernels of csrc/conjgrad.hip.

All three run the reference's ``conjgrad()`` (conjgrad.py:13-57) line for line: ``x = 0, r = -b, p = b``; ``dot`` is the
sum per row (per image over C, H and W), so ``alpha = rs_old / curv`` and ``rs_new / rs_old`` are one number PER ROW,
while the five exits test sums over the WHOLE batch, in the reference's order inside an iteration:

  1  ``sum|r| <= termcond``, before the product; ``termcond = rtol * |b|_1 * min(sqrt(|b|_1), 0.5)``
  2  ``0 <= curv_sum <= 3 eps``;  3  ``curv_sum < 0`` (at ``i == 0`` with the fallback ``x = -(rs_old / curv) * b``)
  0  ``sqrt(sum rs_new) < tol``, after ``x`` and ``r`` moved and before ``p`` does;  4  ``maxiter`` iterations ran

Nothing is checked or repaired: a row whose ``curv`` is 0 gets ``0 / 0`` as it does in ATen, and with a NaN in the batch
no exit fires and ``maxiter`` iterations run.  The sums are folded in double in a fixed order and rounded once to the
tensors' dtype, in which ``termcond`` and the comparisons are then evaluated: two calls with the same arguments return
bitwise equal results.  The result is a new tensor on the device of ``b``; no input is modified; CPU tensors are staged
through the device.

Each function gains one keyword, ``return_info=False``: with it the call returns ``(x, info)``, ``info`` a dict with
``iterations`` (the index of the iteration an exit fired in; ``maxiter`` for status 4), ``status`` (0 to 4), ``message``
(the reference's text), per iteration the lists ``r_abs`` (``sum|r|`` at its top), ``curv_sum`` and ``rs``
(``sqrt(sum rs_new)``) as the dtype holds them, ``termcond``, ``host_reads`` (waits of the host for the device: one per
chunk of iterations, and with ``rtol=0, tol=0`` one at the end) and ``form`` (which kernels ran).  ``verbose`` prints the
reference's status line, ``verbose > 1`` also its ``iter: %i - rs: %0.4f`` lines, both after the solve (the iterations
run inside one native call) and in the reference's order.

float32 is implemented for all three, float64 (IEEE double throughout; ``tol=1e-10`` is a double-precision tolerance
and can never fire in float32) for ``cg`` and ``batch_cg``.  Refusals, all before any native call: bfloat16, float16,
mixed dtypes and float64 ``batch_cg_conv2d`` raise NotImplementedError naming the dtype; an input that requires grad
under grad mode raises NotImplementedError ("requires_grad": the reference's loop would build a graph); shape
mismatches are AssertionError like the reference's asserts; a negative ``maxiter``, ``tol``, ``rtol`` or ``tik`` raises
ValueError; ``conv_kwargs`` other than ``stride`` and ``padding`` raise NotImplementedError naming the key.

Not provided, by design: the generic ``conjgrad(b, Adot, dot, ...)``.  Its operator is a Python closure; this package
has no torch-op compute path and no CPU fallback.  Out of scope as well: ``iterative_ridge(cg=True)`` (it keeps
raising; this module is what a later change would call), autograd, row sharding over GPUs (every exit is batch-wide).
"""
import ctypes as C

import torch

from . import _native as nat
from .conv2d.ista import _pair

# conjgrad.py:4-10
_status_messages = {
    0: 'Absolute tolerance reached.',
    1: 'Relative tolerance reached.',
    2: 'Curvature has converged.',
    3: 'Curvature is negative.',
    4: 'Maximum iterations reached.'
}


def _dtype_of(name, tensors, allowed):
    dtypes = [t.dtype for t in tensors]
    for dt in dtypes:
        if dt not in allowed or dt != dtypes[0]:
            raise NotImplementedError("lasso_amd: %s is not implemented for %s tensors (got %s)"
                                      % (name, dt, ", ".join(str(d) for d in dtypes)))
    return dtypes[0]


def _check(name, tensors, allowed, maxiter, tol, rtol, tik=0):
    dtype = _dtype_of(name, tensors, allowed)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise NotImplementedError("lasso_amd: %s does not build an autograd graph; inputs that require grad "
                                  "(requires_grad=True) are not supported -- detach them" % name)
    maxiter, tol, rtol, tik = int(maxiter), float(tol), float(rtol), float(tik)
    if maxiter < 0 or not tol >= 0 or not rtol >= 0 or not tik >= 0:
        raise ValueError("%s: maxiter, tol, rtol and tik must be >= 0" % name)
    return dtype, maxiter, tol, rtol, tik


def _counts(status, it):
    """how many entries of r_abs, curv_sum and rs an exit with `status` in iteration `it` leaves"""
    if status == nat.CG_REL_TOL:
        return it + 1, it, it
    if status in (nat.CG_CURV_CONVERGED, nat.CG_CURV_NEGATIVE):
        return it + 1, it + 1, it
    if status == nat.CG_ABS_TOL:
        return it + 1, it + 1, it + 1
    return it, it, it


def _report(info, verbose):
    verbose = int(verbose)
    if verbose > 1:
        # :54-55 -- every iteration that went on to move p, i.e. all but one that ended in exit 0
        shown = len(info['rs']) - (1 if info['status'] == nat.CG_ABS_TOL else 0)
        for i in range(shown):
            print('iter: %i - rs: %0.4f' % (i, info['rs'][i]))
    if verbose:
        print(info['message'])


def _finish(res, traces, want_trace):
    status, it = res.status, res.n_iter
    info = dict(iterations=it, status=status, message=_status_messages[status], termcond=res.termcond,
                host_reads=res.host_reads, form=nat.CG_FORMS[res.form])
    nr, nc, ns = _counts(status, it) if want_trace else (0, 0, 0)
    info['r_abs'], info['curv_sum'], info['rs'] = list(traces[0][:nr]), list(traces[1][:nc]), list(traces[2][:ns])
    return info


def _empty_info(maxiter):
    # no rows: |b|_1 = 0 and sum|r| = 0 <= termcond = 0 at the top of iteration 0 (if there is one)
    status = nat.CG_REL_TOL if maxiter > 0 else nat.CG_MAXITER
    return dict(iterations=0, status=status, message=_status_messages[status], termcond=0.0, host_reads=0, form='none',
                r_abs=[0.0] if maxiter > 0 else [], curv_sum=[], rs=[])


def _request(maxiter, tol, rtol, tik, want_trace, plain):
    cap = maxiter if want_trace else 0
    traces = [(C.c_double * max(cap, 1))() for _ in range(3)]
    trace = nat.CgTrace(cap, 0, traces[0], traces[1], traces[2])
    options = nat.CgOptions(maxiter, nat.CG_PLAIN_FORM if plain else 0, tol, rtol, tik)
    res = nat.CgResult()
    res.trace = C.pointer(trace)
    return options, res, traces, trace


def _dense(name, A, b, maxiter, tol, rtol, verbose, return_info):
    n, k = b.shape
    assert A.shape == (k, k)
    dtype, maxiter, tol, rtol, _ = _check(name, (A, b), (torch.float32, torch.float64), maxiter, tol, rtol)
    if n == 0:
        x, info = torch.empty_like(b), _empty_info(maxiter)
    else:
        nat.require_gpu()
        dev = nat.pick_device(b, A)
        ag = A.detach().to(device=dev).contiguous()
        bg = b.detach().to(device=dev).contiguous()
        x = torch.empty((n, k), dtype=dtype, device=dev)
        want_trace = bool(return_info) or int(verbose) > 1
        options, res, traces, _trace = _request(maxiter, tol, rtol, 0.0, want_trace, _FORCE_PLAIN[0])
        L = nat.lib()
        with torch.cuda.device(dev):
            ws = nat.workspace(dev, L.lasso_cg_workspace_bytes(n, k, nat.DT[dtype]), "conjgrad")
            status = L.lasso_cg_solve(nat.ptr(ag), k, nat.ptr(bg), k, nat.ptr(x), k, n, k, nat.DT[dtype],
                                      C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
        nat.check(status)
        info = _finish(res, traces, want_trace)
        x = x.to(device=b.device)
    _report(info, verbose)
    return (x, info) if return_info else x


def cg(A, b, maxiter=None, tol=1e-10, rtol=1.0, verbose=False, return_info=False):
    """Solve ``A x = b`` for one right-hand side: A [k,k], b [k] -> x [k].  The n = 1 batch of ``batch_cg`` (the
    reference's ``Adot = A.matmul(v)`` and ``dot = u.dot(v)``, conjgrad.py:60-69); ``maxiter`` defaults to ``20 * len(b)``."""
    assert A.dim() == 2
    assert b.dim() == 1
    if maxiter is None:
        maxiter = 20 * len(b)
    out = _dense("cg", A, b.reshape(1, -1), maxiter, tol, rtol, verbose, return_info)
    if return_info:
        return out[0].reshape(-1), out[1]
    return out.reshape(-1)


def batch_cg(A, b, maxiter=None, tol=1e-10, rtol=1.0, verbose=False, return_info=False):
    """Solve ``x A^T = b`` for a batch of right-hand sides with one step length per row: A [k,k] (not assumed
    symmetric), b [n,k] -> x [n,k] (conjgrad.py:72-81: ``Adot(v) = torch.mm(v, A.T)``, ``dot`` the sum over dim 1);
    ``maxiter`` defaults to ``20 * b.size(1)``.  float32: one fp32-MFMA product per iteration whose epilogue takes the
    per-row curvature; float64: the fp64-MFMA product and a pass that takes it."""
    assert A.dim() == 2
    assert b.dim() == 2
    if maxiter is None:
        maxiter = 20 * b.size(1)
    return _dense("batch_cg", A, b, maxiter, tol, rtol, verbose, return_info)


def batch_cg_conv2d(kernel, b, tik=0, maxiter=None, tol=1e-10, rtol=1.0, verbose=False, return_info=False, **conv_kwargs):
    """Solve ``(W^T W + tik I) z = b`` where ``W`` is the Toeplitz matrix of ``conv_transpose2d(., kernel)``
    (conjgrad.py:84-107): kernel [K,C,kh,kw] (the layout of ``ista_conv2d``'s ``weight``), b [N,K,Hz,Wz] -> z of b's
    shape.  ``Adot(v) = conv2d(conv_transpose2d(v, kernel), kernel) + tik * v``, the ``tik`` term only when ``tik > 0``;
    ``dot`` sums over C, H and W: one step length per image.  ``conv_kwargs`` accepts ``stride`` and ``padding`` (an int
    or a pair each); ``maxiter`` defaults to ``20 * b[0].numel()``.  This is the ridge code of a convolutional
    dictionary: ``batch_cg_conv2d(w, conv2d(x, w), tik)``.  float32 only."""
    assert kernel.dim() == 4
    assert b.dim() == 4
    for key in conv_kwargs:
        if key not in ('stride', 'padding'):
            raise NotImplementedError("lasso_amd: batch_cg_conv2d takes the conv_kwargs stride and padding; %r is not "
                                      "implemented" % key)
    assert b.shape[1] == kernel.shape[0]
    if maxiter is None:
        maxiter = 20 * (b[0].numel() if b.shape[0] > 0 else b.shape[1] * b.shape[2] * b.shape[3])
    dtype, maxiter, tol, rtol, tik = _check("batch_cg_conv2d", (kernel, b), (torch.float32,), maxiter, tol, rtol, tik)
    sh, sw = _pair(conv_kwargs.get('stride', 1))
    ph, pw = _pair(conv_kwargs.get('padding', 0))
    N, K, Hz, Wz = b.shape
    _, Cc, kh, kw = kernel.shape
    H, W = (Hz - 1) * sh - 2 * ph + kh, (Wz - 1) * sw - 2 * pw + kw
    if N == 0 or b.numel() == 0:
        z, info = torch.empty_like(b), _empty_info(maxiter)
    else:
        assert H > 0 and W > 0, "conv_transpose2d of b would be empty"
        nat.require_gpu()
        dev = nat.pick_device(b, kernel)
        wg = kernel.detach().to(device=dev).contiguous()
        bg = b.detach().to(device=dev).contiguous()
        z = torch.empty((N, K, Hz, Wz), dtype=dtype, device=dev)
        want_trace = bool(return_info) or int(verbose) > 1
        options, res, traces, _trace = _request(maxiter, tol, rtol, tik, want_trace, _FORCE_PLAIN[0])
        geom = (N, Cc, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw)
        L = nat.lib()
        with torch.cuda.device(dev):
            ws = nat.workspace(dev, L.lasso_conv_cg_workspace_bytes(*geom), "conjgrad_conv")
            status = L.lasso_conv_cg_solve(nat.ptr(wg), nat.ptr(bg), nat.ptr(z), *geom, nat.LASSO_F32,
                                           C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
        nat.check(status)
        info = _finish(res, traces, want_trace)
        z = z.to(device=b.device)
    _report(info, verbose)
    return (z, info) if return_info else z


# tests and tools/bench_conjgrad.py: take the plain forms (bit 0 of lasso_cg_options.reserved) where a fused or implicit
# kernel would run
_FORCE_PLAIN = [False]
