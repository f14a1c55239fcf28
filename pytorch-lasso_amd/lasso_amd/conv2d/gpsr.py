"""HIP-backed convolutional GPSR-Basic: the reference's ``gpsr_basic(y, A, tau, AT, x0, ...)`` (gpsr.py:209-365) with
the two closures a user passes for a convolutional dictionary,

    A  = lambda v: F.conv_transpose2d(v, W, stride=s, padding=p)
    AT = lambda v: F.conv2d(v, W, stride=s, padding=p)

on the kernels of csrc/conv_gpsr.hip (the loop and the decision kernels are those of the linear solver)."""
import ctypes as C
import os

import torch

from .. import _native as nat
from ..linear.solvers.gpsr import _KW_DEFAULTS, _request, _report
from .ista import _pair


def _forced_general():
    """LASSO_CONV_GPSR_FORM=patches forces the general kernel family (bit 0 of options.reserved) where the implicit
    one would run: the A/B knob of tests/test_gpsr_conv_gpu.py and tools/bench_conv_gpsr.py"""
    return 1 if os.environ.get("LASSO_CONV_GPSR_FORM", "") == "patches" else 0


def gpsr_conv2d(x, weight, tau, z0=None, stride=1, padding=0, stop_criterion=3, tol=1e-2, maxiter=1000, miniter=5,
                init=0, continuation=False, debias=False, verbose=0, return_info=False, **kwargs):
    """min_z 0.5 ||x - conv_transpose2d(z, W)||^2 + tau ||z||_1 over the whole batch by GPSR-Basic.
    x [N,C,H,W], weight [K,C,kh,kw] -> z [N,K,Hz,Wz], the shape of ``conv2d(x, weight, stride, padding)`` (a new
    tensor; no input is modified).  ``stride`` and ``padding`` take what ``ista_conv2d`` takes (an int or a pair).

    Every other argument, default, warning and print is that of ``lasso_amd.linear.solvers.gpsr_basic``: every inner
    product is a sum over all images, so an iteration has one step size, one line search and one stop decision.
    ``**kwargs``: mu, lambda_backtrack, cont_steps, first_tau_factor, tol_debias, maxiter_debias, miniter_debias;
    any other keyword raises TypeError.  An unknown ``stop_criterion`` or ``init`` raises ValueError.  ``init=1``
    draws the start with ``randn`` on the device, ``init=2`` starts at ``conv2d(x, W)``.  Debias refuses a code with
    more nonzeros than ``x.numel()`` (gpsr.py:142).

    An image size that ``conv_transpose2d`` of the code does not give back, (Hz-1) s - 2 p + k != H, raises
    RuntimeError (the reference fails at ``y - A(x)``).  float32 tensors only: any other dtype, and inputs that
    require grad under grad mode, raise NotImplementedError.  CPU tensors are staged through the device and the
    result comes back on the device of ``x``.  ``return_info`` also returns the dictionary of the linear function
    plus ``form``, the kernel family that ran: ``'implicit'`` where the implicit-GEMM convolution kernels cover the
    geometry (stride 1, few channels, 3/5/7 kernels), else ``'patches'``; the environment variable
    ``LASSO_CONV_GPSR_FORM=patches`` forces the latter.  No CPU fallback."""
    verbose = int(verbose)
    if stop_criterion not in (0, 1, 2, 3, 4):
        raise ValueError('Unknown stopping criterion')                       # gpsr.py:240-241
    if z0 is None and init not in (0, 1, 2):
        raise ValueError('Unknown initialization option')                    # :272
    for name in kwargs:
        if name not in _KW_DEFAULTS:
            raise TypeError("gpsr_conv2d() got an unexpected keyword argument '%s'" % name)
    opt = dict(_KW_DEFAULTS, **kwargs)
    if x.dim() != 4 or weight.dim() != 4:
        raise RuntimeError("gpsr_conv2d expects 4-D x and weight")
    N, Cin, H, W = x.shape
    K, Cw, kh, kw = weight.shape
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    if Cw != Cin:
        raise RuntimeError("shape mismatch: x %s, weight %s" % (tuple(x.shape), tuple(weight.shape)))
    Hz, Wz = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1       # the shape of conv2d(x, W)
    if z0 is not None:
        if z0.dim() != 4 or z0.shape[0] != N or z0.shape[1] != K:
            raise RuntimeError("shape mismatch: x %s, weight %s, z0 %s"
                               % (tuple(x.shape), tuple(weight.shape), tuple(z0.shape)))
        Hz, Wz = z0.shape[2], z0.shape[3]
    if Hz < 1 or Wz < 1 or (Hz - 1) * sh - 2 * ph + kh != H or (Wz - 1) * sw - 2 * pw + kw != W:
        raise RuntimeError("The size of conv_transpose2d of the code (%d x %d) must match the size of x (%d x %d)"
                           % ((Hz - 1) * sh - 2 * ph + kh, (Wz - 1) * sw - 2 * pw + kw, H, W))
    tensors = [t for t in (x, weight, z0) if t is not None]
    for t in tensors:
        if t.dtype != torch.float32:
            raise NotImplementedError("lasso_amd: gpsr_conv2d is not implemented for %s tensors" % t.dtype)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise NotImplementedError("lasso_amd: gpsr_conv2d does not build an autograd graph; inputs that "
                                  "require grad (requires_grad=True) are not supported -- detach them")
    nat.require_gpu()
    out_device = x.device
    dev = nat.pick_device(x, weight, z0)
    xg = x.detach().to(dev).contiguous()
    wg = weight.detach().to(dev).contiguous()
    if z0 is None and init == 1:
        z0 = torch.randn(N, K, Hz, Wz, dtype=torch.float32, device=dev)      # :268 randn_like(Ay)
    z0g = z0.detach().to(dev).contiguous() if z0 is not None else None
    z = torch.empty((N, K, Hz, Wz), dtype=torch.float32, device=dev)
    info = dict(iterations=0, objective=[], accepted_lambda=[], trials=[], criterion=[], final_objective=float('nan'))
    form = 'patches'
    if N > 0:
        geom = (N, Cin, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw)
        options, res, keep = _request(stop_criterion, tol, maxiter, miniter, init, continuation, debias, opt,
                                      z0 is not None)
        options.reserved = _forced_general()
        L = nat.lib()
        with torch.cuda.device(dev):
            form = L.lasso_conv_gpsr_form(*geom, options.reserved).decode()
            ws = nat.workspace(dev, L.lasso_conv_gpsr_workspace_bytes(*geom), "conv_gpsr")
            nat.check(L.lasso_conv_gpsr_solve(
                nat.ptr(xg), nat.ptr(wg), nat.ptr(z0g), nat.ptr(z), *geom, nat.LASSO_F32, float(tau),
                C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)))
        info = _report(res, keep, stop_criterion, tol, debias, opt, verbose)
    info['form'] = form
    z = z.to(out_device)
    return (z, info) if return_info else z
