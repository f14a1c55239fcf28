"""HIP-backed convolutional ISTA/FISTA: same signature, defaults and error behaviour as
``lasso.conv2d.ista.ista_conv2d`` (reference lasso/conv2d/ista.py:7-49)."""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import _native as nat
from .lip_const import lip_bound_conv2d, lip_constant


def _pair(v):
    if isinstance(v, (tuple, list)):
        if len(v) == 1:
            return int(v[0]), int(v[0])
        if len(v) != 2:
            raise RuntimeError("expected an int or a pair, got %r" % (v,))
        return int(v[0]), int(v[1])
    return int(v), int(v)


def _geometry(x, z0, weight, stride, padding):
    if x.dim() != 4 or z0.dim() != 4 or weight.dim() != 4:
        raise RuntimeError("ista_conv2d expects 4-D x, z0, weight")
    N, Cin, H, W = x.shape
    K, Cw, kh, kw = weight.shape
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    if z0.shape[0] != N or z0.shape[1] != K or Cw != Cin:
        raise RuntimeError("shape mismatch: x %s, weight %s, z0 %s"
                           % (tuple(x.shape), tuple(weight.shape), tuple(z0.shape)))
    Hz, Wz = z0.shape[2], z0.shape[3]
    if (Hz - 1) * sh - 2 * ph + kh != H or (Wz - 1) * sw - 2 * pw + kw != W:
        # the reference fails at `x_hat - x` (ista.py:19) with torch's broadcasting RuntimeError
        raise RuntimeError("The size of conv_transpose2d(z0) (%d x %d) must match the size of x (%d x %d)"
                           % ((Hz - 1) * sh - 2 * ph + kh, (Wz - 1) * sw - 2 * pw + kw, H, W))
    return (N, Cin, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw)


class _F32:
    """What differs between the two tensor dtypes of the convolutional path: the byte-count functions, the workspace
    tags and how the solve's last sum comes back."""
    dtype, code, itemsize = torch.float32, nat.LASSO_F32, 4
    ws_bytes, trace_bytes, bw_bytes = ('lasso_conv_ista_workspace_bytes', 'lasso_conv_ista_trace_bytes',
                                       'lasso_conv_ista_backward_workspace_bytes')
    tag, bw_tag = "conv", "conv_bw"

    @staticmethod
    def solve(L, ptrs, geom, alpha, lr, fast, maxiter, tol, want, ws):
        """one lasso_conv_ista_solve -> (iterations, last_delta)"""
        iters, last = C.c_int32(0), C.c_float(float('nan'))
        nat.check(L.lasso_conv_ista_solve(*ptrs, *geom, nat.LASSO_F32, float(alpha), float(lr), int(bool(fast)),
                                          int(maxiter), float(tol), C.byref(iters) if want else None,
                                          C.byref(last) if want else None, *ws))
        return iters.value, last.value

    @staticmethod
    def budget(numel, tol):
        return nat.stop_budget(numel, tol)


class _F64(_F32):
    dtype, code, itemsize = torch.float64, nat.LASSO_F64, 8
    ws_bytes, trace_bytes, bw_bytes = ('lasso_conv_ista_workspace_bytes_f64', 'lasso_conv_ista_trace_bytes_f64',
                                       'lasso_conv_ista_backward_workspace_bytes_f64')
    tag, bw_tag = "conv_f64", "conv_bw_f64"

    @staticmethod
    def solve(L, ptrs, geom, alpha, lr, fast, maxiter, tol, want, ws):
        iters, last = C.c_int32(0), C.c_double(float('nan'))
        nat.check(L.lasso_conv_ista_solve_f64(*ptrs, *geom, float(alpha), float(lr), int(bool(fast)), int(maxiter),
                                              float(tol), C.byref(iters) if want else None,
                                              C.byref(last) if want else None, *ws))
        return iters.value, last.value

    @staticmethod
    def budget(numel, tol):
        return float(numel) * tol            # ista.py:16 in double


def _path(what, *tensors):
    """_F32 / _F64 for tensors that are all float32 / all float64; anything else is refused before any launch."""
    for P in (_F32, _F64):
        if all(t.dtype == P.dtype for t in tensors):
            return P
    raise NotImplementedError("lasso_amd: %s is implemented for float32 and for float64 tensors (all of one dtype), "
                              "got %s" % (what, ", ".join(str(t.dtype) for t in tensors)))


def conv_loss(x, z, weight, alpha, stride=1, padding=0):
    """(0.5*||x - conv_transpose2d(z, W)||^2 + alpha*||z||_1) / N on the GPU (ista.py:23-26): a 0-d tensor of the
    inputs' dtype (float32 or float64)."""
    nat.require_gpu()
    geom = _geometry(x, z, weight, stride, padding)
    P = _path("conv_loss", x, z, weight)
    dev = nat.pick_device(x)
    xg, zg, wg = (t.detach().to(dev).contiguous() for t in (x, z, weight))
    L = nat.lib()
    loss = torch.empty((), dtype=P.dtype, device=dev)
    with torch.cuda.device(dev):
        ws = nat.workspace(dev, getattr(L, P.ws_bytes)(*geom), P.tag)
        if P is _F64:
            nat.check(L.lasso_conv_objective_f64(nat.ptr(xg), nat.ptr(wg), nat.ptr(zg), *geom, float(alpha),
                                                 nat.ptr(loss), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)))
        else:
            nat.check(L.lasso_conv_objective(nat.ptr(xg), nat.ptr(wg), nat.ptr(zg), *geom, nat.LASSO_F32, float(alpha),
                                             nat.ptr(loss), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)))
    return loss


def _solve(P, xg, zg, wg, geom, alpha, lr, fast, maxiter, tol, verbose, dev):
    """The solve on device tensors (contiguous, of P's dtype) -> (z, iterations, last_delta)."""
    L = nat.lib()
    z = torch.empty_like(zg)
    iters, last = 0, float('nan')
    with torch.cuda.device(dev):
        ws = nat.workspace(dev, getattr(L, P.ws_bytes)(*geom), P.tag)
        wsa = (nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
        if geom[0] == 0:
            z = zg.clone()
        elif not verbose:
            iters, last = P.solve(L, (nat.ptr(xg), nat.ptr(wg), nat.ptr(zg), nat.ptr(z)), geom, alpha, lr, fast,
                                  maxiter, tol, True, wsa)
        else:
            # the reference prints the objective of z before every iteration (:37-38); one HIP
            # iteration at a time cannot carry the momentum state across calls, so the verbose
            # trace re-solves with maxiter = i for the printed value (debugging mode)
            stride, padding = geom[9:11], geom[11:13]
            budget = P.budget(zg.numel(), tol)
            for i in range(int(maxiter)):
                zi = zg
                if i > 0:
                    zi = torch.empty_like(zg)
                    P.solve(L, (nat.ptr(xg), nat.ptr(wg), nat.ptr(zg), nat.ptr(zi)), geom, alpha, lr, fast, i, 0.0,
                            False, wsa)
                print('loss: %0.4f' % conv_loss(xg, zi, wg, alpha, stride, padding).item())
                iters, last = P.solve(L, (nat.ptr(xg), nat.ptr(wg), nat.ptr(zg), nat.ptr(z)), geom, alpha, lr, fast,
                                      i + 1, tol, True, wsa)
                if iters <= i or (tol > 0 and last <= budget):
                    break
    return z, iters, last


class _UnrolledConvIsta(torch.autograd.Function):
    """Differentiable convolutional solve (SURVEY.md 8f rows f3 + f4): the reference's loop is plain
    torch code, so torch.autograd differentiates through its unrolled iterations (ista.py:36-46).
    Forward: the solve as without grad (its z, iteration count and last delta are returned), then
    lasso_conv_ista_run_traced replays its T iterations keeping z_0..z_T; backward:
    lasso_conv_ista_backward (csrc/conv_autograd.hip; float64 tensors: the double trace and the double
    reverse pass of csrc/conv_f64.hip).  The step lr, the momentum schedule and the stop decision are
    constants of the graph."""

    @staticmethod
    def forward(ctx, x, z0, weight, geom, alpha, lr, fast, maxiter, tol, verbose, info):
        dev = x.device
        P = _path("ista_conv2d", x, z0, weight)
        xg, zg, wg = (t.detach().contiguous() for t in (x, z0, weight))
        L = nat.lib()
        z, iters, last = None, int(maxiter), float('nan')
        # With the stop rule active T is not known in advance: the ordinary solve finds it first (bitwise
        # deterministic, so the replay lands on the same iterates) -- the trace is then exactly T + 1 iterates
        if tol > 0 or verbose or geom[0] == 0:
            z, iters, last = _solve(P, xg, zg, wg, geom, alpha, lr, fast, maxiter, tol, verbose, dev)
        steps = int(iters)
        trace = torch.empty(getattr(L, P.trace_bytes)(*geom, steps) // P.itemsize, dtype=P.dtype, device=dev)
        if geom[0] > 0:
            zt = torch.empty_like(zg)
            with torch.cuda.device(dev):
                ws = nat.workspace(dev, getattr(L, P.ws_bytes)(*geom), P.tag)
                nat.check(L.lasso_conv_ista_run_traced(nat.ptr(xg), nat.ptr(wg), nat.ptr(zg), nat.ptr(zt), *geom,
                                                       P.code, float(alpha), float(lr), int(bool(fast)), steps,
                                                       nat.ptr(trace), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)))
            if z is None:
                z = zt
        ctx.save_for_backward(xg, wg, trace)
        ctx.geom, ctx.lr, ctx.fast, ctx.steps, ctx.zshape, ctx.path = geom, float(lr), bool(fast), steps, zg.shape, P
        info.update(iterations=iters, last_delta=last)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_z):
        xg, wg, trace = ctx.saved_tensors
        dev, P = xg.device, ctx.path
        L = nat.lib()
        need_x, need_z0, need_w = ctx.needs_input_grad[:3]
        gx = torch.empty_like(xg) if need_x else None
        gw = torch.empty_like(wg) if need_w else None
        gz0 = torch.empty(ctx.zshape, dtype=P.dtype, device=dev) if need_z0 else None
        gz = grad_z.detach().to(device=dev, dtype=P.dtype).contiguous()
        with torch.cuda.device(dev):
            ws = nat.workspace(dev, getattr(L, P.bw_bytes)(*ctx.geom), P.bw_tag)
            nat.check(L.lasso_conv_ista_backward(nat.ptr(xg), nat.ptr(wg), nat.ptr(trace), nat.ptr(gz), *ctx.geom,
                                                 P.code, ctx.lr, int(ctx.fast), ctx.steps, nat.ptr(gx),
                                                 nat.ptr(gw), nat.ptr(gz0), nat.ptr(ws), ws.numel(),
                                                 nat.stream_ptr(dev)))
        return (gx, gz0, gw) + (None,) * 8


def ista_conv2d(x, z0, weight, alpha=1.0, stride=1, padding=0, fast=True,
                maxiter=10, lr='auto', tol=1e-5, verbose=False, return_info=False):
    """x [N,C,H,W], z0 [N,K,Hz,Wz], weight [K,C,kh,kw] -> z [N,K,Hz,Wz] (a new tensor;
    ``maxiter=0`` returns ``z0`` itself, ista.py:32,49).  ``lr='auto'`` uses the Toeplitz
    bound and, like the reference, needs ``stride == 1`` (:9-15).  ``lr='exact'`` (extension)
    takes the step ``1 / (theta + residual)`` from ``lip_constant`` of the detached weight at x's
    size: the exact constant instead of its bound (up to 11x longer steps for dictionaries with
    many channels), for any stride; like ``'auto'`` it is a constant of the graph.  ``return_info``
    (extension) also returns ``dict(iterations=..., last_delta=...)``.  No CPU fallback.

    x, z0 and weight are all float32 or all float64.  float64 tensors run in IEEE double throughout
    (fp64 MFMA, csrc/conv_f64.hip): the result, ``last_delta`` and the gradients are doubles and
    ``lr='auto'`` uses the double bound; ``torch.autograd.gradcheck`` applies.  Any other dtype, or a
    mix, raises NotImplementedError.

    Differentiable like the reference's loop: with grad mode on and any of x, z0, weight
    requiring grad, z carries the derivative of the iterations run (the step, the momentum
    schedule and the stop decision are constants; double backward is not supported).  With
    ``lr='auto'`` the step is computed from the detached weight and is a constant too -- an
    extension: the reference raises TypeError there when weight requires grad."""
    nat.require_gpu()
    wants_grad = torch.is_grad_enabled() and (x.requires_grad or z0.requires_grad or weight.requires_grad)
    if lr == 'auto':
        if stride != 1:
            raise NotImplementedError("auto lr is only implemented for stride == 1.")   # :10-12
        Lb = lip_bound_conv2d(weight, padding)                                           # :14
        if Lb.dtype == torch.float64:
            lr = 1.0 / Lb.item()                                                        # :15 in double
        else:
            lr = float(np.float32(1.0) / np.float32(Lb.item()))                         # :15 (fp32 like the tensor op)
    geom = _geometry(x, z0, weight, stride, padding)
    P = _path("ista_conv2d", x, z0, weight)
    if isinstance(lr, str) and lr == 'exact':
        # theta approaches lambda_max from below and some eigenvalue lies within `residual` of it: L = theta + residual
        _, linfo = lip_constant(weight.detach(), x.shape[-2:], stride=stride, padding=padding, return_info=True)
        lr = 1.0 / (linfo['theta'] + linfo['residual'])
    if maxiter == 0:
        return (z0, dict(iterations=0, last_delta=float('nan'))) if return_info else z0
    out_device = z0.device
    dev = nat.pick_device(x, weight, z0)
    if wants_grad:
        # CPU inputs are staged through the device inside the graph: their gradients arrive on their own devices
        info = {}
        z = _UnrolledConvIsta.apply(x.to(dev), z0.to(dev), weight.to(dev), geom, float(alpha), float(lr), bool(fast),
                                    int(maxiter), float(tol), bool(verbose), info)
        iters, last = info['iterations'], info['last_delta']
    else:
        xg, zg, wg = (t.detach().to(dev).contiguous() for t in (x, z0, weight))
        z, iters, last = _solve(P, xg, zg, wg, geom, alpha, lr, fast, maxiter, tol, verbose, dev)
    if z.device != out_device:
        z = z.to(out_device)
    if return_info:
        return z, dict(iterations=iters, last_delta=last)
    return z
