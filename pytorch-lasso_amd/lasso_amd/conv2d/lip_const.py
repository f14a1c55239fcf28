"""The Lipschitz constant of a convolutional dictionary.  ``lip_constant``: the exact value (reference
lip_const.py:8-31), Lanczos on the GPU by ``lasso_conv_lip_constant``.  ``lip_bound_conv2d`` / ``LipBoundConv2d``: the
Toeplitz bound of a stride-1 conv2d, same call surface as the reference's (lip_const.py:32-135), computed by
``lasso_conv_lip_bound`` on the GPU."""
import ctypes as C
import math
import warnings

import torch

from .. import _native as nat


def _check(kernel_size, stride):
    if not kernel_size[-1] == kernel_size[-2]:
        raise ValueError("The last 2 dim of the kernel must be equal.")     # :99-100
    if not kernel_size[-1] % 2 == 1:
        raise ValueError("The dimension of the kernel must be odd.")        # :101-102
    if not stride == 1:
        raise NotImplementedError("LipBound not implemented for stride > 1.")  # :103-104


def lip_bound_conv2d(kernel, padding, stride=1, sample=50, sqrt=False):
    """-> 0-d float32 tensor on the kernel's device, like the reference (:131-135).

    A float64 kernel gives a float64 0-d tensor: phases, sin / cos and every sum in double on the frequency grid
    ``2*pi*i/(sample-1)``.  This is an extension -- the reference multiplies a double kernel by its float32 phase
    table and fails with a dtype RuntimeError."""
    assert kernel.dim() == 4                                                # :98
    _check(kernel.shape, stride)
    nat.require_gpu()
    if kernel.dtype not in (torch.float32, torch.float64):
        raise NotImplementedError("lasso_amd: lip_bound_conv2d is implemented for float32 and float64 kernels")
    f64 = kernel.dtype == torch.float64
    out_device = kernel.device
    dev = nat.pick_device(kernel)
    wg = kernel.detach().to(dev).contiguous()
    K, Cin, ks, _ = wg.shape
    L = nat.lib()
    val = C.c_double(0.0)
    with torch.cuda.device(dev):
        size_fn, bound_fn = ((L.lasso_conv_lip_workspace_bytes_f64, L.lasso_conv_lip_bound_f64) if f64 else
                             (L.lasso_conv_lip_workspace_bytes, L.lasso_conv_lip_bound))
        ws = nat.workspace(dev, size_fn(K, Cin, ks, int(sample)), "convlip")
        nat.check(bound_fn(nat.ptr(wg), K, Cin, ks, int(padding), int(sample), int(bool(sqrt)),
                           C.byref(val), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)))
    return torch.tensor(val.value, dtype=kernel.dtype, device=out_device)


def _pair(v):
    if isinstance(v, (tuple, list)):
        if len(v) == 1:
            return int(v[0]), int(v[0])
        if len(v) != 2:
            raise RuntimeError("expected an int or a pair, got %r" % (v,))
        return int(v[0]), int(v[1])
    return int(v), int(v)


_LIP_DEFAULT_TOL = {torch.float32: 1e-5, torch.float64: 1e-10}


def lip_constant(kernel, imsize, transpose=False, sqrt=False, *, tol=None, maxiter=None, return_info=False, **kwargs):
    """The exact Lipschitz constant of a convolutional dictionary -> Python float, like ``lasso.conv2d.lip_const.
    lip_constant`` (reference lip_const.py:8-31): the largest eigenvalue of ``conv_transpose2d(conv2d(v))`` on
    ``C x imsize`` images (``transpose=False``) or of ``conv2d(conv_transpose2d(v))`` on ``K x imsize`` codes
    (``transpose=True``); ``sqrt=True`` returns its square root (:28-29).  ``kernel`` is ``[K, C, kh, kw]``, float32 or
    float64; the value is computed in that dtype.  ``kwargs`` takes ``stride`` and ``padding`` (an int or a pair each).

    Where the reference calls ARPACK with a numpy -> torch -> numpy round trip per product, this runs Lanczos with full
    reorthogonalisation on the device (``lasso_conv_lip_constant``, csrc/conv_lanczos.hip): the two convolution
    launchers of ``ista_conv2d``, four kernels of vector arithmetic per step, and one host read per chunk of 8, 16, 32,
    32, ... steps.  The nonzero spectra of the two operators coincide, so the iteration runs in the smaller of the two
    spaces whatever ``transpose`` says (``info['space']``); ``imsize`` keeps the reference's meaning.  The start vector
    is a fixed counter-based pseudo-random vector and every sum is folded in a fixed order: the same input gives the
    same bits.

    ``tol`` (default 1e-5 for float32, 1e-10 for float64) is relative: the first step ``j`` with
    ``beta_j * |s_j| <= tol * theta_j`` stops -- some eigenvalue lies within ``beta_j * |s_j|`` of the Ritz value
    ``theta_j``; ``tol=0`` runs to ``maxiter`` or to breakdown.  ``maxiter`` (default ``min(dim, 512)``, ``dim`` of the
    space ``transpose`` names) caps the Lanczos steps; reaching it warns once and returns the best ``theta``.  More than
    512 steps, or a basis beyond 1 GiB, restart from the current Ritz vector.  ``return_info=True`` returns ``(value,
    info)`` with ``theta``, ``residual``, ``steps``, ``matvecs``, ``host_reads``, ``space`` ('image' / 'code'), ``dim``,
    ``status`` ('converged'; 'breakdown': an invariant subspace was found or the basis spans the space, the value is
    exact; 'maxiter'; 'nonfinite'), ``restarts`` and ``history`` (``theta_1 .. theta_steps``).

    Departures from the reference, where ARPACK raises: a NaN or Inf in the kernel returns NaN, an all-zero kernel 0.0.
    A kernel that requires grad is detached (the reference is ``@torch.no_grad()``).  Refusals, before any native call:
    ``kwargs`` other than ``stride`` and ``padding`` and dtypes other than float32 / float64 raise NotImplementedError
    naming the key / dtype; with ``transpose=False`` a size that does not round-trip, ``(H + 2p - kh) % stride != 0`` or
    likewise the width, raises ValueError (the reference fails inside ARPACK); so do a negative ``tol`` and
    ``maxiter < 1``."""
    if kernel.dim() != 4:
        raise ValueError("lip_constant expects a 4-D kernel [K, C, kh, kw], got %d-D" % kernel.dim())
    for key in kwargs:
        if key not in ('stride', 'padding'):
            raise NotImplementedError("lasso_amd: lip_constant takes the conv kwargs stride and padding; %r is not "
                                      "implemented" % key)
    if kernel.dtype not in _LIP_DEFAULT_TOL:
        raise NotImplementedError("lasso_amd: lip_constant is implemented for float32 and float64 kernels, got %s"
                                  % kernel.dtype)
    sh, sw = _pair(kwargs.get('stride', 1))
    ph, pw = _pair(kwargs.get('padding', 0))
    K, Cc, kh, kw = (int(v) for v in kernel.shape)
    H, W = (int(v) for v in imsize)
    if min(K, Cc, kh, kw, H, W, sh, sw) < 1 or min(ph, pw) < 0:
        raise ValueError("lip_constant: empty kernel or image, stride < 1 or padding < 0")
    if transpose:
        if (H - 1) * sh - 2 * ph + kh < 1 or (W - 1) * sw - 2 * pw + kw < 1:
            raise ValueError("lip_constant: conv_transpose2d of a %d x %d code would be empty" % (H, W))
        dim = K * H * W
    else:
        eh, ew = H + 2 * ph - kh, W + 2 * pw - kw
        if eh < 0 or ew < 0 or eh % sh != 0 or ew % sw != 0:
            raise ValueError("lip_constant: a %d x %d image does not round-trip through conv2d and conv_transpose2d "
                             "with kernel %d x %d, stride (%d, %d), padding (%d, %d): (H + 2p - kh) %% stride must be 0"
                             % (H, W, kh, kw, sh, sw, ph, pw))
        dim = Cc * H * W
    tol = _LIP_DEFAULT_TOL[kernel.dtype] if tol is None else float(tol)
    maxiter = min(dim, 512) if maxiter is None else int(maxiter)
    if not tol >= 0 or maxiter < 1:
        raise ValueError("lip_constant: tol must be >= 0 and maxiter >= 1")
    nat.require_gpu()
    dev = nat.pick_device(kernel)
    wg = kernel.detach().to(dev).contiguous()
    L = nat.lib()
    history = (C.c_double * maxiter)()
    options = nat.ConvLipOptions(maxiter, 0, tol)
    res = nat.ConvLipResult()
    res.history, res.history_capacity = history, maxiter
    geom = (K, Cc, kh, kw, H, W, sh, sw, ph, pw, int(bool(transpose)), nat.DT[kernel.dtype])
    with torch.cuda.device(dev):
        ws = nat.workspace(dev, L.lasso_conv_lip_constant_workspace_bytes(*geom, maxiter), "conv_lanczos")
        nat.check(L.lasso_conv_lip_constant(nat.ptr(wg), *geom, C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(),
                                            nat.stream_ptr(dev)))
    status = nat.LIP_STATUS[res.status]
    if status == 'maxiter':
        warnings.warn("lip_constant: maxiter=%d Lanczos steps reached with residual %.3g (tol * theta = %.3g); "
                      "returning the best Ritz value" % (maxiter, res.residual, tol * res.theta), RuntimeWarning, stacklevel=2)
    theta = float(res.theta)
    value = math.sqrt(max(theta, 0.0)) if sqrt else theta
    if not return_info:
        return value
    info = dict(theta=theta, residual=float(res.residual), steps=int(res.steps), matvecs=int(res.matvecs),
                host_reads=int(res.host_reads), space=nat.LIP_SPACES[res.space], dim=int(res.dim), status=status,
                restarts=int(res.restarts), history=list(history[:min(res.steps, maxiter)]))
    return value, info


class LipBoundConv2d(torch.nn.Module):
    """Module form (lip_const.py:32-93): the geometry is fixed at construction, ``forward``
    takes the kernel."""

    def __init__(self, kernel_size, padding, stride=1, sample=50, sqrt=False):
        super().__init__()
        assert len(kernel_size) == 4                                        # :47
        _check(kernel_size, stride)
        self.ksize = kernel_size[-1]
        self.padding, self.sample, self.sqrt = padding, sample, sqrt

    def forward(self, kernel):
        assert kernel.dim() == 4                                            # :74
        assert kernel.size(2) == kernel.size(3) == self.ksize              # :75
        return lip_bound_conv2d(kernel, self.padding, sample=self.sample, sqrt=self.sqrt)
