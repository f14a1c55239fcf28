"""lip_constant as a host model: plain Lanczos with full reorthogonalisation (classical Gram-Schmidt done twice) on
torch's conv2d / conv_transpose2d on the CPU, the algorithm of csrc/conv_lanczos.hip written independently of it -- the
tridiagonal problems go through numpy's dense symmetric eigensolver, not through csrc/lanczos_host.hpp.

Knobs give the spread of "another correct implementation": ``order_seed`` permutes the summation order of every dot,
``fold64`` accumulates the dots of a float32 run in double, ``start_seed`` takes another start vector, ``space`` forces
the space iterated.  ``variants()`` lists the combinations the fixture generator measures."""
import math

import numpy as np
import torch
import torch.nn.functional as F

STATUS = ("converged", "breakdown", "maxiter", "nonfinite")


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def geometry(kernel, imsize, transpose, stride, padding):
    """(image size, code size) of the operator ``imsize`` and ``transpose`` name; ValueError if it does not round-trip"""
    _, _, kh, kw = kernel.shape
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    H, W = (int(v) for v in imsize)
    if transpose:
        return ((H - 1) * sh - 2 * ph + kh, (W - 1) * sw - 2 * pw + kw), (H, W)
    eh, ew = H + 2 * ph - kh, W + 2 * pw - kw
    if eh < 0 or ew < 0 or eh % sh or ew % sw:
        raise ValueError("the image size does not round-trip")
    return (H, W), (eh // sh + 1, ew // sw + 1)


def _dot(a, b, perm, fold64):
    if perm is not None:
        a, b = a[perm], b[perm]
    if fold64:
        return float((a.double() * b.double()).sum())
    return float((a * b).sum())


def variants(order_seeds):
    out = [dict(order_seed=s) for s in order_seeds]
    out += [dict(fold64=True), dict(fold64=True, order_seed=order_seeds[0]), dict(start_seed=1), dict(start_seed=2, fold64=True)]
    return out


@torch.no_grad()
def lip_constant(kernel, imsize, transpose=False, sqrt=False, *, tol=None, maxiter=None, return_info=False,
                 order_seed=None, fold64=False, start_seed=0, space=None, **kwargs):
    stride, padding = kwargs.get("stride", 1), kwargs.get("padding", 0)
    K, C = kernel.shape[:2]
    (H, W), (Hz, Wz) = geometry(kernel, imsize, transpose, stride, padding)
    dtype = kernel.dtype
    eps = float(torch.finfo(dtype).eps)
    dim_image, dim_code = C * H * W, K * Hz * Wz
    if space is None:
        space = "code" if dim_code < dim_image else "image"
    dim = dim_code if space == "code" else dim_image
    named = K * int(imsize[0]) * int(imsize[1]) if transpose else C * int(imsize[0]) * int(imsize[1])
    tol = (1e-5 if dtype == torch.float32 else 1e-10) if tol is None else float(tol)
    maxiter = min(named, 512) if maxiter is None else int(maxiter)
    ck = dict(stride=stride, padding=padding)

    def apply(v):
        if space == "code":
            return F.conv2d(F.conv_transpose2d(v.view(1, K, Hz, Wz), kernel, **ck), kernel, **ck).reshape(-1)
        return F.conv_transpose2d(F.conv2d(v.view(1, C, H, W), kernel, **ck), kernel, **ck).reshape(-1)

    g = torch.Generator().manual_seed(1234 + start_seed)
    q = (torch.rand(dim, generator=g, dtype=torch.float64) * 2 - 1).to(dtype)
    perm = torch.randperm(dim, generator=torch.Generator().manual_seed(order_seed)) if order_seed is not None else None
    fold = fold64 and dtype == torch.float32
    Q = [q / math.sqrt(_dot(q, q, perm, fold))]
    alpha, beta, history = [], [], []
    status, theta, resid = "maxiter", float("nan"), float("nan")
    steps = 0
    for j in range(min(maxiter, dim)):
        w = apply(Q[j])
        a = 0.0
        for _ in range(2):
            c = [_dot(qi, w, perm, fold) for qi in Q]
            for ci, qi in zip(c, Q):
                w = w - ci * qi
            a += c[j]
        b = math.sqrt(_dot(w, w, perm, fold))
        alpha.append(a)
        beta.append(b)
        steps = j + 1
        if not (math.isfinite(a) and math.isfinite(b)):
            status, theta, resid = "nonfinite", float("nan"), float("nan")
            break
        T = np.diag(np.array(alpha)) + np.diag(np.array(beta[:-1]), 1) + np.diag(np.array(beta[:-1]), -1)
        lam, vec = np.linalg.eigh(T)
        theta, resid = float(lam[-1]), b * abs(float(vec[-1, -1]))
        history.append(theta)
        if b <= eps * abs(theta) or steps >= dim:
            status = "breakdown"
            break
        if resid <= tol * abs(theta):
            status = "converged"
            break
        Q.append(w / b)
    value = math.sqrt(max(theta, 0.0)) if sqrt else theta
    if not return_info:
        return value
    return value, dict(theta=theta, residual=resid, steps=steps, matvecs=steps, space=space, dim=dim, status=status,
                       history=history)


@torch.no_grad()
def fista_loss(x, weight, alpha, lr, iters, stride=1, padding=0):
    """conv_loss after ``iters`` FISTA iterations from z0 = 0 with the fixed step lr (ista.py:7-49 with tol = 0)"""
    ck = dict(stride=stride, padding=padding)
    z = torch.zeros_like(F.conv2d(x, weight, **ck))
    y, t = z, 1.0
    for _ in range(iters):
        grad = F.conv2d(F.conv_transpose2d(y, weight, **ck) - x, weight, **ck)
        z_next = F.softshrink(y - lr * grad, alpha * lr)
        t_next = (1 + math.sqrt(1 + 4 * t * t)) / 2
        y = z_next + ((t - 1) / t_next) * (z_next - z)
        z, t = z_next, t_next
    r = F.conv_transpose2d(z, weight, **ck) - x
    return float((0.5 * r.pow(2).sum() + alpha * z.abs().sum()) / x.shape[0])
