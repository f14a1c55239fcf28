"""Mirror of lasso/linear/utils.py:1-58, the reference's numeric helpers: ``qr``, ``lstsq``, ``ridge`` and
``batch_cholesky_solve`` with its names, argument order and defaults.

``batch_cholesky_solve(b [B,D], A [B,D,D])`` solves one dense system per batch entry on the kernels of
csrc/batch_solve.hip.  The Cholesky route reads only the lower triangle of each ``A_i`` (as the reference's
``cholesky_ex`` does) and picks one of three kernels by ``D``: ``'wave'`` (``D <= WAVE_CAP``: one wave per system),
``'lds'`` (``D <= LDS_CAP[dtype]``: one workgroup, the packed triangle in LDS) and ``'general'`` (``D <= CAP[dtype]``:
``GENERAL_WORKGROUPS`` workgroups at most, their triangles in the scratch buffer).  If any system's factorisation meets
a pivot that is not positive (or NaN) the call warns with the reference's text and solves the WHOLE batch by LU with
partial pivoting, which reads the full matrices; a system that is singular there raises ``torch.linalg.LinAlgError``
with torch's text, naming the lowest such batch element; a NaN pivot is no error, that system's row comes back NaN.
Every system is solved on its own in a fixed order of operations: a row does not depend on the rest of the batch, and
two calls give the same bits.  The result is a new tensor on ``b``'s device; no input is modified; CPU tensors are
staged through the device.  ``return_info=True`` returns ``(x, info)`` with ``info = dict(route='cholesky' | 'lu',
tier, bad_system, bad_minor)``: the first system whose Cholesky factorisation failed and 1 + the index of its pivot
(``None`` on the Cholesky route).

float32 and float64.  Refused with NotImplementedError before any native call: bfloat16 and float16, mixed dtypes, ``D``
beyond ``CAP[dtype]`` and tensors that require grad under grad mode.  Shape mismatches are AssertionError like the
reference's asserts.

``ridge(b, A, alpha)`` and ``lstsq(b, A)`` run on the library's Gram and Cholesky kernels (csrc/mstep.hip, ridge.hip)
for float32 tensors outside an autograd graph with at most 4096 unknowns, and on torch.linalg otherwise;
``initialize_code`` calls them the way the reference does.  ``qr`` is the reference's shim around ``torch.linalg.qr``.
"""
import ctypes as C
import warnings

import torch

from .. import _native as nat

__all__ = ['qr', 'lstsq', 'ridge', 'batch_cholesky_solve']

TIERS = ('wave', 'lds', 'general')                                   # LASSO_BATCH_TIER_*
WAVE_CAP = 32                                                        # largest D of the wave tier
LDS_CAP = {torch.float32: 256, torch.float64: 160}                   # ... of the LDS tier
CAP = {torch.float32: 1024, torch.float64: 512}                      # ... of the general tier: the largest D at all
GENERAL_WORKGROUPS = 256                                             # workgroups of the general tier, at most


class BatchSolveResult(C.Structure):
    """lasso_batch_solve_result (include/lasso_hip.h)"""
    _fields_ = [('bad_system', C.c_int64), ('bad_minor', C.c_int32), ('tier', C.c_int32)]


def qr(A):
    """utils.py:5-10"""
    return torch.linalg.qr(A, mode='reduced')


def _engine_for(x, weight):
    from ..engine import HipEngine
    nat.require_gpu()
    return HipEngine(nat.pick_device(x, weight))


def _native_ok(x, weight):
    # the library's Gram / Cholesky kernels: fp32, no autograd graph, systems of at most 4096 unknowns
    return (x.dtype == torch.float32 and weight.dtype == torch.float32 and x.size(0) > 0
            and not (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)))


def _lstsq_qr(x, weight):
    # least-norm (d < k) / least-squares (d >= k) code through a reduced QR of the dictionary
    # (utils.py:13-25, the reference's own route): torch.linalg on the tensors' device
    d, k = weight.shape
    rhs = x.T
    if d < k:
        q, r = qr(weight.T)
        return (q @ torch.linalg.solve_triangular(r.T, rhs, upper=False)).T
    q, r = qr(weight)
    return torch.linalg.solve_triangular(r, q.T @ rhs, upper=True).T


def _lstsq_rows(x, weight):
    """the codes z [n,k] of the rows of x [n,d] for the dictionary weight [d,k]: lstsq(x.T, weight).T"""
    d, k = weight.shape
    if not _native_ok(x, weight) or min(d, k) > 4096:
        return _lstsq_qr(x, weight)
    eng = _engine_for(x, weight)
    xg, wg = eng.to_device(x), eng.to_device(weight)
    n = xg.shape[0]
    wt = wg.T.contiguous()                                       # [k,d]
    try:
        if d >= k:
            buf = torch.empty(k * k + k * n, dtype=torch.float32, device=eng.device)
            A, B = eng.gram(wg, xg.T.contiguous(), buf)          # A = W^T W [k,k], B = W^T x^T [k,n]
            z0 = eng.ridge(A, B, 0.0, check=True)                # [n,k]
            r = xg - eng.init_transpose(z0, wt)                  # x - z W^T  [n,d]
            A, B = eng.gram(wg, r.T.contiguous(), buf)
            z0 = z0 + eng.ridge(A, B, 0.0)
        else:
            buf = torch.empty(2 * d * d, dtype=torch.float32, device=eng.device)
            A, _ = eng.gram(wt, wt, buf)                         # A = W W^T [d,d]
            u = eng.ridge(A, xg.T.contiguous(), 0.0, check=True)  # ((W W^T)^-1 x^T)^T  [n,d]
            r = xg - eng.init_transpose(eng.init_transpose(u, wg), wt)      # x - (u W) W^T
            u = u + eng.ridge(A, r.T.contiguous(), 0.0)
            z0 = eng.init_transpose(u, wg)                       # u W  [n,k]
    except torch.linalg.LinAlgError:
        return _lstsq_qr(x, weight)
    return z0.to(x.device)


def lstsq(b, A):
    """utils.py:13-25: the least-squares (m >= n) or least-norm (m < n) solution x [n,r] of ``A x = b`` for A [m,n],
    b [m,r].  On the library's own kernels through the normal equations with ONE step of iterative refinement (the
    corrected semi-normal equations): m >= n: (A^T A) x = A^T b (Gram product + blocked Cholesky, csrc/mstep.hip and
    ridge.hip), then the same solve for the residual b - A x; m < n: x = A^T u, (A A^T) u = b, refined the same way.
    The refinement step brings the normal equations' cond(A)^2 error back to the level of the reference's QR route as
    long as cond(A)^2 * 2^-24 < 1 (measured against fp64: cond 3 -> 8e-7, cond 50 -> 3e-6, cond 560 -> 5e-6 of
    max|x|, QR: 8e-7 / 1e-6 / 3e-6); when the Cholesky factorisation meets a non-positive pivot -- a rank-deficient A
    -- the reference's QR route runs instead (torch.linalg on the device).  float64 tensors, tensors in an autograd
    graph and min(m, n) > 4096 take the QR route as well."""
    if A.dim() != 2 or b.dim() != 2:
        raise NotImplementedError("lasso_amd: lstsq takes a 2-D A [m,n] and a 2-D b [m,r] (the reference's only "
                                  "caller); batched operands are not implemented")
    assert b.shape[0] == A.shape[0]
    return _lstsq_rows(b.T, A).T


def _ridge_rows(x, weight, alpha):
    """the codes z [n,k] of the rows of x [n,d] for the dictionary weight [d,k]: ridge(x.T, weight, alpha).T"""
    d, k = weight.shape
    if not _native_ok(x, weight) or k > 4096:
        gram = weight.T @ weight
        gram.diagonal().add_(alpha)
        chol, info = torch.linalg.cholesky_ex(gram)
        if info != 0:
            raise RuntimeError("The Gram matrix is not positive definite. Try increasing 'alpha'.")
        return torch.cholesky_solve(weight.T @ x.T, chol).T
    eng = _engine_for(x, weight)
    xg, wg = eng.to_device(x), eng.to_device(weight)
    n = xg.shape[0]
    buf = torch.empty(k * k + k * n, dtype=torch.float32, device=eng.device)
    A, B = eng.gram(wg, xg.T.contiguous(), buf)
    try:
        z0 = eng.ridge(A, B, float(alpha), check=True)
    except torch.linalg.LinAlgError:
        raise RuntimeError("The Gram matrix is not positive definite. Try increasing 'alpha'.")   # utils.py:36-38
    return z0.to(x.device)


def ridge(b, A, alpha=1e-4):
    """utils.py:28-40: x [n,r] with (A^T A + alpha I) x = A^T b for A [m,n], b [m,r].  A^T A and A^T b are ONE launch
    of the Gram kernel (lasso_gram_accumulate with A in the role of the codes), the Cholesky factorisation and both
    triangular solves are lasso_ridge_solve (csrc/ridge.hip); float64 tensors, tensors in an autograd graph and
    n > 4096 go to torch.linalg.  A Gram matrix that is not positive definite raises the reference's RuntimeError."""
    assert A.dim() == 2 and b.dim() == 2 and b.shape[0] == A.shape[0]
    return _ridge_rows(b.T, A, alpha).T


def _tier_name(D, dtype):
    return 'wave' if D <= WAVE_CAP else 'lds' if D <= LDS_CAP[dtype] else 'general'


def batch_cholesky_solve(b, A, return_info=False):
    """Solve a batch of PSD linear systems, with a unique matrix A_k for each batch entry b_k (utils.py:43-58):
    b [B,D], A [B,D,D] -> x [B,D].  See the module's text for the routes, the tiers and the refusals."""
    assert b.dim() == 2  # [B,D]
    assert A.dim() == 3  # [B,D,D]
    nb, D = b.shape
    assert A.shape == (nb, D, D)
    for t in (b, A):
        if t.dtype not in CAP or t.dtype != b.dtype:
            raise NotImplementedError("lasso_amd: batch_cholesky_solve is implemented for float32 and float64 tensors "
                                      "of one dtype (got %s and %s)" % (b.dtype, A.dtype))
    dtype = b.dtype
    if torch.is_grad_enabled() and (b.requires_grad or A.requires_grad):
        raise NotImplementedError("lasso_amd: batch_cholesky_solve does not build an autograd graph; inputs that "
                                  "require grad (requires_grad=True) are not supported -- detach them")
    if D > CAP[dtype]:
        raise NotImplementedError("lasso_amd: batch_cholesky_solve takes systems of at most D = %d unknowns (the cap) in "
                                  "%s; got D = %d" % (CAP[dtype], dtype, D))
    if nb == 0 or D == 0:
        x = torch.empty((nb, D), dtype=dtype, device=b.device)
        info = dict(route='cholesky', tier=_tier_name(D, dtype), bad_system=None, bad_minor=None)
        return (x, info) if return_info else x
    nat.require_gpu()
    dev = nat.pick_device(b, A)
    ag = A.detach().to(device=dev)
    if ag.stride(2) != 1 or ag.stride(1) < D or ag.stride(0) < 0:
        ag = ag.contiguous()
    bg = b.detach().to(device=dev)
    if bg.stride(1) != 1 or bg.stride(0) < D:
        bg = bg.contiguous()
    x = torch.empty((nb, D), dtype=dtype, device=dev)
    res = BatchSolveResult()
    L = nat.lib()
    dt = nat.DT[dtype]
    with torch.cuda.device(dev):
        ws = nat.workspace(dev, L.lasso_batch_solve_workspace_bytes(nb, D, dt), "batch_solve")
        operands = (nat.ptr(ag), ag.stride(0), ag.stride(1), nat.ptr(bg), bg.stride(0), nat.ptr(x), x.stride(0), nb, D, dt,
                    C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
        nat.check(L.lasso_batch_chol_solve(*operands))
        info = dict(route='cholesky', tier=TIERS[res.tier], bad_system=None, bad_minor=None)
        if res.bad_system >= 0:
            info.update(route='lu', bad_system=int(res.bad_system), bad_minor=int(res.bad_minor))
            warnings.warn('Cholesky factorization failed. Reverting to LU '
                          'decomposition...')                            # utils.py:55-56
            nat.check(L.lasso_batch_lu_solve(*operands))
            if res.bad_system >= 0:
                raise torch.linalg.LinAlgError("torch.linalg.solve: (Batch element %d): The solver failed because the input "
                                               "matrix is singular." % res.bad_system)
    x = x.to(device=b.device)
    return (x, info) if return_info else x
