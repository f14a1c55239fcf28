"""Host model of the conjugate-gradient module (TEST INFRASTRUCTURE): a torch restatement, in this project's words, of
what lasso/conjgrad.py computes -- conjgrad() in the reference's order, and its three operators -- with knobs the
reference does not have:

  order_seed  an integer: the elements of every per-row dot and of every batch-wide sum are permuted before they are
              summed, and so is the contraction index of every product (the columns of A; the atoms that
              conv_transpose2d sums over and the channels that conv2d sums over): another summation order -- the
              reference's own BLAS and convolution kernels fix one, a GEMM on matrix cores another
  sum64       every per-row dot and every batch-wide sum is folded in double and rounded once to the tensors' dtype
              (the HIP path's choice)

With every knob off the arithmetic is the reference's operation for operation; the generator
(tests/golden/generate_golden_conjgrad.py) checks torch.equal against the real reference when it writes the fixture.
Every other setting is "another correct implementation" of the same dtype.  It runs on the device of its tensors, through
torch.mm / conv2d / conv_transpose2d: on a GPU it is the yardstick tools/bench_conjgrad.py times the HIP path against.
Every function returns (x, info); info carries status, iterations (the index of the iteration the exit fired in;
maxiter for status 4), termcond and the per-iteration lists r_abs, curv_sum, rs as doubles."""
import torch
import torch.nn.functional as F

MESSAGES = {0: 'Absolute tolerance reached.', 1: 'Relative tolerance reached.', 2: 'Curvature has converged.',
            3: 'Curvature is negative.', 4: 'Maximum iterations reached.'}


class _Sums:
    def __init__(self, order_seed, sum64):
        self.gen = None if order_seed is None else torch.Generator().manual_seed(int(order_seed))
        self.sum64 = sum64
        self.plain = order_seed is None and not sum64

    def _fold(self, flat):
        """sum over the last dim of a 2-D tensor"""
        if self.gen is not None:
            flat = flat[:, torch.randperm(flat.shape[1], generator=self.gen).to(flat.device)]
        if self.sum64:
            return flat.double().sum(1).to(flat.dtype)
        return flat.sum(1)

    def rows(self, t, dims):
        """the reference's dot: u.dot(v) for vectors (dims None), else the sum over dims, kept"""
        if self.plain:
            return t.sum() if dims is None else torch.sum(t, dims, keepdim=True)
        if dims is None:
            return self._fold(t.reshape(1, -1)).reshape(())
        return self._fold(t.reshape(t.shape[0], -1)).reshape([t.shape[0]] + [1] * (t.dim() - 1))

    def total(self, t):
        if self.plain:
            return t.sum()
        return self._fold(t.reshape(1, -1)).reshape(())


def conjgrad(b, Adot, dims, maxiter=None, tol=1e-10, rtol=1e-1, order_seed=None, sum64=False, record=True):
    """conjgrad.py:13-57; dims: what dot sums over (None: b is a vector)"""
    sums = _Sums(order_seed, sum64)
    if sums.plain and dims is None:
        dot = lambda u, v: u.dot(v)                                    # noqa: E731
    else:
        dot = lambda u, v: sums.rows(u * v, dims)                      # noqa: E731
    if maxiter is None:
        maxiter = 20 * (b.numel() if b.dim() == 1 else b[0].numel())
    b_abs = sums.total(b.abs())
    termcond = rtol * b_abs * b_abs.sqrt().clamp(0, 0.5)
    float_eps = torch.finfo(b.dtype).eps
    info = dict(status=4, iterations=maxiter, termcond=float(termcond), r_abs=[], curv_sum=[], rs=[])

    def done(status, i, x):
        info['status'], info['iterations'], info['message'] = status, i, MESSAGES[status]
        return x, info

    x = torch.zeros_like(b)
    r = -b
    p = b
    rs_old = dot(r, r)
    for i in range(maxiter):
        r_abs = sums.total(r.abs())
        if record:
            info['r_abs'].append(float(r_abs))
        if r_abs <= termcond:
            return done(1, i, x)
        Ap = Adot(p)
        curv = dot(p, Ap)
        curv_sum = sums.total(curv)
        if record:
            info['curv_sum'].append(float(curv_sum))
        if 0 <= curv_sum <= 3 * float_eps:
            return done(2, i, x)
        elif curv_sum < 0:
            if i == 0:
                x = - rs_old / curv * b
            return done(3, i, x)
        alpha = rs_old / curv
        x = x + alpha * p
        r = r + alpha * Ap
        rs_new = dot(r, r)
        rs = sums.total(rs_new).sqrt()
        if record:
            info['rs'].append(float(rs))
        if rs < tol:
            return done(0, i, x)
        p = - r + (rs_new / rs_old) * p
        rs_old = rs_new
    return done(4, maxiter, x)


def _perm(gen, n, like):
    return torch.randperm(n, generator=gen).to(like.device)


def _product_gen(order_seed):
    return None if order_seed is None else torch.Generator().manual_seed(7919 + int(order_seed))


def cg(A, b, maxiter=None, tol=1e-10, rtol=1.0, order_seed=None, **knobs):
    assert A.dim() == 2 and b.dim() == 1
    if maxiter is None:
        maxiter = 20 * len(b)
    gen = _product_gen(order_seed)

    def Adot(v):
        if gen is None:
            return A.matmul(v)
        p = _perm(gen, v.shape[0], v)
        return A[:, p].contiguous().matmul(v[p].contiguous())

    return conjgrad(b, Adot, None, maxiter, tol, rtol, order_seed=order_seed, **knobs)


def batch_cg(A, b, maxiter=None, tol=1e-10, rtol=1.0, order_seed=None, **knobs):
    assert A.dim() == 2 and b.dim() == 2
    if maxiter is None:
        maxiter = 20 * b.size(1)
    At = A.T
    gen = _product_gen(order_seed)

    def Adot(v):
        if gen is None:
            return torch.mm(v, At)
        p = _perm(gen, v.shape[1], v)
        return torch.mm(v[:, p].contiguous(), At[p].contiguous())

    return conjgrad(b, Adot, 1, maxiter, tol, rtol, order_seed=order_seed, **knobs)


def adot_conv2d(kernel, v, tik=0, gen=None, **conv_kwargs):
    if gen is None:
        Av = F.conv_transpose2d(v, kernel, **conv_kwargs)
        Av = F.conv2d(Av, kernel, **conv_kwargs)
    else:
        pk, pc = _perm(gen, kernel.shape[0], v), _perm(gen, kernel.shape[1], v)
        Av = F.conv_transpose2d(v[:, pk].contiguous(), kernel[pk].contiguous(), **conv_kwargs)
        Av = F.conv2d(Av[:, pc].contiguous(), kernel[:, pc].contiguous(), **conv_kwargs)
    if tik > 0:
        Av = Av + tik * v
    return Av


def batch_cg_conv2d(kernel, b, tik=0, maxiter=None, tol=1e-10, rtol=1.0, order_seed=None, sum64=False, record=True,
                    **conv_kwargs):
    assert kernel.dim() == 4 and b.dim() == 4
    if maxiter is None:
        maxiter = 20 * b[0].numel()
    gen = _product_gen(order_seed)
    return conjgrad(b, lambda v: adot_conv2d(kernel, v, tik, gen, **conv_kwargs), [1, 2, 3], maxiter, tol, rtol,
                    order_seed=order_seed, sum64=sum64, record=record)


# "another correct implementation" of the same dtype: the variants whose distance from the reference's run is the spread
def variants(order_seeds):
    return [dict(sum64=True)] + [dict(order_seed=s) for s in order_seeds] + [dict(order_seed=s, sum64=True) for s in order_seeds]
