"""Host model of the Split Bregman solver (TEST INFRASTRUCTURE): a torch restatement, in this project's words, of what
lasso/linear/solvers/split_bregman.py computes, with knobs the reference does not have:

  dtype       the precision everything runs in (float32: the reference's own arithmetic; float64: the yardstick)
  row_major   False: the reference's layout -- the state is [k,n], every product is ``Hinv @ T``.  True: the state is
              [n,k] and every product is ``T @ Hinv^T``, as the HIP path computes it (another summation order inside
              the BLAS, the same mathematics: H is symmetric)
  hinv64      Hinv from a float64 Gram and factorisation, rounded once to ``dtype`` (the HIP path's choice)
  order_seed  an integer: the contraction index of every product is permuted (another summation order)

With float32 and every knob off the arithmetic is the reference's operation for operation; the generator
(tests/golden/generate_golden_split_bregman.py) checks torch.equal against the real reference when it writes the
fixture.  Every other setting is "another correct float32 implementation".  Returns (x [n,k], itn, info); info carries
iterations, stopped, the update of every executed outer iteration as a double and, with ``iterates=True``, a copy of X
[n,k] after every outer iteration."""
import torch
import torch.nn.functional as F


def objective64(A, y, x, alpha):
    """0.5 |x A^T - y|^2 + alpha |x|_1 in double"""
    r = torch.mm(x.double(), A.double().T) - y.double()
    return 0.5 * float(r.square().sum()) + alpha * float(x.double().abs().sum())


def split_bregman(A, y, x0=None, alpha=1.0, lambd=1.0, maxiter=20, niter_inner=5, tol=1e-10, tau=1., dtype=torch.float32,
                  row_major=False, hinv64=False, order_seed=None, iterates=False):
    assert y.dim() == 2 and A.dim() == 2 and y.shape[1] == A.shape[0]
    d, k = A.shape
    n = y.shape[0]
    A = A.detach().to(dtype)
    y = y.detach().to(dtype)
    gen = None if order_seed is None else torch.Generator().manual_seed(int(order_seed))

    def mm(a, b):
        if gen is None:
            return torch.mm(a, b)
        p = torch.randperm(a.shape[1], generator=gen)
        return torch.mm(a[:, p].contiguous(), b[p].contiguous())

    # the state in the reference's layout [k,n], or transposed
    yt = y.T.contiguous()
    if x0 is None:
        x = y.new_zeros(k, n)
    else:
        assert x0.shape == (n, k)
        x = x0.detach().to(dtype).T.clone(memory_format=torch.contiguous_format)
    aty = mm(A.T, yt) / alpha
    if hinv64:
        h = torch.mm(A.double().T, A.double()) / alpha
        h.diagonal().add_(lambd)
        hinv = torch.cholesky_inverse(torch.linalg.cholesky(h)).to(dtype)
    else:
        h = mm(A.T, A) / alpha
        h.diagonal().add_(lambd)
        hinv = torch.cholesky_inverse(torch.linalg.cholesky(h))
    if row_major:
        x, aty = x.T.contiguous(), aty.T.contiguous()
    b = torch.zeros_like(x)
    dd = torch.zeros_like(x)
    update = y.new_tensor(float('inf'))
    info = dict(iterations=0, stopped=False, update=[], iterates=[])
    itn = 0
    for itn in range(maxiter):
        if update <= tol:
            info['stopped'] = True
            break
        xold = x.clone()
        for _ in range(niter_inner):
            t = aty.add(dd - b, alpha=lambd)
            x = mm(t, hinv.T) if row_major else mm(hinv, t)
            dd = F.softshrink(x + b, 1 / lambd)
        b.add_(x - dd, alpha=tau)
        update = torch.norm(x - xold)
        info['iterations'] += 1
        info['update'].append(float(update.double()))
        if iterates:
            info['iterates'].append((x if row_major else x.T).clone())
    x = x.contiguous() if row_major else x.T.contiguous()
    return x, itn, info


# "another correct float32 implementation": the variants whose distance from the reference's float32 run is the spread
def variants(order_seeds):
    out = [dict(row_major=True), dict(hinv64=True), dict(row_major=True, hinv64=True)]
    for s in order_seeds:
        out.append(dict(order_seed=s))
        out.append(dict(row_major=True, hinv64=True, order_seed=s))
    return out
