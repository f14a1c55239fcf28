"""Host model of the orthant-wise Newton solver (TEST INFRASTRUCTURE): a torch restatement, in this project's words,
of what lasso/linear/solvers/orthant_wise_newton.py computes, with three knobs the reference does not have:

  dtype       the precision everything runs in (float32: the reference's own arithmetic; float64: the yardstick)
  accurate_f  fold the objective (and the backtracking's inner product) in double and hand it on un-rounded, as the
              HIP path does, instead of as a value of ``dtype``
  order_seed  None: the reference's operation order.  An integer: "another correct implementation" -- the contraction
              index of every product is permuted (another summation order) and Hinv comes from a float64
              factorisation rounded once to ``dtype``

With float32, accurate_f=False and order_seed=None the arithmetic is the reference's operation for operation; the
generator (tests/golden/generate_golden_own.py) checks torch.equal against the real reference when it writes the
fixture.  The Brent arm needs scipy, imported when it is used.  Returns (z, info); info also carries every backtracking
decision (f_new, bound, f) so that a test can tell whether rounding could flip one."""
import warnings

import torch

LS_DEFAULTS = dict(tol=0.1, decay=0.95, maxiter=500)
SHIFT = 1e-4


def keep_sign(u, w):
    """u where sign(u) == sign(w), an exact zero elsewhere"""
    return torch.where(u.sign() == w.sign(), u, torch.zeros_like(u))


def pseudo_gradient(z, g, alpha):
    """the right derivative where it is negative, the left where it is positive, else 0"""
    at_zero = z == 0
    reg = alpha * z.sign()
    right = g + torch.where(at_zero, torch.full_like(z, alpha), reg)
    left = g + torch.where(at_zero, torch.full_like(z, -alpha), reg)
    pg = torch.zeros_like(z)
    pg = torch.where(right < 0, right, pg)
    return torch.where(left > 0, left, pg)


class Model:
    def __init__(self, weight, x, alpha, dtype=torch.float32, accurate_f=False, order_seed=None):
        self.w = weight.detach().to(dtype)
        self.x = x.detach().to(dtype)
        self.alpha, self.dtype, self.accurate_f = alpha, dtype, accurate_f
        self.gen = None if order_seed is None else torch.Generator().manual_seed(int(order_seed))
        h = self.mm(self.w.T, self.w)
        h.diagonal().add_(SHIFT)
        if order_seed is None:
            self.hinv = torch.cholesky_inverse(torch.linalg.cholesky(h))
        else:
            h64 = torch.mm(self.w.double().T, self.w.double())
            h64.diagonal().add_(SHIFT)
            self.hinv = torch.cholesky_inverse(torch.linalg.cholesky(h64)).to(dtype)

    def mm(self, a, b):
        if self.gen is None:
            return torch.mm(a, b)
        p = torch.randperm(a.shape[1], generator=self.gen)
        return torch.mm(a[:, p].contiguous(), b[p].contiguous())

    def objective(self, z):
        """-> (f, resid); f a 0-dim tensor of dtype, or a python float folded in double"""
        resid = self.mm(z, self.w.T) - self.x
        if self.accurate_f:
            return 0.5 * float(resid.double().square().sum()) + self.alpha * float(z.double().abs().sum()), resid
        return 0.5 * resid.square().sum() + self.alpha * z.norm(p=1), resid

    def evaluate(self, z):
        f, resid = self.objective(z)
        return f, pseudo_gradient(z, self.mm(resid, self.w), self.alpha)

    def direction(self, z, pg):
        """-> (v, d, eta)"""
        v = pg.neg()
        d = keep_sign(self.mm(v, self.hinv.T), v)
        return v, d, torch.where(z == 0, v.sign(), z.sign())

    def step(self, z, t, d, eta):
        return keep_sign(z.add(d, alpha=t), eta)

    def inner(self, v, dz):
        return float(v.double().mul(dz.double()).sum()) if self.accurate_f else v.mul(dz).sum()


def orthant_wise_newton(weight, x, z0, alpha=1., lr=1., maxiter=20, xtol=1e-5, line_search='brent', ls_options=None,
                        dtype=torch.float32, accurate_f=False, order_seed=None):
    assert z0.dim() == 2
    if line_search not in ('brent', 'backtrack', 'none'):
        raise ValueError("line_search must be one of {'brent', 'backtrack', 'none'}.")
    ls = dict(LS_DEFAULTS, **(ls_options or {}))
    m = Model(weight, x, alpha, dtype, accurate_f, order_seed)
    z = z0.detach().to(dtype)
    f, pg = m.evaluate(z)
    info = dict(iterations=0, f0=float(f), t=[], ls_iters=[], objective=[], delta_z=[], evaluations=[], decisions=[],
                warnings=[])
    for it in range(1, maxiter + 1):
        v, d, eta = m.direction(z, pg)
        if line_search == 'brent':
            from scipy.optimize import minimize_scalar

            def line(t):
                ft = float(m.objective(m.step(z, t, d, eta))[0])
                info['evaluations'].append((it, float(t), ft))
                return ft
            found = minimize_scalar(line, bounds=(0, 10), method='bounded')
            t, trials = found.x, found.nfev
        elif line_search == 'backtrack':
            t = lr
            for trials in range(1, ls['maxiter'] + 1):
                z_new = m.step(z, t, d, eta)
                f_new = m.objective(z_new)[0]
                bound = f - ls['tol'] * m.inner(v, z_new - z)
                info['evaluations'].append((it, float(t), float(f_new)))
                info['decisions'].append((float(f_new), float(bound), float(f)))
                if f_new <= bound:
                    break
                t = t * ls['decay']
            else:
                warnings.warn('line search did not converge.')
                info['warnings'].append('line search did not converge.')
        else:
            t, trials = lr, 0
        z_new = m.step(z, t, d, eta)
        delta = torch.norm(z_new - z, p=2)
        z = z_new
        f, pg = m.evaluate(z)
        info['iterations'] = it
        info['t'].append(float(t))
        info['ls_iters'].append(int(trials))
        info['objective'].append(float(f))
        info['delta_z'].append(float(delta))
        if delta <= xtol:
            break
    return z, info


def first_line_objective(weight, x, z0, alpha, dtype=torch.float64, accurate_f=True):
    """t -> f(project(z0 + t d, eta)) of the first iteration's line search, in ``dtype``"""
    m = Model(weight, x, alpha, dtype, accurate_f, None)
    z = z0.detach().to(dtype)
    _, pg = m.evaluate(z)
    _, d, eta = m.direction(z, pg)
    return lambda t: float(m.objective(m.step(z, float(t), d, eta))[0])


def objective64(weight, x, z, alpha):
    """the objective of a code, in double"""
    r = torch.mm(z.double(), weight.double().T) - x.double()
    return 0.5 * float(r.square().sum()) + alpha * float(z.double().abs().sum())
