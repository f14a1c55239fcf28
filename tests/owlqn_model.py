"""Host model of the OWL-QN solver (TEST INFRASTRUCTURE): a torch restatement, in this project's words, of what
lasso/nonlinear/owlqn.py computes for fun(z) = 0.5 |z W^T - x|^2, with three knobs the reference does not have:

  dtype       the precision everything runs in (float32: the reference's own arithmetic; float64: the yardstick)
  accurate_f  fold the objective (and the backtracking's inner product) in double and hand it on un-rounded, as the
              HIP path does, instead of as a value of ``dtype``
  order_seed  None: the reference's operation order.  An integer: "another correct implementation" -- the contraction
              index of every product is permuted (another summation order) AND the direction comes from the
              vector-free form of the two-loop recursion (dots in double, the recursion on S^T Y, Y^T Y, S^T v, Y^T v,
              one combination rounded once)

With float32, accurate_f=False and order_seed=None the arithmetic is the reference's operation for operation; the
generator (tests/golden/generate_golden_owlqn.py) checks torch.equal against the real reference when it writes the
fixture.  The Brent arm needs scipy, imported when it is used.  Returns (z, info); info also carries every decision:
``decisions`` (f_new, bound, f) of each backtracking trial and ``curvature`` (iteration, y.s) of each memory update,
so that a test can tell whether rounding could flip one (``assert_robust``)."""
import warnings

import torch

LS_DEFAULTS = dict(tol=0.1, decay=0.95, maxiter=500)
CURV_MIN = 1e-10


def keep_sign(u, w):
    """u where sign(u) == sign(w), an exact zero elsewhere"""
    return u.masked_fill(u.sign() != w.sign(), 0)


def pseudo_gradient(z, g, alpha):
    """the right derivative where it is negative, the left where it is positive, else 0"""
    reg = alpha * z.sign()
    right = g + reg.masked_fill(z == 0, alpha)
    left = g + reg.masked_fill(z == 0, -alpha)
    pg = torch.zeros_like(z)
    pg = torch.where(right < 0, right, pg)
    return torch.where(left > 0, left, pg)


class Memory:
    """L_BFGS of owlqn.py:8-51: lists of flattened pairs, oldest first"""

    def __init__(self, z, g, history_size, vector_free):
        self.s, self.y, self.rho = [], [], []
        self.h_diag = 1.
        self.alpha = z.new_empty(history_size)
        self.history_size, self.vector_free = history_size, vector_free
        self.z_prev, self.g_prev = z.clone(), g.clone()

    def solve(self, v):
        return self.solve_vector_free(v) if self.vector_free else self.solve_two_loop(v)

    def solve_two_loop(self, v):
        m = len(self.y)
        q = v.reshape(-1).clone()
        for i in reversed(range(m)):
            self.alpha[i] = self.s[i].dot(q) * self.rho[i]
            q.add_(self.y[i], alpha=-self.alpha[i])
        q.mul_(self.h_diag)
        for i in range(m):
            beta = self.y[i].dot(q) * self.rho[i]
            q.add_(self.s[i], alpha=self.alpha[i] - beta)
        return q.view(v.shape)

    def solve_vector_free(self, v):
        """H v = gamma v + sum c_i s_i + sum e_i y_i from the small arrays alone, everything in double"""
        m = len(self.y)
        q = v.reshape(-1).double()
        if m == 0:
            return v.clone()
        S, Y = torch.stack(self.s).double(), torch.stack(self.y).double()
        sy, yy, sv, yv = S @ Y.T, Y @ Y.T, S @ q, Y @ q          # sy[i, j] = s_i . y_j
        gamma = float(sy[m - 1, m - 1] / yy[m - 1, m - 1])
        a, c = [0.0] * m, [0.0] * m
        for i in reversed(range(m)):
            a[i] = float(sv[i] - sum(a[j] * sy[i, j] for j in range(i + 1, m))) / float(sy[i, i])
        for i in range(m):
            yq = float(yv[i]) - sum(a[j] * float(yy[i, j]) for j in range(m))
            b = (gamma * yq + sum(c[j] * float(sy[j, i]) for j in range(i))) / float(sy[i, i])
            c[i] = a[i] - b
        out = gamma * q
        for i in range(m):
            out = out + c[i] * S[i] - gamma * a[i] * Y[i]
        return out.to(v.dtype).view(v.shape)

    def update(self, z, g):
        """-> (kept, y.s)"""
        s = (z - self.z_prev).view(-1)
        y = (g - self.g_prev).view(-1)
        ys = y.dot(s)
        if ys <= CURV_MIN:
            return False, float(ys)
        if len(self.y) == self.history_size:
            self.y.pop(0)
            self.s.pop(0)
            self.rho.pop(0)
        self.y.append(y)
        self.s.append(s)
        self.rho.append(ys.reciprocal())
        self.h_diag = ys / y.dot(y)
        self.z_prev.copy_(z)
        self.g_prev.copy_(g)
        return True, float(ys)


class Model:
    def __init__(self, weight, x, alpha, dtype=torch.float32, accurate_f=False, order_seed=None):
        self.w = weight.detach().to(dtype)
        self.x = x.detach().to(dtype)
        self.alpha, self.dtype, self.accurate_f = alpha, dtype, accurate_f
        self.gen = None if order_seed is None else torch.Generator().manual_seed(int(order_seed))

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
        return 0.5 * resid.pow(2).sum() + self.alpha * z.norm(p=1), resid

    def evaluate(self, z):
        """-> (f, g, pg)"""
        f, resid = self.objective(z)
        g = self.mm(resid, self.w)
        return f, g, pseudo_gradient(z, g, self.alpha)

    def step(self, z, t, d, eta):
        return keep_sign(z.add(d, alpha=t), eta)

    def inner(self, v, dz):
        return float(v.double().mul(dz.double()).sum()) if self.accurate_f else v.mul(dz).sum()


def owlqn(weight, x, z0, alpha=1., lr=1, max_iter=20, xtol=1e-5, history_size=100, line_search='brent', ls_options=None,
          dtype=torch.float32, accurate_f=False, order_seed=None):
    assert z0.dim() == 2
    if line_search not in ('brent', 'backtrack', 'none'):
        raise RuntimeError
    ls = dict(LS_DEFAULTS, **(ls_options or {}))
    m = Model(weight, x, alpha, dtype, accurate_f, order_seed)
    z = z0.detach().to(dtype)
    f, g, pg = m.evaluate(z)
    info = dict(iterations=0, f0=float(f), t=[], ls_iters=[], objective=[], delta_x=[], evaluations=[], decisions=[],
                curvature=[], pairs=[], skipped=[], H_diag=[], warnings=[])
    mem = Memory(z, g, history_size, order_seed is not None)
    t = torch.clamp(lr / pg.norm(p=1), max=lr)
    for it in range(1, max_iter + 1):
        v = pg.neg()
        d = keep_sign(mem.solve(v), v)
        eta = torch.where(z == 0, v.sign(), z.sign())
        if line_search == 'brent':
            from scipy.optimize import minimize_scalar

            def line(tt):
                ft = float(m.objective(m.step(z, tt, d, eta))[0])
                info['evaluations'].append((it, float(tt), ft))
                return ft
            found = minimize_scalar(line, bounds=(0, 10), method='bounded')
            t, trials = found.x, found.nfev
        elif line_search == 'backtrack':
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
            trials = 0
        z_new = m.step(z, t, d, eta)
        delta = torch.norm(z_new - z, p=2)
        z = z_new
        f, g, pg = m.evaluate(z)
        info['iterations'] = it
        info['t'].append(float(t))
        info['ls_iters'].append(int(trials))
        info['objective'].append(float(f))
        info['delta_x'].append(float(delta))
        stop = bool(delta <= xtol)
        skipped = False
        if not stop:
            kept, ys = mem.update(z, g)
            skipped = not kept
            info['curvature'].append((it, ys))
            t = lr
        info['pairs'].append(len(mem.y))
        info['skipped'].append(skipped)
        info['H_diag'].append(float(mem.h_diag))
        if stop:
            break
    return z, info


def assert_robust(info):
    """no decision of the run is close enough to its threshold for rounding to flip it: every backtracking test at least
    1e-4 |f| from its bound, every y.s a factor 10 from 1e-10"""
    for fn, bound, f in info['decisions']:
        assert abs(fn - bound) >= 1e-4 * abs(f), "a backtracking decision that rounding could flip: %r" % ((fn, bound, f),)
    for it, ys in info['curvature']:
        assert ys >= 10 * CURV_MIN or ys <= CURV_MIN / 10, "y.s = %r at iteration %d is within 10x of 1e-10" % (ys, it)


def first_line_objective(weight, x, z0, alpha, dtype=torch.float64, accurate_f=True):
    """t -> f(project(z0 + t d, eta)) of the first iteration's line search (d = v: the memory is empty), in ``dtype``"""
    m = Model(weight, x, alpha, dtype, accurate_f, None)
    z = z0.detach().to(dtype)
    _, _, pg = m.evaluate(z)
    v = pg.neg()
    eta = torch.where(z == 0, v.sign(), z.sign())
    return lambda t: float(m.objective(m.step(z, float(t), v.clone(), eta))[0])


def objective64(weight, x, z, alpha):
    """the objective of a code, in double"""
    r = torch.mm(z.double(), weight.double().T) - x.double()
    return 0.5 * float(r.square().sum()) + alpha * float(z.double().abs().sum())
