"""Host model of the BFGS iterated-ridge solver (TEST INFRASTRUCTURE): a torch restatement, in this project's words, of
what lasso/nonlinear/iterative_ridge_bfgs.py computes for f(z) = 0.5 |z W^T - x|^2, with two knobs the reference does
not have:

  dtype       the precision everything runs in (float32: the reference's own arithmetic; float64: the yardstick)
  order_seed  None: the reference's operation order.  An integer: "another correct float32 implementation" -- the
              contraction index of every product is permuted (another summation order), y.s, y.y, B s and s^T B s are
              summed in double and rounded once, the update is the symmetric form (B + rho (y_i y_j)) - (Bs_i Bs_j) /
              (s^T B s), the objective is folded in double and the line objective is the quadratic form
              0.5 (|r|^2 - 2 t <r,q> + t^2 |q|^2) + alpha |z - t d|_1 with q = d W^T

With float32 and order_seed=None the arithmetic is the reference's operation for operation; the generator
(tests/golden/generate_golden_irbfgs.py) checks torch.equal against the real reference when it writes the fixture.
The Brent arm needs scipy, imported when it is used.  Returns (z, info); info carries per iteration t, ls_iters,
objective, delta_x, whether the LU route ran and -- per update -- every row's y.s (``curvature``: (iteration, [n]
values)) and the count of invalid rows (-1: no update followed), so that a test can tell whether rounding could flip a
decision (``assert_robust``)."""
import warnings

import torch

CURV_MIN = 1e-10
LU_WARNING = 'Cholesky factorization failed. Reverting to LU decomposition...'


def batch_solve(rhs, A, info):
    """batch_cholesky_solve of lasso/linear/utils.py:43-58: Cholesky of every system, LU of the whole batch if one fails"""
    b = rhs.unsqueeze(2)
    L, bad = torch.linalg.cholesky_ex(A)
    if torch.all(bad == 0):
        info['lu'].append(False)
        return torch.cholesky_solve(b, L).squeeze(2)
    warnings.warn(LU_WARNING)
    info['warnings'].append(LU_WARNING)
    info['lu'].append(True)
    return torch.linalg.solve(A, b).squeeze(2)


class Model:
    def __init__(self, weight, x, alpha, dtype=torch.float32, order_seed=None):
        self.w = weight.detach().to(dtype)
        self.x = x.detach().to(dtype)
        self.alpha, self.dtype = alpha, dtype
        self.seeded = order_seed is not None
        self.gen = None if order_seed is None else torch.Generator().manual_seed(int(order_seed))

    def mm(self, a, b):
        if self.gen is None:
            return torch.mm(a, b)
        p = torch.randperm(a.shape[1], generator=self.gen)
        return torch.mm(a[:, p].contiguous(), b[p].contiguous())

    def smooth(self, z):
        """-> (f without the penalty, resid)"""
        resid = self.mm(z, self.w.T) - self.x
        if self.seeded:
            return 0.5 * float(resid.double().square().sum()), resid
        return 0.5 * resid.pow(2).sum(), resid

    def evaluate(self, z):
        """-> (fval = f + alpha |z|_1, grad of f, resid)"""
        f, resid = self.smooth(z)
        g = self.mm(resid, self.w)
        if self.seeded:
            return f + self.alpha * float(z.double().abs().sum()), g, resid
        return f + self.alpha * z.norm(p=1), g, resid


class Hessians:
    """BFGS of iterative_ridge_bfgs.py:9-42: one estimate per batch row"""

    def __init__(self, z, g, symmetric):
        self.B = torch.diag_embed(torch.ones_like(z))
        self.z_prev, self.g_prev = z.clone(), g.clone()
        self.n_updates = 0
        self.symmetric = symmetric

    def update(self, z, g):
        """-> (y.s per row [n], valid per row [n])"""
        s = (z - self.z_prev).unsqueeze(2)
        y = (g - self.g_prev).unsqueeze(2)
        if self.symmetric:
            ys, valid = self._update_symmetric(s, y)
        else:
            rho_inv = torch.bmm(y.transpose(1, 2), s)
            valid = rho_inv.abs().gt(CURV_MIN)
            rho = torch.where(valid, rho_inv.reciprocal(), torch.full_like(rho_inv, 1000.))
            if self.n_updates == 0:
                self.B.mul_(rho * torch.bmm(y.transpose(1, 2), y))
            Bs = torch.bmm(self.B, s)
            self.B = torch.where(
                valid,
                torch.addcdiv(torch.baddbmm(self.B, rho * y, y.transpose(1, 2)), torch.bmm(Bs, Bs.transpose(1, 2)),
                              torch.bmm(s.transpose(1, 2), Bs), value=-1),
                self.B)
            ys = rho_inv
        self.z_prev.copy_(z)
        self.g_prev.copy_(g)
        self.n_updates += 1
        return ys.reshape(-1).double(), valid.reshape(-1)

    def _update_symmetric(self, s, y):
        dt = s.dtype
        sd, yd = s.double(), y.double()
        ys = (yd * sd).sum(1, keepdim=True).to(dt)
        yy = (yd * yd).sum(1, keepdim=True).to(dt)
        valid = ys.abs().gt(CURV_MIN)
        rho = torch.where(valid, ys.reciprocal(), torch.full_like(ys, 1000.))
        if self.n_updates == 0:
            self.B.mul_(rho * yy)
        Bs = torch.bmm(self.B.double(), sd).to(dt)
        sBs = (sd * Bs.double()).sum(1, keepdim=True).to(dt)
        new = (self.B + rho * (y * y.transpose(1, 2))) - (Bs * Bs.transpose(1, 2)) / sBs
        self.B = torch.where(valid, new, self.B)
        return ys, valid


def masked_system(B, z, g, alpha, tikhonov, eps):
    """-> (system [n,k,k], rhs [n,k], is_zero [n,k]) of iterative_ridge_bfgs.py:101-108"""
    zmag = z.abs()
    is_zero = zmag < eps
    diag = (alpha / zmag).masked_fill(is_zero, 0)
    rhs = (g + diag * z).masked_fill(is_zero, 0)
    A = B.masked_fill((is_zero.unsqueeze(1) | is_zero.unsqueeze(2)), 0.)
    A.diagonal(dim1=1, dim2=2).add_(diag + tikhonov)
    return A, rhs, is_zero


def iterative_ridge_bfgs(weight, x, z0, alpha=1.0, lr=1.0, xtol=1e-5, tikhonov=1e-4, eps=None, line_search=True,
                         maxiter=None, dtype=torch.float32, order_seed=None):
    assert z0.dim() == 2
    if maxiter is None:
        maxiter = z0.size(1) * 5
    if eps is None:
        eps = torch.finfo(dtype).eps
    m = Model(weight, x, alpha, dtype, order_seed)
    z = z0.detach().to(dtype)
    fval, g, resid = m.evaluate(z)
    info = dict(iterations=0, f0=float(fval), t=[], ls_iters=[], objective=[], delta_x=[], evaluations=[], curvature=[],
                invalid_rows=[], lu=[], warnings=[])
    t = torch.clamp(lr / g.norm(p=1), max=lr)
    hess = Hessians(z, g, m.seeded)
    for it in range(1, maxiter + 1):
        A, rhs, is_zero = masked_system(hess.B, z, g, alpha, tikhonov, eps)
        d = batch_solve(rhs, A, info)
        trials = 0
        if line_search:
            from scipy.optimize import minimize_scalar
            if m.seeded:
                q = m.mm(d, m.w.T).double()
                rr, rq, qq = float(resid.double().square().sum()), float((resid.double() * q).sum()), float(q.square().sum())

                def line(tt):
                    tf = float(torch.tensor(tt, dtype=dtype))
                    l1 = float(z.add(d, alpha=-tf).double().abs().sum())
                    ft = 0.5 * (rr - 2.0 * tf * rq + tf * tf * qq) + alpha * l1
                    info['evaluations'].append((it, float(tt), ft))
                    return ft
            else:
                def line(tt):
                    z_new = z.add(d, alpha=-tt)
                    ft = float(m.smooth(z_new)[0] + alpha * z_new.norm(p=1))
                    info['evaluations'].append((it, float(tt), ft))
                    return ft
            found = minimize_scalar(line, bounds=(0, 10), method='bounded')
            t, trials = found.x, found.nfev
        z_new = torch.where(is_zero, z, z.add(d, alpha=-t))
        delta = torch.norm(z_new - z, p=2)
        z = z_new
        fval, g, resid = m.evaluate(z)
        info['iterations'] = it
        info['t'].append(float(t))
        info['ls_iters'].append(int(trials))
        info['objective'].append(float(fval))
        info['delta_x'].append(float(delta))
        finite = bool(torch.isfinite(torch.as_tensor(fval)))
        if bool(delta <= xtol) or not finite:
            info['invalid_rows'].append(-1)
            break
        ys, valid = hess.update(z, g)
        info['curvature'].append((it, ys.tolist()))
        info['invalid_rows'].append(int((~valid).sum()))
        t = lr
    return z, info


def assert_robust(info):
    """no |y.s| of the run is within a factor 10 of 1e-10"""
    for it, row in info['curvature']:
        for ys in row:
            a = abs(ys)
            assert a >= 10 * CURV_MIN or a <= CURV_MIN / 10, "|y.s| = %r at iteration %d is within 10x of 1e-10" % (a, it)


def update_reference(B, z, g, z_prev, g_prev, alpha, tikhonov, eps, first, update=True):
    """One BFGS.update (the reference's formula) and the masked system of the new z, everything in double:
    -> (B_new, system, rhs, valid)"""
    B, z, g, z_prev, g_prev = (t.double() for t in (B, z, g, z_prev, g_prev))
    n = z.shape[0]
    valid = torch.ones(n, dtype=torch.bool)
    if update:
        s, y = (z - z_prev).unsqueeze(2), (g - g_prev).unsqueeze(2)
        ys = torch.bmm(y.transpose(1, 2), s)
        # the verdict is taken on the float32 value of y.s
        vmask = ys.float().abs().gt(CURV_MIN)
        rho = torch.where(vmask, ys.float().double().reciprocal(), torch.full_like(ys, 1000.))
        if first:
            B = B * (rho * torch.bmm(y.transpose(1, 2), y))
        Bs = torch.bmm(B, s)
        new = B + rho * y * y.transpose(1, 2) - torch.bmm(Bs, Bs.transpose(1, 2)) / torch.bmm(s.transpose(1, 2), Bs)
        B = torch.where(vmask, new, B)
        valid = vmask.reshape(-1)
    A, rhs, _ = masked_system(B, z, g, alpha, tikhonov, eps)
    return B, A, rhs, valid


def objective64(weight, x, z, alpha):
    """the objective of a code, in double"""
    r = torch.mm(z.double(), weight.double().T) - x.double()
    return 0.5 * float(r.square().sum()) + alpha * float(z.double().abs().sum())
