"""Host model of the iterated-ridge solver (TEST INFRASTRUCTURE): a torch restatement, in this project's words, of what
lasso/linear/solvers/iterative_ridge.py computes with cg=False -- but COMPACTED: each row solves
(G[S,S] + diag(alpha / |z_S| + tikhonov)) z_S = (x W)_S on its own support S = {j : |z_j| >= eps}, where the reference
factors the masked k x k matrix (zero rows and columns off the support, tikhonov on their diagonal, zero right-hand
side: the same solution on S, 0 elsewhere).  Knobs the reference does not have:

  dtype       the precision everything runs in (float32: the reference's arithmetic; float64: the yardstick)
  order_seed  None: supports in index order, torch's summation order.  An integer: "another correct implementation" --
              every support is permuted before it is factored, the contraction index of every product is permuted, and
              the line-search objective comes from the three sums |r|^2, <r,q>, |q|^2 folded in double (as the HIP path
              does) instead of from a product of ``dtype`` per trial

The Brent arm needs scipy, imported when it is used.  Returns (z, info); info carries per iteration fval, sum |update|, t,
the support counts of the new z, and `margin`: the smallest relative distance of a stop decision from the scaled tol."""
import torch


def solve_rows(g, rhs, z, alpha, tikhonov, eps, gen=None):
    """z_sol [n,k] of one iteration; masked entries are exact zeros.  Also the first (row, minor) whose factorisation
    failed, or None."""
    n, k = z.shape
    z_sol = torch.zeros_like(z)
    bad = None
    for i in range(n):
        s = torch.nonzero(~(z[i].abs() < eps)).flatten()
        if s.numel() == 0:
            continue
        if gen is not None:
            s = s[torch.randperm(s.numel(), generator=gen)]
        a = g[s][:, s].clone()
        a.diagonal().add_(alpha / z[i, s].abs() + tikhonov)
        chol, info = torch.linalg.cholesky_ex(a)
        if int(info) != 0 and bad is None:
            bad = (i, int(info))
        z_sol[i, s] = torch.cholesky_solve(rhs[i, s].unsqueeze(1), chol).squeeze(1)
    return z_sol, bad


def iterative_ridge(z0, x, weight, alpha=1.0, tol=1e-5, tikhonov=1e-4, eps=None, maxiter=10, line_search=True,
                    dtype=torch.float32, order_seed=None):
    w, x, z = weight.detach().to(dtype), x.detach().to(dtype), z0.detach().to(dtype).clone()
    gen = None if order_seed is None else torch.Generator().manual_seed(int(order_seed))
    if eps is None:
        eps = torch.finfo(torch.float32 if dtype == torch.float32 else dtype).eps
    budget = z.numel() * tol

    def mm(a, b):
        if gen is None:
            return torch.mm(a, b)
        p = torch.randperm(a.shape[1], generator=gen)
        return torch.mm(a[:, p].contiguous(), b[p].contiguous())

    def f(zz):
        return 0.5 * (mm(zz, w.T) - x).pow(2).sum() + alpha * zz.abs().sum()

    info = dict(iterations=0, status="maxiter", f0=float(f(z)), fval=[], update=[], t=[], support_max=[], support_mean=[],
                margin=float("inf"), bad=None)
    rhs, g = mm(x, w), mm(w.T, w)
    for it in range(1, maxiter + 1):
        mask = z.abs() < eps
        z_sol, bad = solve_rows(g, rhs, z, alpha, tikhonov, eps, gen)
        if bad is not None and info["bad"] is None:
            info["bad"] = bad
        if line_search:
            from scipy.optimize import minimize_scalar
            p = z_sol - z
            if gen is None:
                line = lambda t: float(f(z.add(p, alpha=t)))                                    # noqa: E731
            else:
                r, q = (mm(z, w.T) - x).double(), mm(p, w.T).double()
                rr, rq, qq = float((r * r).sum()), float((r * q).sum()), float((q * q).sum())
                line = lambda t: 0.5 * (rr + 2 * t * rq + t * t * qq) + \
                    alpha * float(z.add(p, alpha=float(torch.tensor(t, dtype=dtype))).abs().double().sum())  # noqa: E731
            res = minimize_scalar(line, bounds=(0, 10), method="bounded")
            t, fval = float(res.x), float(res.fun)
            update = p.mul(t)
            z = torch.where(mask, z, z + update)
        else:
            t = 1.0
            update = z_sol - z
            z = torch.where(mask, z, z_sol)
            fval = float(f(z))
        total = float(update.abs().sum())
        counts = (~(z.abs() < eps)).sum(1)
        info["iterations"] = it
        info["fval"].append(fval)
        info["update"].append(total)
        info["t"].append(t)
        info["support_max"].append(int(counts.max()))
        info["support_mean"].append(float(counts.double().mean()))
        if budget > 0:
            info["margin"] = min(info["margin"], abs(total - budget) / budget)
        if total <= budget:
            info["status"] = "converged"
            break
        if fval != fval or bool(update.isnan().any()):
            info["status"] = "nan"
            break
    return z, info
