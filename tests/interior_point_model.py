"""Host model of the interior-point solver (TEST INFRASTRUCTURE): a torch restatement, in this project's words, of what
lasso/linear/solvers/interior_point.py computes -- in the HIP path's formulation.  The reference carries the dictionary
twice, W_pn = [W, -W], and per row factors I + W_pn diag(d) W_pn^T from an [n, 2k, d] intermediate.  Here the two halves
share one dictionary:

  lambda W_pn = [t, -t]               t = lambda W, one product
  z W_pn^T    = (z+ - z-) W^T         one product on the difference of the halves
  M           = I + W diag(c) W^T     c = d+ + d-, a d x d system per row

Three sums of the reference run over the 2k halves: z W_pn^T, the rhs product and M (and, in the start, sign(z0_pn) W_pn^T).
Merging the halves first, as above, rounds them differently -- and after four Newton steps ANY difference of one rounding
in one of them has grown to 150 - 1200 float32 ulp of the codes (measured seam by seam when the fixture was made; the
reference's own float32 and float64 runs are that far apart too).  So the model sums those in one of two orders.

Knobs the reference does not have:

  dtype       the precision everything runs in (float32: the reference's arithmetic; float64: the yardstick)
  order_seed  None: the reference's order -- the sums over the halves run over the 2k entries of [W, -W] as the reference's
              do, everything else in index order and torch's summation order; in float32 this reproduces the reference's
              float32 run, which is what the fixture's certification holds it to.  An integer: the HIP path's order,
              "another correct implementation" -- the halves are merged first (sign(z0), z+ - z-, the difference of the
              rhs halves, c = d+ + d-), the contraction index of every product is permuted, and so are the unknowns of
              every row's system before it is factored

Returns (zf, success, info); info carries `iterations`, the per-iteration lists obj, prim_feas, dual_feas, gap, obj0
(the objective of the start), and `margin`: the smallest relative distance of the largest ratio mean from tol."""
import torch

INF = float("inf")


def newton_rows(w, c, b, gen=None):
    """y [n,d] with (I + W diag(c_i) W^T) y_i = b_i; w [d,k], c [n,k], b [n,d]"""
    n, d = b.shape
    if gen is not None:
        pk = torch.randperm(w.shape[1], generator=gen)
        pd = torch.randperm(d, generator=gen)
        w, c, b = w[pd][:, pk].contiguous(), c[:, pk].contiguous(), b[:, pd].contiguous()
    m = torch.matmul(w.unsqueeze(0) * c.unsqueeze(1), w.T)
    m.diagonal(dim1=1, dim2=2).add_(1)
    chol, _ = torch.linalg.cholesky_ex(m)
    y = torch.cholesky_solve(b.unsqueeze(2), chol).squeeze(2)
    if gen is not None:
        out = torch.empty_like(y)
        out[:, pd] = y
        y = out
    return y


def newton_rows_halves(w, dp, dn, b):
    """the same y with c = dp + dn, summed over the 2k halves in the reference's order"""
    wpn = torch.cat([w, -w], 1)
    m = torch.matmul(wpn, torch.cat([dp, dn], 1).unsqueeze(2) * wpn.T.unsqueeze(0))
    m.diagonal(dim1=1, dim2=2).add_(1)
    chol, _ = torch.linalg.cholesky_ex(m)
    return torch.cholesky_solve(b.unsqueeze(2), chol).squeeze(2)


def start(z0, w, alpha, mm, times_wt):
    """-> zp, zn, lmbda, sp, sn, ok"""
    zp, zn = torch.relu(z0) + 0.1, torch.relu(-z0) + 0.1
    y = times_wt(torch.relu(z0).sign(), torch.relu(-z0).sign())   # sign(z0+) - sign(z0-) = sign(z0)
    omega = 1.1 * mm(y, w).abs().max(1, keepdim=True)[0]
    lmbda = alpha * y / omega
    t = mm(lmbda, w)
    sp, sn = alpha - t, alpha + t
    ok = bool(torch.all(zp > 0) and torch.all(zn > 0) and torch.all(sp > 0) and torch.all(sn > 0)
              and torch.all((-alpha < t) & (t < alpha)))
    return zp, zn, lmbda, sp, sn, ok


def interior_point(x, weight, z0, alpha=1.0, maxiter=20, barrier_init=0.1, tol=1e-2, eps=1e-5, dtype=torch.float32,
                   order_seed=None):
    w, x, z0 = weight.detach().to(dtype), x.detach().to(dtype), z0.detach().to(dtype)
    gen = None if order_seed is None else torch.Generator().manual_seed(int(order_seed))

    def mm(a, b):
        if gen is None:
            return torch.mm(a, b)
        p = torch.randperm(a.shape[1], generator=gen)
        return torch.mm(a[:, p].contiguous(), b[p].contiguous())

    def times_wt(ap, an):
        """[ap, an] W_pn^T = (ap - an) W^T"""
        if gen is None:
            return torch.mm(torch.cat([ap, an], 1), torch.cat([w, -w], 1).T)
        return mm(ap - an, w.T)

    def ginv(v):
        return v.reciprocal().masked_fill(v.abs() < eps, 0)

    def ratio_min(v, dv):
        return (-v / dv).masked_fill(dv >= 0, INF).min(1, keepdim=True)[0]

    zp, zn, lmbda, sp, sn, ok = start(z0, w, alpha, mm, times_wt)
    assert ok
    mu = barrier_init * x.new_ones(x.shape[0], 1)

    def f():
        return float(alpha * (zp.double().sum() + zn.double().sum()) + 0.5 * lmbda.double().pow(2).sum())

    info = dict(iterations=0, obj0=f(), obj=[], prim_feas=[], dual_feas=[], gap=[], margin=INF)
    success = False
    for it in range(1, maxiter + 1):
        t = mm(lmbda, w)
        rap, ran = -t - sp + alpha, t - sn + alpha
        rb = x - times_wt(zp, zn) - lmbda
        rcp, rcn = mu - zp * sp, mu - zn * sn
        sip, sin_ = ginv(sp), ginv(sn)
        dp, dn = sip * zp, sin_ * zn
        rhs = rb - times_wt(sip * rcp - dp * rap, sin_ * rcn - dn * ran)
        d_lmbda = newton_rows_halves(w, dp, dn, rhs) if gen is None else newton_rows(w, dp + dn, rhs, gen)
        u = mm(d_lmbda, w)
        dsp, dsn = rap - u, ran + u
        dzp, dzn = sip * (rcp - zp * dsp), sin_ * (rcn - zn * dsn)
        beta_z = torch.minimum(ratio_min(zp, dzp), ratio_min(zn, dzn)).clamp(None, 1)
        beta_sl = torch.minimum(ratio_min(sp, dsp), ratio_min(sn, dsn)).clamp(None, 1)
        zp, zn = zp + 0.99 * beta_z * dzp, zn + 0.99 * beta_z * dzn
        lmbda = lmbda + 0.99 * beta_sl * d_lmbda
        sp, sn = sp + 0.99 * beta_sl * dsp, sn + 0.99 * beta_sl * dsn
        mu = mu * (1 - torch.min(beta_z, beta_sl).clamp(None, 0.99))
        zp, zn, sp, sn = zp.clamp(min=0), zn.clamp(min=0), sp.clamp(min=0), sn.clamp(min=0)
        z_norm = (zp.pow(2).sum(1) + zn.pow(2).sum(1)).sqrt()
        l_norm = lmbda.norm(dim=1)
        ra_norm = (rap.pow(2).sum(1) + ran.pow(2).sum(1)).sqrt()
        prim = float(torch.mean(rb.norm(dim=1) / (1 + z_norm)))
        dual = float(torch.mean(ra_norm / (1 + l_norm)))
        gap = float(torch.mean(((zp * sp).sum(1) + (zn * sn).sum(1)) / (1 + z_norm * l_norm)))
        info["iterations"] = it
        info["obj"].append(f())
        info["prim_feas"].append(prim)
        info["dual_feas"].append(dual)
        info["gap"].append(gap)
        if tol > 0:
            worst = max(prim, dual, gap)
            info["margin"] = min(info["margin"], abs(worst - tol) / tol if worst == worst else INF)
        if prim < tol and dual < tol and gap < tol:
            success = True
            break
    return zp - zn, success, info
