"""Host model of ``coord_descent_mod`` (reference lasso/linear/solvers/coordinate_descent.py:57-139) in plain torch,
for any floating dtype, with the code shaped ``[n_samples, n_components]`` (the reference allocates
``[n_features, n_components]``, :73, and so only runs when n == d; there the two are the same computation, and
tests/golden/generate_golden_cd_mod.py requires ``torch.equal`` with the real reference on such cases).

Beyond the reference's ``(z, gap)`` it reports, per row, the sweeps run, whether the row converged, how close any of
its evaluated gaps came to the threshold (min |gap / tol_row - 1|) and, in total, the coordinate updates that changed
a value.

`rule_margin` guards the OTHER stop decision, the check rule of :132 (max|change| / max|z| < tol): the smallest relative
distance of that ratio from tol at a sweep where the other outcome would have changed the row's sweep count -- the
sweep it stopped at (fired just below tol: the other outcome sweeps on), or a sweep that just missed the rule while the
gap was already below (1.05 x) the threshold (the other outcome stops there).  inf where no such sweep exists."""
import math

import torch
import torch.nn.functional as F


def duality_gap(z, x, W, alpha):
    """:87-99 for every row of z, in z's dtype."""
    R = x - torch.matmul(z, W.T)
    XtA = torch.mm(R, W)
    dual = XtA.abs().max(1)[0]
    rn2 = R.pow(2).sum(1)
    small = dual <= alpha
    const = (alpha / dual).masked_fill(small, 1.)
    gap = torch.where(small, rn2, 0.5 * rn2 * (1 + const.pow(2)))
    return gap + alpha * z.abs().sum(1) - const * (R * x).sum(1)


def coord_descent_mod(x, W, z0=None, alpha=1.0, max_iter=1000, tol=1e-4):
    """-> z, gap, info;  info = dict(sweeps [n] int32, converged [n] bool, closest [n] float64, rule_margin [n] float64,
    committed int)."""
    d, k = W.shape
    n = x.shape[0]
    assert x.shape[1] == d
    if z0 is None:
        z = x.new_zeros(n, k)
    else:
        assert z0.shape == (n, k)
        z = z0
    gap = z.new_full((n,), tol + 1.)                                  # :78
    converged = torch.zeros(n, dtype=torch.bool)
    sweeps = torch.zeros(n, dtype=torch.int32)
    closest = torch.full((n,), math.inf, dtype=torch.float64)
    rule_margin = torch.full((n,), math.inf, dtype=torch.float64)
    committed = 0
    rel_tol = tol
    tol_row = tol * x.pow(2).sum(1)                                   # :81
    norms = W.pow(2).sum(0)                                           # :84

    def check(z_, x_, R_, tol_):                                      # :87-99 on the residual carried along
        XtA = torch.mm(R_, W)
        dual = XtA.abs().max(1)[0]
        rn2 = R_.pow(2).sum(1)
        small = dual <= alpha
        const = (alpha / dual).masked_fill(small, 1.)
        g = torch.where(small, rn2, 0.5 * rn2 * (1 + const.pow(2)))
        g = g + alpha * z_.abs().sum(1) - const * (R_ * x_).sum(1)
        return g < tol_, g

    R = x - torch.matmul(z, W.T)                                      # :102
    for it in range(max_iter):
        if converged.all():
            break
        act, = torch.where(~converged)
        sweeps[act] += 1
        z_max = z.new_zeros(len(act))
        d_max = z.new_zeros(len(act))
        for i in range(k):                                            # :110-129
            if norms[i] == 0:
                continue
            atom = W[:, i].contiguous()
            old = z[act, i].clone()
            nz = old != 0
            R[act[nz]] += torch.outer(old[nz], atom)
            z[act, i] = F.softshrink(R[act].matmul(atom), alpha)
            z[act, i] /= norms[i]
            new = z[act, i]
            nz = new != 0
            R[act[nz]] -= torch.outer(new[nz], atom)
            committed += int((new != old).sum())
            d_max = torch.maximum(d_max, (new - old).abs())
            z_max = torch.maximum(z_max, new.abs())
        chk = (z_max == 0) | (d_max / z_max < rel_tol) | (it == max_iter - 1)      # :132
        ratio = d_max.double() / z_max.double() / rel_tol if rel_tol > 0 else torch.full((len(act),), math.inf).double()
        by_ratio = (z_max != 0) & (it != max_iter - 1)            # rows whose check hangs on the ratio alone
        miss = by_ratio & ~chk & (ratio < 1.05)                    # just missed the rule: would the gap have passed?
        if miss.any():
            jx = act[miss]
            _, g_miss = check(z[jx], x[jx], R[jx], tol_row[jx])
            hit = g_miss.double() < 1.05 * tol_row[jx].double()
            rule_margin[jx[hit]] = torch.minimum(rule_margin[jx[hit]], ratio[miss][hit] - 1)
        if not chk.any():
            continue
        ix = act[chk]
        converged[ix], gap[ix] = check(z[ix], x[ix], R[ix], tol_row[ix])
        fired = by_ratio[chk] & converged[ix]                      # stopped on a ratio just below tol
        rule_margin[ix[fired]] = torch.minimum(rule_margin[ix[fired]], 1 - ratio[chk][fired])
        ratio = (gap[ix].double() / tol_row[ix].double() - 1).abs()
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        closest[ix] = torch.minimum(closest[ix], ratio)
    return z, gap, dict(sweeps=sweeps, converged=converged, closest=closest, rule_margin=rule_margin,
                        committed=committed)
