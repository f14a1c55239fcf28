"""Host model of convolutional GPSR-Basic as the HIP path runs it (csrc/conv_gpsr.hip): the arithmetic of
tests/gpsr_model.py with the operator as two callables,

    A  = lambda v: F.conv_transpose2d(v, W, stride=s, padding=p)
    AT = lambda v: F.conv2d(v, W, stride=s, padding=p)

which is how a user of the reference's gpsr_basic(y, A, tau, AT, ...) runs it on a convolutional dictionary.
gpsr_model.py's loop multiplies by the dictionary matrix in place, so it cannot take the callables; this file
restates the loop and shares that file's constants and summary.  Every "dot" is a sum over the whole batch.  It runs
in the dtype of its inputs (float32 like the kernels, float64 to measure how far rounding alone moves a result) and
on their device."""
import math
import warnings

import numpy as np
import torch
import torch.nn.functional as F

from gpsr_model import DEFAULTS, MAX_TRIALS, _summary


def _objective(y, rb, u, v, tau):
    r = y - rb
    return 0.5 * torch.sum(r * r) + tau * (u.sum() + v.sum())


def _main_loop(y, A, AT, Ay, z, u, v, tau, mu, beta, maxiter, miniter, tol, crit_id, n_iter, info, verbose):
    rb = A(z)
    f = _objective(y, rb, u, v, tau)
    nz = z != 0
    if verbose:
        print('Initial obj = %10.6e, nz = %d\n' % (f, nz.sum()))
    ok = True
    while True:
        t = AT(rb) - Ay
        gu, gv = t + tau, -t + tau
        u_old, v_old = u, v
        cu = torch.where((u <= 0) & (gu >= 0), torch.zeros_like(gu), gu)
        cv = torch.where((v <= 0) & (gv >= 0), torch.zeros_like(gv), gv)
        q = A(cu - cv)
        lam = (torch.sum(gu * cu) + torch.sum(gv * cv)) / (torch.sum(q * q) + 1e-7)
        trials = 0
        while True:
            trials += 1
            du = torch.relu(u - lam * gu) - u
            dv = torch.relu(v - lam * gv) - v
            u_new, v_new = u + du, v + dv
            dz = du - dv
            rb_new = A(z + dz)
            f_new = _objective(y, rb_new, u_new, v_new, tau)
            bound = f + mu * (torch.sum(gu * du) + torch.sum(gv * dv))
            info['decisions'].append((float(f_new), float(bound), float(f)))
            if f_new <= bound:
                break
            if not math.isfinite(float(f_new)) or trials > MAX_TRIALS:
                ok = False
                break
            lam = lam * beta
            if verbose > 1:
                print('    line-search reducing lambda to %6.2e' % lam)
        if not ok:
            warnings.warn('GPSR line search failed (objective not finite or lambda reduced %d times); '
                          'returning the last accepted iterate' % MAX_TRIALS)
            break
        rb = rb_new
        f_prev, f = f, f_new
        m = torch.min(u_new, v_new)
        u, v = u_new - m, v_new - m
        z = u - v
        nz_prev, nz = nz, z != 0
        n_nz = int(nz.sum())
        n_iter += 1
        if verbose:
            print('It = %4d, obj = %9.5e, lambda = %6.2e, nz = %d' % (n_iter, f, lam, n_nz))
        if crit_id == 0:
            crit = float((nz != nz_prev).sum()) if n_nz >= 1 else float('-inf')
            name = 'd_nz'
        elif crit_id == 1:
            crit = float((f - f_prev).abs() / f_prev)
            name = 'd_f'
        elif crit_id == 2:
            crit = float(dz.norm() / z.norm())
            name = '||d_x|| / ||x||'
        elif crit_id == 3:
            numer = torch.max(torch.min(gu, u_old).abs().max(), torch.min(gv, v_old).abs().max())
            denom = torch.max(u_old.abs().max(), v_old.abs().max()).clamp(min=1e-6)
            crit = float(numer / denom)
            name = 'LCP'
        else:
            crit = float(f)
            name = 'f'
        if verbose:
            print(4 * ' ' + name + ' = %e (target = %e)' % (crit, tol))
        info['objective'].append(float(f))
        info['accepted_lambda'].append(float(lam))
        info['trials'].append(trials)
        info['criterion'].append(crit)
        info['stops'].append((crit, float(tol), crit_id))
        if (n_iter > miniter and crit <= tol) or n_iter >= maxiter:
            break
    return z, u, v, rb, f, n_iter, ok


def _debias(y, A, AT, z, tau, tol, n_iter, miniter, maxiter, verbose):
    resid = A(z) - y
    n_nz = int((z != 0).sum())
    if n_nz > y.numel() or n_nz == 0:
        warnings.warn('Debiasing requested but not performed. ' +
                      ('x has no nonzeros.' if n_nz == 0 else 'There are too many nonzeros in x.'))
        return z, 0.5 * torch.sum(resid * resid) + tau * z.abs().sum(), resid, n_iter
    off = z == 0
    start = n_iter
    r = AT(resid).masked_fill(off, 0.)
    rtr = torch.sum(r * r)
    thresh = tol * rtr
    p = -r
    while True:
        wp = A(p)
        ap = AT(wp).masked_fill(off, 0.)
        a = rtr / torch.sum(p * ap)
        z = z + a * p
        resid = resid + a * wp
        r = r + a * ap
        rtr_new = torch.sum(r * r)
        p = -r + (rtr_new / rtr) * p
        rtr = rtr_new
        n_iter += 1
        f = 0.5 * torch.sum(resid * resid) + tau * z.abs().sum()
        if verbose:
            print(' Iter = %5d, resid = %13.8e, convergence = %8.3e' % (n_iter, torch.sum(resid * resid), rtr / thresh))
        it = n_iter - start
        if not (it <= miniter or (bool(rtr > thresh) and it <= maxiter)):
            break
    return z, f, resid, n_iter


def gpsr_operator(y, A, AT, tau, x0=None, stop_criterion=3, tol=1e-2, maxiter=1000, miniter=5, init=0,
                  continuation=False, debias=False, verbose=0, return_info=False, **kwargs):
    """The model's solve with the operator as two callables; the arguments of the reference's gpsr_basic.  With
    return_info the second result carries what tests/gpsr_model.py's does (iterations, per iteration of the main phase
    objective, accepted_lambda, trials, criterion; final_objective; 'decisions': (f_new, bound, f) of every
    line-search trial) and 'stops': (criterion, tol, criterion id) of every stop test."""
    verbose = int(verbose)
    if stop_criterion not in (0, 1, 2, 3, 4):
        raise ValueError('Unknown stopping criterion')
    for name in kwargs:
        if name not in DEFAULTS:
            raise TypeError("gpsr_basic() got an unexpected keyword argument '%s'" % name)
    opt = dict(DEFAULTS, **kwargs)
    Ay = AT(y)
    if x0 is not None:
        z = x0
    elif init == 0:
        z = torch.zeros_like(Ay)
    elif init == 1:
        z = torch.randn_like(Ay)
    elif init == 2:
        z = Ay
    else:
        raise ValueError('Unknown initialization option')
    info = dict(objective=[], accepted_lambda=[], trials=[], criterion=[], decisions=[], stops=[], iterations=0)
    max_tau = Ay.abs().max() if Ay.numel() else Ay.new_tensor(float('inf'))
    if Ay.numel() and tau >= max_tau:
        warnings.warn('tau is too small; solution is zero vector')
        z = torch.zeros_like(Ay)
        info['final_objective'] = float('nan')
        return (z, info) if return_info else z
    if Ay.numel() == 0:
        info['final_objective'] = 0.0
        return (torch.zeros_like(Ay), info) if return_info else torch.zeros_like(Ay)
    if continuation:
        steps = opt['cont_steps']
        first = opt['first_tau_factor']
        if first is None or first * tau >= max_tau:
            warnings.warn('parameter FirstTauFactor too large; changing')
            first = float(0.8 * max_tau / tau)
        factors = 10 ** np.linspace(np.log10(first), 0, steps)
    else:
        steps, factors = 1, [1]
    u0, v0 = torch.relu(z), torch.relu(-z)
    n_iter = 0
    f = rb = None
    for i in range(steps):
        tau_i = float(tau * factors[i])
        if verbose > 1:
            print('Setting tau = %8.4f\n' % tau_i)
        last = i + 1 == steps
        z, _, _, rb, f, n_iter, ok = _main_loop(
            y, A, AT, Ay, z, u0, v0, tau_i, opt['mu'], opt['lambda_backtrack'], maxiter, miniter,
            tol if last else 1e-3, stop_criterion if last else 3, n_iter, info, verbose)
        if not ok:
            break
    if verbose:
        _summary('main algorithm', y - rb, z, f, verbose)
    if debias:
        if verbose:
            print('\nStarting the debiasing phase...\n')
        z, f, resid, n_iter = _debias(y, A, AT, z, tau, opt['tol_debias'], n_iter, opt['miniter_debias'],
                                      opt['maxiter_debias'], verbose)
        if verbose:
            _summary('debiasing phase', resid, z, f, verbose)
    info['iterations'] = n_iter
    info['final_objective'] = float(f)
    return (z, info) if return_info else z


def closures(weight, stride=1, padding=0):
    """(A, AT) for the convolutional dictionary `weight` [K,C,kh,kw]"""
    return (lambda v: F.conv_transpose2d(v, weight, stride=stride, padding=padding),
            lambda v: F.conv2d(v, weight, stride=stride, padding=padding))


def gpsr_conv2d(x, weight, tau, z0=None, stride=1, padding=0, **kwargs):
    """The model's convolutional solve; same arguments as lasso_amd.conv2d.gpsr_conv2d."""
    A, AT = closures(weight, stride, padding)
    return gpsr_operator(x, A, AT, tau, x0=z0, **kwargs)
