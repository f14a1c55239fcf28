"""HIP-backed GPSR-Basic: the arguments, defaults, warnings and prints of
``lasso.linear.solvers.gpsr.gpsr_basic`` (reference gpsr.py:209-365) on the kernels of csrc/gpsr.hip."""
import ctypes as C
import warnings

import torch

from ... import _native as nat

_KW_DEFAULTS = dict(mu=0.1, lambda_backtrack=0.5, cont_steps=5, first_tau_factor=None,
                    tol_debias=1e-4, maxiter_debias=500, miniter_debias=0)
_CRITERION_NAMES = ('d_nz', 'd_f', '||d_x|| / ||x||', 'LCP', 'f')


def _f32(n):
    return (C.c_float * max(n, 1))()


def _i32(n):
    return (C.c_int32 * max(n, 1))()


def _summary(phase, rr, l1, f, nz, verbose):
    if verbose == 1:
        print('\nFinal obj = %10.6e, nz = %d' % (f, nz))
    elif verbose > 1:
        print('\nFinished the %s.\nResults:' % phase)
        print('    ||A x - y ||_2^2 = %10.3e' % rr)
        print('    ||x||_1 = %10.3e' % l1)
        print('     Obj. function: %10.3e' % f)
        print('     Num. non-zero components: %d' % nz)


def _request(stop_criterion, tol, maxiter, miniter, init, continuation, debias, opt, has_z0):
    """The options, result and trace structs of one solve (lasso_gpsr_solve and lasso_conv_gpsr_solve take the same):
    -> (options, res, keep) where ``keep`` holds the host arrays the trace points to, for _report."""
    steps = int(opt['cont_steps']) if continuation else 1
    cap = int(maxiter) + steps + 1
    dcap = (max(int(opt['maxiter_debias']), int(opt['miniter_debias'])) + 2) if debias else 0
    lam, lam0, obj, crit = _f32(cap), _f32(cap), _f32(cap), _f32(cap)
    trials, nz = _i32(cap), _i32(cap)
    s_tau, s_f0, s_nz0, s_end = (C.c_double * steps)(), _f32(steps), _i32(steps), _i32(steps)
    db_rr, db_conv = _f32(dcap), _f32(dcap)
    trace = nat.GpsrTrace(cap, lam, lam0, trials, obj, crit, nz, steps, s_tau, s_f0, s_nz0, s_end,
                          dcap, db_rr, db_conv)
    first = opt['first_tau_factor']
    options = nat.GpsrOptions(
        int(stop_criterion), int(maxiter), int(miniter), int(init) if not has_z0 else 0,
        int(bool(continuation)), int(bool(debias)), steps, int(opt['maxiter_debias']),
        int(opt['miniter_debias']), 0, float(tol), float(opt['mu']), float(opt['lambda_backtrack']),
        float(first) if first is not None else -1.0, float(opt['tol_debias']))
    res = nat.GpsrResult()
    res.trace = C.pointer(trace)
    return options, res, (steps, cap, dcap, lam, lam0, obj, crit, trials, nz, s_tau, s_f0, s_nz0, s_end, db_rr, db_conv,
                          trace)


def _report(res, keep, stop_criterion, tol, debias, opt, verbose):
    """The reference's warnings and prints for a finished solve (after it: the iterations ran inside one native
    call) -> the ``return_info`` dictionary."""
    steps, cap, dcap, lam, lam0, obj, crit, trials, nz, s_tau, s_f0, s_nz0, s_end, db_rr, db_conv, _ = keep
    flags = res.flags
    if flags & nat.GPSR_ZERO_SOLUTION:
        warnings.warn('tau is too small; solution is zero vector')       # :278
    if flags & nat.GPSR_TAU_FACTOR_CHANGED:
        warnings.warn('parameter FirstTauFactor too large; changing')    # :290
    its = min(res.n_iter - res.db_iters, cap)
    info = dict(iterations=res.n_iter, objective=list(obj[:its]), accepted_lambda=list(lam[:its]),
                trials=list(trials[:its]), criterion=list(crit[:its]), final_objective=res.objective)
    if verbose and not flags & nat.GPSR_ZERO_SOLUTION:
        beta32 = torch.tensor(float(opt['lambda_backtrack']), dtype=torch.float32)
        it = 0
        for s in range(res.steps):
            if verbose > 1:
                print('Setting tau = %8.4f\n' % s_tau[s])
            print('Initial obj = %10.6e, nz = %d\n' % (s_f0[s], s_nz0[s]))
            last = s + 1 == steps
            name = _CRITERION_NAMES[stop_criterion if last else 3]
            while it < min(s_end[s], cap):
                if verbose > 1:
                    lam_t = torch.tensor(lam0[it], dtype=torch.float32)
                    for _ in range(trials[it] - 1):
                        lam_t = lam_t * beta32
                        print('    line-search reducing lambda to %6.2e' % lam_t)
                print('It = %4d, obj = %9.5e, lambda = %6.2e, nz = %d' % (it + 1, obj[it], lam[it], nz[it]))
                print(4 * ' ' + name + ' = %e (target = %e)' % (crit[it], tol if last else 1e-3))
                it += 1
        _summary('main algorithm', res.main_rr, res.main_l1, res.main_objective, res.main_nz, verbose)
    if flags & nat.GPSR_LINESEARCH_FAILED:
        warnings.warn('GPSR line search failed (objective not finite or lambda reduced 100 times); '
                      'returning the last accepted iterate')
    if debias and not flags & (nat.GPSR_ZERO_SOLUTION | nat.GPSR_LINESEARCH_FAILED):
        if verbose:
            print('\nStarting the debiasing phase...\n')
        if flags & nat.GPSR_DEBIAS_NO_NONZEROS:
            warnings.warn('Debiasing requested but not performed. x has no nonzeros.')            # :143-148
        elif flags & nat.GPSR_DEBIAS_TOO_MANY:
            warnings.warn('Debiasing requested but not performed. There are too many nonzeros in x.')
        if verbose:
            if res.db_iters:
                for i in range(min(res.db_iters, dcap)):
                    print(' Iter = %5d, resid = %13.8e, convergence = %8.3e' %
                          (res.n_iter - res.db_iters + i + 1, db_rr[i], db_conv[i]))
                _summary('debiasing phase', res.db_rr, res.db_l1, res.objective, res.db_nz, verbose)
            else:
                _summary('debiasing phase', res.main_rr, res.main_l1, res.objective, res.main_nz, verbose)
    return info


def gpsr_basic(x, weight, tau, x0=None, stop_criterion=3, tol=1e-2, maxiter=1000, miniter=5, init=0,
               continuation=False, debias=False, verbose=0, return_info=False, **kwargs):
    """GPSR-Basic (Figueiredo, Nowak, Wright 2007): min_z 0.5 ||x - z W^T||^2 + tau ||z||_1 for the whole batch
    by gradient projection on the split z = u - v, u, v >= 0.  x [n,d], weight [d,k] -> z [n,k] (a new tensor;
    no input is modified).

    The arguments are the reference's (gpsr.py:209-211) except that the dictionary ``weight`` takes the place of
    its ``A`` / ``AT`` callables -- a Python callable cannot run inside a HIP kernel; ``A(v) = v W^T`` and
    ``AT(v) = v W`` are what sparse_encode.py:56-59 passes.  ``**kwargs``: mu (0.1), lambda_backtrack (0.5),
    cont_steps (5), first_tau_factor (None), tol_debias (1e-4), maxiter_debias (500), miniter_debias (0); any
    other keyword raises TypeError.  An unknown ``stop_criterion`` or ``init`` raises ValueError.

    Every inner product is a sum over the whole batch, as in the reference, so the rows of a batch share one step
    size, one line search and one stop decision per iteration.  ``verbose`` prints the reference's lines (after
    the solve: the iterations run inside one native call).  One extension: the reference's line search has no
    cap and never ends once the objective is NaN; here a search whose objective is not finite, or that has
    reduced lambda 100 times, ends the solve with a warning and returns the last accepted z.

    bfloat16 / float16 tensors are computed in float32 on their exact up-conversions and rounded once at the
    end; float64 tensors, and tensors that require grad under grad mode (the reference's loop would build an
    autograd graph), raise NotImplementedError.  CPU tensors are staged through the device and the result comes
    back on the device of ``x``.  ``return_info`` (extension) also returns
    ``dict(iterations, objective, accepted_lambda, trials, criterion, final_objective)``: the iteration count
    (debias steps included, like the reference's counter), per iteration of the main phase the objective, the
    accepted step, the number of line-search trials and the stop criterion, and the objective at the end.
    No CPU fallback."""
    verbose = int(verbose)
    if stop_criterion not in (0, 1, 2, 3, 4):
        raise ValueError('Unknown stopping criterion')                       # gpsr.py:240-241
    if x0 is None and init not in (0, 1, 2):
        raise ValueError('Unknown initialization option')                    # :272
    for name in kwargs:
        if name not in _KW_DEFAULTS:
            raise TypeError("gpsr_basic() got an unexpected keyword argument '%s'" % name)
    opt = dict(_KW_DEFAULTS, **kwargs)
    if x.dim() != 2 or weight.dim() != 2:
        raise RuntimeError("gpsr_basic expects 2-D x and weight")
    d, k = weight.shape
    n = x.size(0)
    assert x.size(1) == d
    if x0 is not None:
        assert x0.shape == (n, k)
    tensors = [t for t in (x, weight, x0) if t is not None]
    for t in tensors:
        if t.dtype == torch.float64:
            raise NotImplementedError("lasso_amd: gpsr_basic is not implemented for torch.float64 tensors")
        if t.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise NotImplementedError("lasso_amd: gpsr_basic is not implemented for %s tensors" % t.dtype)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise NotImplementedError("lasso_amd: gpsr_basic does not build an autograd graph; inputs that "
                                  "require grad (requires_grad=True) are not supported -- detach them")
    nat.require_gpu()
    out_device, out_dtype = x.device, x.dtype
    dev = nat.pick_device(x, weight, x0)
    xg = x.detach().to(device=dev, dtype=torch.float32).contiguous()
    wg = weight.detach().to(device=dev, dtype=torch.float32).contiguous()
    if x0 is None and init == 1:
        x0 = torch.randn(n, k, dtype=torch.float32, device=dev)              # :268 randn_like(Ay)
    z0g = x0.detach().to(device=dev, dtype=torch.float32).contiguous() if x0 is not None else None
    z = torch.empty((n, k), dtype=torch.float32, device=dev)
    info = dict(iterations=0, objective=[], accepted_lambda=[], trials=[], criterion=[], final_objective=float('nan'))
    if n > 0:
        options, res, keep = _request(stop_criterion, tol, maxiter, miniter, init, continuation, debias, opt,
                                      x0 is not None)
        L = nat.lib()
        with torch.cuda.device(dev):
            ws = nat.workspace(dev, L.lasso_gpsr_workspace_bytes(n, d, k, nat.LASSO_F32), "gpsr")
            nat.check(L.lasso_gpsr_solve(
                nat.ptr(xg), xg.stride(0) if n > 1 else d, nat.ptr(wg), wg.stride(0) if d > 1 else k,
                nat.ptr(z0g), k, nat.ptr(z), k, n, d, k, nat.LASSO_F32, float(tau),
                C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)))
        info = _report(res, keep, stop_criterion, tol, debias, opt, verbose)
    z = z.to(device=out_device, dtype=out_dtype)
    return (z, info) if return_info else z
