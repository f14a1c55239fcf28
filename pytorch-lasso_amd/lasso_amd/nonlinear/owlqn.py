"""HIP-backed OWL-QN: the arguments, defaults, warnings and prints of ``lasso.nonlinear.owlqn`` (reference
lasso/nonlinear/owlqn.py:80-199) on the kernels of csrc/owlqn.hip, for the objectives ``rss(x, weight)`` and ``bernoulli(x, weight)``."""
import ctypes as C
import warnings
from typing import NamedTuple

import torch

from .. import _native as nat

_LINE_SEARCHES = {'brent': nat.OWN_BRENT, 'backtrack': nat.OWN_BACKTRACK, 'none': nat.OWN_NONE}
_LS_DEFAULTS = dict(tol=0.1, decay=0.95, maxiter=500)          # backtracking(), owlqn.py:68
_BRENT_MAXFUN = 500                                            # evaluations one bounded Brent search makes at most


class rss(NamedTuple):
    """The objective ``fun(z) = 0.5 * (z @ weight.T - x).pow(2).sum()`` over the whole batch: x [n,d], weight [d,k].
    A description, not a function: ``owlqn`` hands its tensors to the HIP kernels and nothing is computed in torch."""
    x: torch.Tensor
    weight: torch.Tensor


class bernoulli(NamedTuple):
    """The objective ``fun(z) = sum(softplus(u) - x * u)`` with ``u = z @ weight.T`` over the whole batch, which is
    ``F.binary_cross_entropy_with_logits(u, x, reduction='sum')``: x [n,d], weight [d,k].  ``x`` is any real target --
    hard 0/1 or soft in [0, 1]; as in torch it is not validated.  A description, not a function, like ``rss``."""
    x: torch.Tensor
    weight: torch.Tensor


_FAMILIES = {bernoulli: nat.GLM_BERNOULLI}                     # rss: lasso_owlqn_solve; these: lasso_owlqn_glm_solve


def owlqn(fun, x0, alpha=1., lr=1, max_iter=20, xtol=1e-5, history_size=100, line_search='brent', ls_options=None,
          verbose=0, return_info=False):
    """Orthant-wise limited-memory quasi-Newton for min_z fun(z) + alpha ||z||_1 with ``fun = rss(x, weight)`` or
    ``fun = bernoulli(x, weight)``: x0 [n,k] -> z [n,k] (a new tensor on the device of ``x0``; no input is modified).
    Any other ``fun`` raises NotImplementedError: only these two descriptions run on the HIP path.

        z = owlqn(rss(x, weight), z0, alpha=0.5)
        # reference: owlqn(lambda z: 0.5 * (z @ weight.T - x).pow(2).sum(), z0, alpha=0.5)
        z = owlqn(bernoulli(x, weight), z0, alpha=0.1)
        # reference: owlqn(lambda z: F.binary_cross_entropy_with_logits(z @ weight.T, x, reduction='sum'), z0, alpha=0.1)

    The arguments and defaults are the reference's (owlqn.py:81-82) plus ``return_info``.  One objective, one line
    search, one L-BFGS memory and one stop test ``||x_new - x||_2 <= xtol`` serve the whole batch.  ``line_search``:
    'brent' (bounded Brent on (0, 10)), 'backtrack' (``ls_options``: tol 0.1, decay 0.95, maxiter 500; any other key
    raises TypeError) or 'none'; anything else raises RuntimeError.  The first step size is
    ``clamp(lr / ||pg||_1, max=lr)``, later ones ``lr`` ('backtrack' and 'none').  A pair (s, y) is dropped when
    ``y.s <= 1e-10``; the oldest leaves once ``history_size`` are held; no update follows the iteration that stops.
    ``verbose`` prints the reference's lines (after the solve: the iterations run inside one native call), and 'line
    search did not converge.' is warned once per backtracking that ran out of trials.  A non-finite objective ends
    the solve with the last accepted iterate (a warning).  ``return_info`` also returns ``dict(iterations, t,
    ls_iters, objective, delta_x, evaluations, pairs, skipped, H_diag)``: per iteration the step, the line-search
    evaluations, the objective and ||dx||_2 of the new iterate, the pairs held after its update, whether that update
    was dropped and the memory's scaling; ``evaluations`` lists the ``(iteration, t, f)`` the search evaluated.

    Deviations from the reference, all on purpose:
      * The objective and every dot product (y.s, y.y, the dots of the recursion) are folded in double; the
        backtracking test keeps the reference's float32 operation order, and Brent sees the un-rounded double.
      * The direction comes from the vector-free form of the two-loop recursion: the dots of v and of a new pair
        against the held pairs, the recursion on the small arrays S^T Y, Y^T Y, S^T v, Y^T v in double, and
        d = project(gamma v + S c + Y e, v) accumulated in double and rounded once -- the same operator, another
        order of operations.
      * An unknown ``line_search`` raises its RuntimeError up front, not at the first iteration.
      * ``bernoulli``: the objective is the double fold of per-element float32 losses, and the link is evaluated in
        the stable form e = exp(-|u|), loss = max(u, 0) - x u + log1p(e), sigmoid(u) = (u >= 0 ? 1 : e) / (1 + e):
        no exp(+|u|), so logits beyond 88.7 give a finite loss and residual.
    Only min(history_size, max_iter - 1) pairs are ever reserved (at most 1535).

    float32 tensors only, all of one dtype (anything else raises NotImplementedError naming the dtype); no cap on k.
    Like the reference (``@torch.no_grad()``), inputs that require grad are accepted and the result carries no graph.
    CPU tensors are staged through the device.  No CPU fallback."""
    assert x0.dim() == 2
    verbose = int(verbose)
    if ls_options is None:
        ls_options = {}
    if line_search not in _LINE_SEARCHES:
        raise RuntimeError("line_search must be one of {'brent', 'backtrack', 'none'}.")
    if not isinstance(fun, (rss, bernoulli)):
        raise NotImplementedError("lasso_amd: only rss(x, weight) objectives run on the HIP path (got %s)"
                                  % type(fun).__name__)
    for name in ls_options:
        if name not in _LS_DEFAULTS:
            raise TypeError("backtracking() got an unexpected keyword argument '%s'" % name)
    ls = dict(_LS_DEFAULTS, **ls_options)
    x, weight = fun.x, fun.weight
    if not (torch.is_tensor(x) and torch.is_tensor(weight)) or x.dim() != 2 or weight.dim() != 2:
        raise RuntimeError("owlqn: %s(x, weight) expects 2-D tensors x [n,d] and weight [d,k]" % type(fun).__name__)
    d, k = weight.shape
    n = x.size(0)
    assert x.size(1) == d
    assert x0.shape == (n, k)
    for t in (weight, x, x0):
        if t.dtype != torch.float32:
            raise NotImplementedError("lasso_amd: owlqn is not implemented for %s tensors" % t.dtype)
    max_iter, history_size = int(max_iter), int(history_size)
    if max_iter < 0 or history_size < 1 or int(ls['maxiter']) < 1 or alpha < 0:
        raise ValueError("owlqn: max_iter >= 0, history_size >= 1, ls_options['maxiter'] >= 1 and alpha >= 0 are "
                         "required")
    pairs = max(0, min(history_size, max_iter - 1))
    if pairs > nat.OWLQN_MAX_PAIRS:
        raise NotImplementedError("lasso_amd: owlqn holds at most %d pairs (min(history_size, max_iter - 1) = %d)"
                                  % (nat.OWLQN_MAX_PAIRS, pairs))
    nat.require_gpu()
    out_device = x0.device
    dev = nat.pick_device(x0, x, weight)
    xg = x.detach().to(device=dev).contiguous()
    wg = weight.detach().to(device=dev).contiguous()
    z0g = x0.detach().to(device=dev).contiguous()
    z = torch.empty((n, k), dtype=torch.float32, device=dev)
    info = dict(iterations=0, t=[], ls_iters=[], objective=[], delta_x=[], evaluations=[], pairs=[], skipped=[],
                H_diag=[])
    if n > 0:
        mode = _LINE_SEARCHES[line_search]
        cap = max(max_iter, 1)
        per_iter = {nat.OWN_BRENT: _BRENT_MAXFUN, nat.OWN_BACKTRACK: int(ls['maxiter']), nat.OWN_NONE: 0}[mode]
        ecap = max(max_iter * per_iter, 1)
        t_arr, f_arr, dx_arr, h_arr = ((C.c_double * cap)() for _ in range(4))
        ls_arr, p_arr, s_arr = ((C.c_int32 * cap)() for _ in range(3))
        e_iter, e_t, e_f = (C.c_int32 * ecap)(), (C.c_double * ecap)(), (C.c_double * ecap)()
        trace = nat.OwlqnTrace(cap, ecap, t_arr, ls_arr, f_arr, dx_arr, p_arr, s_arr, h_arr, e_iter, e_t, e_f, 0)
        options = nat.OwlqnOptions(max_iter, mode, int(ls['maxiter']), min(history_size, 2 ** 31 - 1), float(lr),
                                   float(xtol), float(ls['tol']), float(ls['decay']), 0)
        res = nat.OwlqnResult()
        res.trace = C.pointer(trace)
        L = nat.lib()
        with torch.cuda.device(dev):
            ws = nat.workspace(dev, L.lasso_owlqn_workspace_bytes(n, d, k, nat.LASSO_F32, pairs), "owlqn")
            head = (nat.ptr(xg), xg.stride(0) if n > 1 else d, nat.ptr(wg), wg.stride(0) if d > 1 else k,
                    nat.ptr(z0g), k, nat.ptr(z), k, n, d, k, nat.LASSO_F32, float(alpha))
            tail = (C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
            if isinstance(fun, rss):
                status = L.lasso_owlqn_solve(*head, *tail)
            else:
                status = L.lasso_owlqn_glm_solve(*head, _FAMILIES[type(fun)], *tail)
        nat.check(status)
        its = min(res.n_iter, cap)
        evs = min(trace.eval_count, ecap)
        info = dict(iterations=res.n_iter, t=list(t_arr[:its]), ls_iters=list(ls_arr[:its]), objective=list(f_arr[:its]),
                    delta_x=list(dx_arr[:its]), evaluations=[(e_iter[i], e_t[i], e_f[i]) for i in range(evs)],
                    pairs=list(p_arr[:its]), skipped=[bool(v) for v in s_arr[:its]], H_diag=list(h_arr[:its]))
        for _ in range(res.ls_failures):
            warnings.warn('line search did not converge.')                    # owlqn.py:76
        if res.flags & nat.OWN_NONFINITE:
            warnings.warn('owlqn: the objective is not finite; returning the last accepted iterate')
        if verbose:
            print('initial f: %0.4f' % res.f0)                                   # :129
            if verbose > 1:
                for i in range(its):
                    print('iter %3d - ls_iters: %3d - f: %0.4f - dx: %0.3e' % (i + 1, ls_arr[i], f_arr[i], dx_arr[i]))
            print("         Current function value: %f" % res.f_final)           # :196-197
            print("         Iterations: %d" % res.n_iter)
    else:
        z = z0g.clone()
    z = z.to(device=out_device)
    return (z, info) if return_info else z
