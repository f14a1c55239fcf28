"""HIP-backed ``ista_nl``: the arguments, defaults, error and prints of ``lasso.nonlinear.ista_nl`` (reference
lasso/nonlinear/ista.py:55-128) on the kernels of csrc/ista_nl.hip, for decoders of one affine layer and a pointwise
activation, ``decoder(z) = act(z @ weight.T + bias)``."""
import ctypes as C
from typing import NamedTuple, Optional

import torch

from .. import _native as nat

_ACTIVATIONS = {'identity': nat.ACT_IDENTITY, 'sigmoid': nat.ACT_SIGMOID, 'tanh': nat.ACT_TANH, 'relu': nat.ACT_RELU}
_MODULES = {torch.nn.Identity: 'identity', torch.nn.Sigmoid: 'sigmoid', torch.nn.Tanh: 'tanh', torch.nn.ReLU: 'relu'}


class affine(NamedTuple):
    """The decoder ``decoder(z) = act(z @ weight.T + bias)``: weight [d,k] (``torch.nn.Linear``'s own layout), bias [d]
    or None, activation 'identity', 'sigmoid', 'tanh' or 'relu'.  A description, not a function: ``ista_nl`` hands its
    tensors to the HIP kernels and nothing is computed in torch."""
    weight: torch.Tensor
    bias: Optional[torch.Tensor] = None
    activation: str = 'identity'


def _describe(decoder):
    """-> affine(weight, bias, activation) of a decoder the HIP path runs; NotImplementedError naming the type otherwise.
    A module's tensors are read and nothing of it -- its training flag, its parameters' requires_grad -- is changed."""
    if isinstance(decoder, affine):
        if decoder.activation not in _ACTIVATIONS:
            raise NotImplementedError("lasso_amd: ista_nl has no activation %r (one of %s)"
                                      % (decoder.activation, ", ".join(sorted(_ACTIVATIONS))))
        return decoder
    if type(decoder) is torch.nn.Linear:
        return affine(decoder.weight, decoder.bias, 'identity')
    if type(decoder) is torch.nn.Sequential:
        layers = list(decoder)
        if len(layers) != 2 or type(layers[0]) is not torch.nn.Linear:
            raise NotImplementedError("lasso_amd: ista_nl runs Sequential(Linear, activation) only, not Sequential(%s)"
                                      % ", ".join(type(m).__name__ for m in layers))
        if type(layers[1]) not in _MODULES:
            raise NotImplementedError("lasso_amd: ista_nl has no activation %s (one of Identity, Sigmoid, Tanh, ReLU)"
                                      % type(layers[1]).__name__)
        return affine(layers[0].weight, layers[0].bias, _MODULES[type(layers[1])])
    raise NotImplementedError("lasso_amd: ista_nl runs nn.Linear, nn.Sequential(nn.Linear, activation) and "
                              "affine(weight, bias, activation) decoders on the HIP path, not %s" % type(decoder).__name__)


def ista_nl(x, z0, decoder, alpha=1.0, fast=True, maxiter=10, lr='auto', power_iters=10, tol=1e-5, eval_mode=True,
            verbose=0, power_init=None, return_info=False):
    """ISTA / FISTA for min_z 0.5 ||decoder(z) - x||^2 + alpha ||z||_1 with ``decoder(z) = act(z @ weight.T + bias)``:
    x [n,d], z0 [n,k] -> z [n,k] (a new tensor on the device of ``z0``; no input is modified).

        z = ista_nl(x, z0, torch.nn.Sequential(torch.nn.Linear(k, d), torch.nn.Sigmoid()), alpha=0.1)
        z = ista_nl(x, z0, affine(weight, bias, 'tanh'), alpha=0.1, lr=0.05)

    The arguments and defaults are the reference's (ista.py:55-56) plus ``power_init`` and ``return_info``.  ``decoder``:
    ``nn.Linear(k, d)`` (with or without bias), ``nn.Sequential(nn.Linear(k, d), A)`` with A one of ``nn.Identity``,
    ``nn.Sigmoid``, ``nn.Tanh``, ``nn.ReLU``, or the description ``affine(weight, bias=None, activation='identity')``;
    anything else -- deeper stacks, other activations, other modules -- raises NotImplementedError naming the type.  For
    this family the gradient and the Hessian-vector products the reference takes from autograd have a closed form, a
    pair of GEMMs with fused epilogues.  ``eval_mode`` is accepted and has nothing to do for these decoders.

    ``lr``: a Python float or 'auto' (anything else, an int included, raises the reference's ValueError).  'auto'
    takes, at every step, the per-row step 0.98 / L_i with L_i from the reference's power iteration (``power_iters``
    rounds, 2 power_iters + 1 Hessian products) on the row's Hessian of the rss term at the step's point.
    ``power_init`` [n,k] is its start vector; None draws ``torch.randn(n, k)`` on the device once per solve.  A row
    whose Hessian is zero (a dead ReLU row) gets the reference's inf / NaN; nothing is checked or repaired.
    The stop rule is the reference's: ``sum|z - z_next| <= z0.numel() * tol`` over the whole batch ends the solve with
    that iteration's z_next; ``tol <= 0`` runs ``maxiter`` iterations (no host read at all without ``verbose`` /
    ``return_info``).  ``verbose`` prints the reference's lines after the solve (the iterations run inside one native
    call); the per-iteration loss of ``verbose > 1`` costs one more decoder product per iteration and is computed only
    then.  ``return_info`` also returns ``dict(iterations, deltas, stopped, L)``: the per-iteration sums
    ``sum|z - z_next|``, whether the rule fired, and under 'auto' the [n] estimates L of the last step (else None).

    Deviations from the reference, all on purpose:
      * 'auto' uses the SAME start vector at every step where the reference draws ``torch.randn_like`` at every step:
        one independent estimate per step all the same, deterministic given ``power_init``, and comparable with the
        reference (patched to return ``power_init``).
      * The normalisation of the power iteration is applied as a per-row scale after the next product instead of to
        the vector before it (the product is linear), and sigmoid / tanh are evaluated from exp(-|u|) / exp(-2|u|).
      * ``sum|z - z_next|`` and the losses are folded in double in a fixed order: two solves give the same bits.

    float32 tensors only (anything else raises NotImplementedError naming the dtype); any n, d, k.  Inputs that require
    grad are accepted and the result carries no graph.  CPU tensors are staged through the device.  No CPU fallback."""
    if not (lr == 'auto' or isinstance(lr, float)):
        raise ValueError('expected `lr` to be either float or "auto".')
    dec = _describe(decoder)
    weight, bias = dec.weight, dec.bias
    verbose = max(0, min(int(verbose), 2))
    maxiter, power_iters = int(maxiter), int(power_iters)
    lr_auto = lr == 'auto'
    if not (torch.is_tensor(x) and torch.is_tensor(z0) and torch.is_tensor(weight)) or x.dim() != 2 or z0.dim() != 2 \
            or weight.dim() != 2:
        raise RuntimeError("ista_nl: expected 2-D tensors x [n,d], z0 [n,k] and a decoder weight [d,k]")
    d, k = weight.shape
    n = x.size(0)
    assert x.size(1) == d
    assert z0.shape == (n, k)
    assert bias is None or bias.shape == (d,)
    assert power_init is None or power_init.shape == (n, k)
    for t in (x, z0, weight, bias, power_init):
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError("lasso_amd: ista_nl is not implemented for %s tensors" % t.dtype)
    if maxiter < 0 or (lr_auto and power_iters < 1):
        raise ValueError("ista_nl: maxiter >= 0 and, with lr='auto', power_iters >= 1 are required")
    nat.require_gpu()
    out_device = z0.device
    dev = nat.pick_device(z0, x, weight)
    xg = x.detach().to(device=dev).contiguous()
    wg = weight.detach().to(device=dev).contiguous()
    bg = bias.detach().to(device=dev).contiguous() if bias is not None else None
    z0g = z0.detach().to(device=dev).contiguous()
    ug = None
    if lr_auto:
        ug = torch.randn(n, k, device=dev) if power_init is None else power_init.detach().to(device=dev).contiguous()
    info = dict(iterations=0, deltas=[], stopped=False, L=None)
    if n == 0:
        z = z0g.clone().to(device=out_device)
        return (z, info) if return_info else z
    z = torch.empty((n, k), dtype=torch.float32, device=dev)
    want_trace = return_info or verbose > 0
    cap = max(maxiter, 1)
    deltas, losses = (C.c_double * cap)(), (C.c_double * cap)()
    trace = nat.IstaNlTrace(cap, verbose, deltas, losses)
    options = nat.IstaNlOptions(maxiter, 1 if fast else 0, 1 if lr_auto else 0, power_iters, 0.0 if lr_auto else lr,
                                float(tol), 0)
    res = nat.IstaNlResult()
    l_row = torch.empty(n, dtype=torch.float32, device=dev) if lr_auto and return_info else None
    res.l_dev = l_row.data_ptr() if l_row is not None else None
    L = nat.lib()
    with torch.cuda.device(dev):
        ws = nat.workspace(dev, L.lasso_ista_nl_workspace_bytes(n, d, k, nat.LASSO_F32, 1 if lr_auto else 0), "ista_nl")
        status = L.lasso_ista_nl_solve(nat.ptr(xg), xg.stride(0) if n > 1 else d, nat.ptr(wg), wg.stride(0) if d > 1 else k,
                                       nat.ptr(bg), nat.ptr(z0g), k, nat.ptr(z), k, nat.ptr(ug), k, n, d, k, nat.LASSO_F32,
                                       float(alpha), _ACTIVATIONS[dec.activation], C.byref(options), C.byref(res),
                                       C.byref(trace) if want_trace else None, nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
    nat.check(status)
    its = res.n_iter
    if want_trace:
        info = dict(iterations=its, deltas=list(deltas[:its]), stopped=bool(res.stopped),
                    L=l_row if (l_row is not None and its > 0) else None)
    if verbose > 0:
        print('initial loss: %0.4f' % res.f0)                                           # ista.py:98
        if verbose > 1:
            for i in range(its - (1 if res.stopped else 0)):                          # (:117-118: not the one that stops)
                print('iter %3d - loss: %0.4f' % (i + 1, losses[i]))
        print('final loss: %0.4f' % res.f_final)                                        # :121
    z = z.to(device=out_device)
    if info['L'] is not None:
        info['L'] = info['L'].to(device=out_device)
    return (z, info) if return_info else z
