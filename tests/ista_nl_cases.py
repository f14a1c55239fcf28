"""The golden cases of ``ista_nl`` (tests/golden/ista_nl_cases.npz): shapes, seeds and arguments, shared by the generator
(tests/golden/generate_golden_ista_nl.py) and the tests.  Inputs: unit-norm atoms W [d,k], a 10 %-sparse code,
x = decoder(2 code) + 0.01 noise with decoder(z) = act(z W^T + b); the bias is 0.1 randn, for ReLU 0.5 + |0.1 randn| so
that every row is alive at the zero start; a zero start unless the case says 'warm'.

The generator ran the REAL reference (``torch.randn_like`` patched to return the case's ``power_init``) in float32 and
float64 and certified every case: every code finite, some code non-zero, no sum |z - z_next| within 1 % of the stop
budget, and spread_z -- how far "another correct float32 implementation" (tests/ista_nl_model.py with permuted
summation orders, the normalisation folded behind the product, and the link in float64 rounded once) moves the codes --
at most SPREAD_Z_CAP = 2.5e-3 for every case: all are compared by their codes.

A fixed step must stay below 1 / L of its case: about 1 / (1 + sqrt(k / d))^2 for the identity (0.1 here), four times
that under the sigmoid's slope of 1/4; WIDE (k = 4100, L ~ 560) takes 'auto'."""
import torch
import torch.nn.functional as F

from owlqn_cases import SPREAD_Z_CAP, load_case  # noqa: F401

import ista_nl_model as model

ORDER_SEEDS = (1, 2, 3, 4)

SMALL, MID, TALL, RAGGED, WIDE = (5, 7, 19), (24, 16, 40), (70, 20, 33), (33, 48, 130), (3, 8, 4100)
BLOCKS = (130, 70, 140)               # crosses a 128-row and a 128-column block boundary and a 64-wide contraction chunk

ALPHA = dict(identity=0.1, sigmoid=0.01, tanh=0.05, relu=0.05)
BIG_ALPHA = 8.0                       # x ALPHA for shapes of more than 1000 codes: sparser codes, a smaller fixture
FIXED_LR = dict(identity=0.1, sigmoid=0.5, tanh=0.1, relu=0.1)


def _case(shape, activation, lr, seed=0, bias=True, fast=True, maxiter=10, tol=0.0, power_iters=10, start="zero", alpha=None):
    n, d, k = shape
    return dict(n=n, d=d, k=k, seed=seed, activation=activation, bias=bias, start=start,
                alpha=(ALPHA[activation] * (BIG_ALPHA if n * k > 1000 else 1.0)) if alpha is None else alpha,
                kwargs=dict(fast=fast, maxiter=maxiter, lr=lr, power_iters=power_iters, tol=tol))


CASES = {}
# every activation at SMALL, MID and BLOCKS under both step rules; bias, momentum and the iteration count vary with them
for _act in model.ACTIVATIONS:
    for _tag, _shape, _it in (("small", SMALL, 20), ("mid", MID, 12), ("blocks", BLOCKS, 6)):
        _plain = _act in ("identity", "tanh") and _tag == "mid"          # no bias, no momentum
        CASES["%s_%s_fixed" % (_act, _tag)] = _case(_shape, _act, FIXED_LR[_act], bias=not _plain, fast=not _plain, maxiter=_it)
        CASES["%s_%s_auto" % (_act, _tag)] = _case(_shape, _act, "auto", bias=_act != "sigmoid" or _tag != "small",
                                                   fast=_tag != "small" or _act != "relu", maxiter=min(_it, 8),
                                                   power_iters=10 if _tag != "blocks" else 4)
CASES.update({
    "sigmoid_tall_fixed": _case(TALL, "sigmoid", 0.5, maxiter=10),
    "tanh_tall_auto": _case(TALL, "tanh", "auto", maxiter=6, bias=False, power_iters=5),
    "identity_ragged_fixed": _case(RAGGED, "identity", 0.1, maxiter=10, start="warm"),
    "relu_ragged_auto": _case(RAGGED, "relu", "auto", maxiter=6, power_iters=5),
    "sigmoid_wide_auto": _case(WIDE, "sigmoid", "auto", maxiter=5, power_iters=6),
    "identity_wide_auto": _case(WIDE, "identity", "auto", maxiter=5, power_iters=6, bias=False),
    # the stop rule fires mid-run
    "sigmoid_mid_stop": _case(MID, "sigmoid", 0.5, maxiter=200, tol=1e-3),
    "tanh_small_stop_auto": _case(SMALL, "tanh", "auto", maxiter=100, tol=1e-3, fast=False),
})


def recipe(n, d, k, seed, activation, bias=True):
    """x [n,d], W [d,k] (unit-norm atoms), b [d] or None"""
    g = torch.Generator().manual_seed(seed)
    w = F.normalize(torch.randn(d, k, generator=g), dim=0)
    code = torch.randn(n, k, generator=g) * (torch.rand(n, k, generator=g) < 0.1)
    b = 0.1 * torch.randn(d, generator=g)
    if activation == "relu":
        b = 0.5 + b.abs()
    noise = 0.01 * torch.randn(n, d, generator=g)
    b = b if bias else None
    return model.decode(activation, 2.0 * code, w, b) + noise, w, b


def case_inputs(spec):
    """x [n,d], W [d,k], b [d] or None, z0 [n,k], power_init [n,k]"""
    n, k = spec["n"], spec["k"]
    x, w, b = recipe(n, spec["d"], k, spec["seed"], spec["activation"], spec["bias"])
    g = torch.Generator().manual_seed(1000 + spec["seed"])
    z0 = torch.zeros(n, k)
    warm = 0.3 * torch.randn(n, k, generator=g) * (torch.rand(n, k, generator=g) < 0.25)
    if spec["start"] == "warm":
        z0 = warm
    return x, w, b, z0, torch.randn(n, k, generator=g)


def run_model(spec, **kw):
    x, w, b, z0, u0 = case_inputs(spec)
    return model.ista_nl(x, z0, w, b, spec["activation"], alpha=spec["alpha"], power_init=u0, **dict(spec["kwargs"], **kw))
