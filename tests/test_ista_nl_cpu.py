"""``ista_nl`` without a GPU: the host model against the reference's recorded runs (tests/golden/ista_nl_cases.npz), the
public signature against the reference's, which decoders are recognised, and the loud failure without a device."""
import inspect

import numpy as np
import pytest
import torch

import ista_nl_model as model
from ista_nl_cases import CASES, SPREAD_Z_CAP, case_inputs, load_case, run_model


@pytest.fixture(scope="module")
def cases(golden):
    return golden("ista_nl_cases")


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_in_reference_order_is_the_recorded_run(cases, name):
    spec, g = CASES[name], load_case(cases, name)
    spread = float(g["spread_z"])
    assert spread <= SPREAD_Z_CAP
    z, info = run_model(spec)
    want = torch.from_numpy(g["z32"])
    assert info["iterations"] == len(g["deltas32"]) and info["stopped"] == bool(g["stopped"])
    if spec["activation"] == "identity":
        assert torch.equal(z, want)
        assert info["deltas"] == list(g["deltas32"])
    else:
        assert float((z - want).abs().max()) <= 4.0 * spread
    z64, i64 = run_model(spec, dtype=torch.float64)
    assert i64["iterations"] == len(g["deltas64"])
    np.testing.assert_allclose(i64["deltas"], g["deltas64"], rtol=1e-9, atol=1e-12)
    if "z64" in g:
        assert float((z64 - torch.from_numpy(g["z64"])).abs().max()) <= 1e-12
    if spec["kwargs"]["lr"] == "auto":
        assert float(((i64["L"] - torch.from_numpy(g["L64"])).abs() / torch.from_numpy(g["L64"]).abs()).max()) <= 1e-9


def test_every_activation_is_covered_at_small_mid_and_blocks_under_both_step_rules():
    for act in model.ACTIVATIONS:
        for tag in ("small", "mid", "blocks"):
            assert CASES["%s_%s_fixed" % (act, tag)]["kwargs"]["lr"] != "auto"
            assert CASES["%s_%s_auto" % (act, tag)]["kwargs"]["lr"] == "auto"
    assert all(spec["kwargs"]["maxiter"] <= 20 or spec["kwargs"]["tol"] > 0 for spec in CASES.values())
    assert any(not s["bias"] for s in CASES.values()) and any(not s["kwargs"]["fast"] for s in CASES.values())


def test_signature_and_defaults_are_the_reference_s():
    from lasso_amd.nonlinear import ista_nl
    sig = inspect.signature(ista_nl)
    assert list(sig.parameters) == ["x", "z0", "decoder", "alpha", "fast", "maxiter", "lr", "power_iters", "tol", "eval_mode",
                                    "verbose", "power_init", "return_info"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(alpha=1.0, fast=True, maxiter=10, lr="auto", power_iters=10, tol=1e-5, eval_mode=True, verbose=0,
                     power_init=None, return_info=False)


def test_decoders_that_are_recognised():
    from lasso_amd.nonlinear import affine
    from lasso_amd.nonlinear.ista import _describe
    nn = torch.nn
    lin = nn.Linear(19, 7)
    got = _describe(lin)
    assert got.weight is lin.weight and got.bias is lin.bias and got.activation == "identity"
    assert _describe(nn.Linear(19, 7, bias=False)).bias is None
    for mod, act in ((nn.Identity, "identity"), (nn.Sigmoid, "sigmoid"), (nn.Tanh, "tanh"), (nn.ReLU, "relu")):
        got = _describe(nn.Sequential(lin, mod()))
        assert got.weight is lin.weight and got.bias is lin.bias and got.activation == act
    w = torch.randn(7, 19)
    assert _describe(affine(w)) == affine(w, None, "identity")
    assert _describe(affine(w, torch.zeros(7), "tanh")).activation == "tanh"
    assert affine._fields == ("weight", "bias", "activation")


@pytest.mark.parametrize("make,named", [
    (lambda nn: nn.Sequential(nn.Linear(19, 7), nn.GELU()), "GELU"),
    (lambda nn: nn.Sequential(nn.Linear(19, 12), nn.Tanh(), nn.Linear(12, 7)), "Linear, Tanh, Linear"),
    (lambda nn: nn.Sequential(nn.Tanh(), nn.Linear(19, 7)), "Tanh, Linear"),
    (lambda nn: nn.Sequential(nn.Linear(19, 7)), "Sequential(Linear)"),
    (lambda nn: nn.Bilinear(19, 19, 7), "Bilinear"),
    (lambda nn: nn.Conv1d(19, 7, 1), "Conv1d"),
    (lambda nn: (lambda z: z), "function"),
])
def test_other_decoders_are_refused_by_name(make, named):
    from lasso_amd.nonlinear import ista_nl
    with pytest.raises(NotImplementedError, match=named.replace("(", r"\(").replace(")", r"\)")):
        ista_nl(torch.zeros(5, 7), torch.zeros(5, 19), make(torch.nn), lr=0.1)


def test_an_unknown_activation_name_and_other_dtypes_are_refused_by_name():
    from lasso_amd.nonlinear import affine, ista_nl
    with pytest.raises(NotImplementedError, match="softplus"):
        ista_nl(torch.zeros(5, 7), torch.zeros(5, 19), affine(torch.zeros(7, 19), None, "softplus"), lr=0.1)
    with pytest.raises(NotImplementedError, match="float64"):
        ista_nl(torch.zeros(5, 7).double(), torch.zeros(5, 19).double(), affine(torch.zeros(7, 19).double()), lr=0.1)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        ista_nl(torch.zeros(5, 7), torch.zeros(5, 19).bfloat16(), affine(torch.zeros(7, 19)), lr=0.1)


@pytest.mark.parametrize("lr", [1, None, "Auto", torch.tensor(0.1)])
def test_lr_is_a_float_or_auto(lr):
    from lasso_amd.nonlinear import affine, ista_nl
    with pytest.raises(ValueError, match='expected `lr` to be either float or "auto".'):
        ista_nl(torch.zeros(5, 7), torch.zeros(5, 19), affine(torch.zeros(7, 19)), lr=lr)


def test_module_flags_are_untouched_and_the_call_fails_loudly_without_a_gpu():
    from lasso_amd import NativeError
    from lasso_amd.nonlinear import ista_nl
    spec = CASES["sigmoid_small_fixed"]
    x, w, b, z0, _ = case_inputs(spec)
    lin = torch.nn.Linear(19, 7)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(b)
    lin.bias.requires_grad_(False)
    decoder = torch.nn.Sequential(lin, torch.nn.Sigmoid()).train()
    before = (lin.weight.detach().clone(), lin.bias.detach().clone())
    try:
        z = ista_nl(x, z0, decoder, alpha=spec["alpha"], **spec["kwargs"])
    except NativeError:
        assert not torch.cuda.is_available()          # no CPU fallback: fails loudly
    else:
        assert torch.cuda.is_available() and z.device.type == "cpu" and not z.requires_grad
    assert decoder.training and lin.training and lin.weight.requires_grad and not lin.bias.requires_grad
    assert torch.equal(lin.weight.detach(), before[0]) and torch.equal(lin.bias.detach(), before[1])
    if not torch.cuda.is_available():
        with pytest.raises(NativeError):
            ista_nl(x, z0, decoder, alpha=spec["alpha"], lr=0.1)
