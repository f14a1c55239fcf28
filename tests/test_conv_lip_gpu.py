"""lasso_amd.conv2d.lip_constant and ista_conv2d(lr='exact') on the GPU against tests/golden/conv_lip_cases.npz (the real
reference's ARPACK values, float32 and float64, both transposes).

The parity bar of a case is ``tol + 4 * max(gap32, spread32)`` (float64: ``tol + 4 * spread64``): ``tol`` is the stop
rule's own relative residual bound, gap32 how far the reference's float32 run is from its float64 run and spread how far
"another correct implementation" (tests/conv_lip_model.py: permuted summation orders, dots folded in double, other start
vectors) moves the value -- all read from the fixture, none from the code under test.  Measured deviations are recorded
next to the bars (tests/margins.py).

Measured on an MI355X (|L - ref64| / ref64, profiles/conv_lip/parity_margins.json): float32 1.3e-9 to 2.4e-8 against
bars of 1.0e-5 to 1.6e-5 (the exhausted case with tol = 0: 4.9e-9 against 1.2e-6), float64 at most 2.7e-15 against 1e-10
(exhausted: 2.2e-16 against 2.6e-15)."""
import math
import warnings

import numpy as np
import pytest
import torch

from conv_lip_cases import (CASES, EXACT_LR_ALPHA, EXACT_LR_CASE, EXACT_LR_ITERS, PARITY, conv_kwargs, dims,
                            exact_lr_image, imsize_of, kernel_of, load_case, parity_bar, tol_of)
from margins import record_margins

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
_ids = {torch.float32: "f32", torch.float64: "f64"}


@pytest.fixture(scope="module")
def cases(golden):
    return golden("conv_lip_cases")


def _lip(spec, dtype, transpose=False, **kw):
    from lasso_amd.conv2d import lip_constant
    if "tol" in spec and "tol" not in kw:
        kw["tol"] = spec["tol"]
    return lip_constant(kernel_of(spec, dtype).cuda(), imsize_of(spec, transpose), transpose=transpose, **kw, **conv_kwargs(spec))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
@pytest.mark.parametrize("name", PARITY)
def test_value_matches_the_reference(cases, name, dtype):
    spec, g = CASES[name], load_case(cases, name)
    ref64, bar = float(g["ref64"][0]), parity_bar(g, dtype, tol_of(spec, dtype))
    devs, infos = [], []
    for transpose in (False, True):
        v, info = _lip(spec, dtype, transpose, return_info=True)
        devs.append(abs(v - ref64) / ref64)
        infos.append(info)
        assert info["status"] in ("converged", "breakdown") and info["dim"] == min(dims(spec))
        assert info["space"] == ("code" if dims(spec)[1] < dims(spec)[0] else "image")
        assert info["theta"] == v and info["steps"] == len(info["history"]) and info["history"][-1] == v
        assert info["residual"] <= max(tol_of(spec, dtype), 1e-300) * v or info["status"] == "breakdown"
    record_margins("conv_lip/%s_%s" % (name, _ids[dtype]), dict(dev=devs, bar=bar, steps=[i["steps"] for i in infos],
                                                                status=[i["status"] for i in infos]))
    print("%s %s: dev %r bar %.3g steps %r" % (name, _ids[dtype], devs, bar, [i["steps"] for i in infos]))
    # both transposes name the same operator pair and run the same iteration: the same bits
    assert infos[0]["theta"] == infos[1]["theta"]
    assert max(devs) <= bar, (devs, bar)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
def test_sqrt_determinism_and_detach(dtype):
    from lasso_amd.conv2d import lip_constant
    spec = CASES["rect_s2"]
    v = _lip(spec, dtype)
    assert isinstance(v, float) and _lip(spec, dtype) == v                          # two calls: the same bits
    assert _lip(spec, dtype, sqrt=True) == math.sqrt(v)
    w = kernel_of(spec, dtype).cuda().requires_grad_()
    assert lip_constant(w, spec["imsize"], **conv_kwargs(spec)) == v                # detached; no graph is built
    assert lip_constant(kernel_of(spec, dtype), spec["imsize"], **conv_kwargs(spec)) == v   # a CPU kernel is staged


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
def test_chunking_does_not_matter(dtype):
    spec = CASES["rgb"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, full = _lip(spec, dtype, tol=0.0, maxiter=40, return_info=True)
    assert full["steps"] == 40 and full["host_reads"] == 3 and full["status"] == "maxiter"     # chunks of 8, 16, 16
    for cut, reads in ((5, 1), (8, 1), (13, 2)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            v, info = _lip(spec, dtype, tol=0.0, maxiter=cut, return_info=True)
        assert v == full["history"][cut - 1] and info["history"] == full["history"][:cut]
        assert info["steps"] == cut and info["matvecs"] == cut and info["host_reads"] == reads
    # a stop inside a chunk returns the value of the step that stopped: the default run's theta is in the long history
    v, info = _lip(spec, dtype, return_info=True)
    assert info["status"] == "converged"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, longer = _lip(spec, dtype, tol=0.0, maxiter=info["steps"] + 3, return_info=True)
    assert longer["history"][info["steps"] - 1] == v
    assert info["matvecs"] >= info["steps"]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
def test_status(cases, dtype):
    eps = float(torch.finfo(dtype).eps)
    v, info = _lip(CASES["delta"], dtype, return_info=True)
    assert info["status"] == "breakdown" and info["steps"] == 1 and info["host_reads"] == 1
    assert abs(v - 1.0) <= 4 * eps
    v, info = _lip(CASES["one"], dtype, return_info=True)                           # dim = 1: the value is w^2
    w = float(kernel_of(CASES["one"], dtype).double().reshape(()))
    assert info["status"] == "breakdown" and info["dim"] == 1 and abs(v - w * w) <= 4 * eps * w * w
    v, info = _lip(CASES["exhaust"], dtype, return_info=True)                       # tol = 0: to the end of the space
    assert info["status"] == "breakdown" and info["steps"] <= 64 and info["dim"] == 64
    with pytest.warns(RuntimeWarning, match="maxiter=3") as rec:
        v, info = _lip(CASES["rgb"], dtype, maxiter=3, return_info=True)
    assert len(rec) == 1 and info["status"] == "maxiter" and info["steps"] == 3 and info["host_reads"] == 1
    assert 0 < v < float(load_case(cases, "rgb")["ref64"][0])                       # a Ritz value: from below
    v, info = _lip(CASES["zero"], dtype, return_info=True)
    assert v == 0.0 and info["status"] == "breakdown"
    v, info = _lip(CASES["nan"], dtype, return_info=True)
    assert math.isnan(v) and info["status"] == "nonfinite" and info["host_reads"] == 1
    assert math.isnan(_lip(CASES["nan"], dtype, sqrt=True))
    w = kernel_of(CASES["rect"], dtype)
    w[0, 0, 0, 0] = float("inf")
    from lasso_amd.conv2d import lip_constant
    assert math.isnan(lip_constant(w.cuda(), CASES["rect"]["imsize"], **conv_kwargs(CASES["rect"])))


def test_a_run_that_ends_in_its_first_chunk_reads_once():
    # the first chunk is 8 steps: a run capped at 8 ends in it whatever it finds (on an MI355X: 'maxiter', float32
    # needs 17 steps for 1e-5 here), and a loose tol stops inside it with the chunk's launches all made
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, info = _lip(CASES["few_atoms"], torch.float32, maxiter=8, return_info=True)
    assert info["steps"] == 8 and info["host_reads"] == 1 and info["matvecs"] == 8
    _, info = _lip(CASES["few_atoms"], torch.float32, tol=0.5, return_info=True)
    if info["steps"] <= 8:
        assert info["status"] == "converged" and info["host_reads"] == 1 and info["matvecs"] == 8
    else:
        assert info["host_reads"] >= 2


def test_restart_when_the_basis_is_full():
    """more steps than the 512 basis vectors of a cycle: the iteration goes on from the Ritz vector, theta keeps rising"""
    spec = CASES["c16"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        v, info = _lip(spec, torch.float32, tol=0.0, maxiter=520, return_info=True)
    assert info["restarts"] == 1 and info["steps"] == 520 and info["status"] == "maxiter"
    h = info["history"]
    # the first Ritz value of the new cycle is the Rayleigh quotient of the old Ritz vector, rounded to float32 once:
    # second order in that rounding (6e-8 per element), so 1e-5 is far outside it
    assert abs(h[512] - h[511]) <= 1e-5 * h[511] and abs(v - h[511]) <= 1e-5 * v


# ---- ista_conv2d(lr='exact') ---------------------------------------------------------------------------------------------
def _ista_inputs(spec, dtype):
    w = kernel_of(spec, dtype).cuda()
    x = exact_lr_image(spec, dtype).cuda()
    z0 = torch.zeros_like(torch.nn.functional.conv2d(x, w, **conv_kwargs(spec)))
    return x, z0, w


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
def test_exact_lr_is_the_explicit_step(dtype):
    from lasso_amd.conv2d import ista_conv2d, lip_constant
    for name in (EXACT_LR_CASE, "rect_s2"):                                         # stride 2: lr='auto' has no step there
        spec = CASES[name]
        x, z0, w = _ista_inputs(spec, dtype)
        kw = dict(alpha=EXACT_LR_ALPHA, maxiter=6, tol=0.0, **conv_kwargs(spec))
        _, info = lip_constant(w, spec["imsize"], return_info=True, **conv_kwargs(spec))
        z = ista_conv2d(x, z0, w, lr="exact", **kw)
        assert torch.equal(z, ista_conv2d(x, z0, w, lr=1.0 / (info["theta"] + info["residual"]), **kw))
        assert z.abs().sum().item() > 0
    with pytest.raises(NotImplementedError):
        ista_conv2d(x, z0, w, lr="auto", **kw)
    # a constant of the graph, like 'auto'
    wg = w.clone().requires_grad_()
    zg = ista_conv2d(x, z0, wg, lr="exact", **kw)
    zg.sum().backward()
    assert torch.equal(zg.detach(), z) and wg.grad is not None and torch.isfinite(wg.grad).all()


def test_exact_lr_reaches_a_lower_loss_than_auto(cases):
    from lasso_amd.conv2d import ista_conv2d
    from lasso_amd.conv2d.ista import conv_loss
    spec = CASES[EXACT_LR_CASE]
    assert float(cases["exact_lr/ratio"]) >= 1.5                                    # the bound is far from the constant
    x, z0, w = _ista_inputs(spec, torch.float32)
    kw = dict(alpha=EXACT_LR_ALPHA, maxiter=EXACT_LR_ITERS, tol=0.0, **conv_kwargs(spec))
    losses = {lr: conv_loss(x, ista_conv2d(x, z0, w, lr=lr, **kw), w, EXACT_LR_ALPHA, **conv_kwargs(spec)).item()
              for lr in ("exact", "auto")}
    record_margins("conv_lip/exact_lr_loss", dict(losses, model_exact=float(cases["exact_lr/loss_exact"]),
                                                  model_auto=float(cases["exact_lr/loss_auto"])))
    assert losses["exact"] < losses["auto"]
    assert abs(losses["auto"] - float(cases["exact_lr/loss_auto"])) <= 1e-3 * losses["auto"]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
def test_auto_and_numeric_lr_take_the_path_they_took(dtype):
    """bitwise the direct call of the native path that lr='auto' and a numeric lr reached before lr='exact' existed"""
    from lasso_amd import _native as nat
    from lasso_amd.conv2d import ista_conv2d, lip_bound_conv2d
    from lasso_amd.conv2d import ista as mod
    spec = CASES["rect"]
    x, z0, w = _ista_inputs(spec, dtype)
    P = mod._path("ista_conv2d", x, z0, w)
    geom = mod._geometry(x, z0, w, spec["stride"], spec["padding"])
    dev = nat.pick_device(x, w, z0)

    def direct(lr):
        return mod._solve(P, x, z0, w, geom, 0.1, lr, True, 7, 1e-5, False, dev)[0]

    assert torch.equal(ista_conv2d(x, z0, w, alpha=0.1, lr=0.02, maxiter=7, **conv_kwargs(spec)), direct(0.02))
    Lb = lip_bound_conv2d(w, spec["padding"])
    lr = 1.0 / Lb.item() if dtype == torch.float64 else float(np.float32(1.0) / np.float32(Lb.item()))
    assert torch.equal(ista_conv2d(x, z0, w, alpha=0.1, lr="auto", maxiter=7, **conv_kwargs(spec)), direct(lr))
