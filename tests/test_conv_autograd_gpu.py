"""Differentiable convolutional solve (SURVEY.md 8f rows f3 + f4): gradients of ista_conv2d
(lasso_conv_ista_run_traced + lasso_conv_ista_backward, csrc/conv_autograd.hip) against
torch.autograd through the CPU oracle's unrolled conv_fista loop -- how the reference itself is
differentiated (lasso/conv2d/ista.py:7-49 is plain torch code).  Tolerance as for the linear
solver: 2e-4 of the gradient's max magnitude."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G_RTOL = 2e-4


def _mods():
    from lasso_amd import _native as nat
    from lasso_amd.conv2d import ista_conv2d
    from oracle import lasso_oracle as orc
    return ista_conv2d, nat, orc


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# (form, N spec, C, K, kh, kw, stride, padding, Hz, Wz); N spec >= 0: CUs + spec images, < 0: CUs // -spec,
# a tuple (n,): n images.  Geometries of tests/test_conv_gpu.py, shrunk where they are large.
GEOMS = [
    ("fused", 3, 1, 100, 3, 3, 1, 1, 9, 9),                       # a workgroup per image; K % 16 != 0, two atom tiles
    ("fused", -4, 2, 48, 3, 3, 1, 1, 40, 24),                     # bands of code rows
    ("conv_synth_kernel", (3,), 8, 32, 3, 3, 1, 1, 12, 12),       # 8 <= C <= 16
    ("conv_synth_few_kernel", (3,), 2, 24, 7, 7, 1, 3, 12, 11),   # C < 8, 98 taps (beyond the fused kernel's 80)
    ("explicit", (3,), 2, 12, 3, 3, 2, 1, 6, 7),                  # stride 2
    ("explicit", (2,), 3, 20, 3, 5, (1, 2), (1, 2), 5, 6),        # stride (1, 2), asymmetric padding, 3 x 5 kernel
    ("explicit", (2,), 17, 8, 3, 3, 1, 1, 6, 6),                  # C = 17: 153 taps, three tap tiles
]


def _n(spec):
    if isinstance(spec, tuple):
        return spec[0]
    return _cus() + spec if spec >= 0 else _cus() // -spec


def _problem(geom, seed=0):
    form, spec, C, K, kh, kw, stride, padding, Hz, Wz = geom
    N = _n(spec)
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    H, W = (Hz - 1) * sh - 2 * ph + kh, (Wz - 1) * sw - 2 * pw + kw
    g = torch.Generator().manual_seed(seed + 7 * K + Hz)
    w = torch.randn(K, C, kh, kw, generator=g) / (C * kh * kw) ** 0.5
    x = torch.randn(N, C, H, W, generator=g)
    z0 = torch.randn(N, K, Hz, Wz, generator=g) * 0.05
    G = torch.randn(N, K, Hz, Wz, generator=g)
    lr = 0.3 / max(w.pow(2).sum().item(), 1e-3)
    return x, w, z0, G, lr, stride, padding


def _assert_form(geom):
    form, spec, C, K, kh, kw, stride, padding, Hz, Wz = geom
    _, nat, _ = _mods()
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    N = _n(spec)
    args = (N, C, (Hz - 1) * sh - 2 * ph + kh, (Wz - 1) * sw - 2 * pw + kw, K, Hz, Wz, kh, kw, sh, sw, ph, pw)
    name = nat.lib().lasso_conv_ista_kernel_name(*args).decode()
    if form == "fused":
        assert "conv_fused_kernel" in name, name
    elif form == "explicit":
        assert "conv_residual_kernel" in name, name
    else:
        assert "conv_fused_kernel" not in name and ("lasso::" + form) in name, name


def _grads(fn, x, w, z0, G, dev, need=(True, True, True)):
    xl = x.detach().clone().to(dev).requires_grad_(need[0])
    wl = w.detach().clone().to(dev).requires_grad_(need[1])
    zl = z0.detach().clone().to(dev).requires_grad_(need[2])
    z = fn(xl, zl, wl)
    (z * G.to(dev)).sum().backward()
    return z.detach().cpu(), [None if t.grad is None else t.grad.cpu() for t in (xl, wl, zl)]


def _close(got, ref, what):
    for name, a, b in zip(("dx", "dW", "dz0"), got, ref):
        if b is None:
            assert a is None, (what, name)
            continue
        assert a.shape == b.shape, (what, name)
        err = (a - b).abs().max().item() if b.numel() else 0.0
        assert err <= G_RTOL * max(b.abs().max().item() if b.numel() else 0.0, 1e-3), (what, name, err)


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%s-C%d-K%d" % (g[0], g[2], g[3]))
def test_gradients_match_autograd_through_the_oracle(geom):
    ista_conv2d, _, orc = _mods()
    _assert_form(geom)
    x, w, z0, G, lr, stride, padding = _problem(geom)
    for fast in (True, False):
        for T in (1, 6):
            kw_ = dict(stride=stride, padding=padding, fast=fast, maxiter=T, lr=lr, tol=0.0)
            zr, ref = _grads(lambda a, b, c: orc.conv_fista(a, b, c, 0.1, **kw_), x, w, z0, G, "cpu")
            zg, got = _grads(lambda a, b, c: ista_conv2d(a, b, c, 0.1, **kw_), x, w, z0, G, "cuda")
            assert (zg - zr).abs().max().item() <= 5e-5
            _close(got, ref, (fast, T))


def test_weight_gradient_forms_agree():
    """conv_wgrad_kernel against the conv_patches + gram_tn composition it replaces (LASSO_CONV_WGRAD=gram)."""
    ista_conv2d, _, _ = _mods()
    x, w, z0, G, lr, stride, padding = _problem(GEOMS[6])
    fn = lambda a, b, c: ista_conv2d(a, b, c, 0.1, stride=stride, padding=padding, maxiter=5, lr=lr, tol=0.0)  # noqa: E731
    _, fused = _grads(fn, x, w, z0, G, "cuda")
    os.environ["LASSO_CONV_WGRAD"] = "gram"
    try:
        _, gram = _grads(fn, x, w, z0, G, "cuda")
    finally:
        os.environ.pop("LASSO_CONV_WGRAD", None)
    _close(fused, gram, "gram")
    assert torch.equal(fused[0], gram[0]) and torch.equal(fused[2], gram[2])     # only dW differs in form


@pytest.mark.parametrize("geom", GEOMS[:5], ids=lambda g: "%s-C%d-K%d" % (g[0], g[2], g[3]))
def test_forward_unchanged(geom):
    """The differentiable call returns bitwise the z, iteration count and last delta of the call without grad -- with
    no stop rule and with a budget the sums cross inside a speculated chunk (just above the sum of iteration 23)."""
    ista_conv2d, _, _ = _mods()
    x, w, z0, _, lr, stride, padding = _problem(geom)
    xg, wg, zg = x.cuda(), w.cuda(), z0.cuda()
    kw_ = dict(stride=stride, padding=padding, lr=lr, return_info=True)
    runs = []
    for fast in (True, False):
        _, probe = ista_conv2d(xg, zg, wg, 0.1, fast=fast, maxiter=23, tol=1e-30, **kw_)
        runs += [(fast, 9, 0.0), (fast, 150, float(np.float32(probe["last_delta"]) * np.float32(1.0 + 1e-4)) / z0.numel())]
    for fast, maxiter, t in runs:
        z_plain, i_plain = ista_conv2d(xg, zg, wg, 0.1, fast=fast, maxiter=maxiter, tol=t, **kw_)
        z_grad, i_grad = ista_conv2d(xg, zg, wg.clone().requires_grad_(True), 0.1, fast=fast, maxiter=maxiter, tol=t,
                                     **kw_)
        assert z_grad.grad_fn is not None and z_plain.grad_fn is None
        assert torch.equal(z_grad.detach(), z_plain), (fast, maxiter)
        assert i_grad["iterations"] == i_plain["iterations"]
        assert (math.isnan(i_grad["last_delta"]) and math.isnan(i_plain["last_delta"])) or \
            i_grad["last_delta"] == i_plain["last_delta"]
        if t > 0:
            assert i_plain["iterations"] <= 23, i_plain
            assert fast or i_plain["iterations"] > 1, i_plain     # (the ISTA sums decrease: the rule fires late)


@pytest.mark.parametrize("gi,fast", [(3, True), (4, False)])
def test_early_stop_matches_the_oracle(gi, fast):
    """tol > 0: the gradient covers the T iterations the ordinary solve runs -- the oracle's T, exactly (a budget with
    room on both sides of the oracle's sums, as tests/test_conv_gpu.py places it)."""
    ista_conv2d, _, orc = _mods()
    x, w, z0, G, lr, stride, padding = _problem(GEOMS[gi], seed=5)
    kw_ = dict(stride=stride, padding=padding, lr=lr, fast=fast)
    sums = [orc.conv_fista(x, z0, w, 0.1, maxiter=m, tol=0.0, return_info=True, **kw_)[1]["last_delta"]
            for m in range(1, 26)]
    pick = None
    for m in range(4, 25):
        lo, hi = sums[m - 1], min(sums[:m - 1])
        if lo < hi and hi / lo >= 1.03:
            pick, budget = m, math.sqrt(lo * hi)
            break
    assert pick is not None, sums
    tol = budget / z0.numel()
    zr, ref = _grads(lambda a, b, c: orc.conv_fista(a, b, c, 0.1, maxiter=200, tol=tol, **kw_), x, w, z0, G, "cpu")
    info = {}

    def run(a, b, c):
        z, i = ista_conv2d(a, b, c, 0.1, maxiter=200, tol=tol, return_info=True, **kw_)
        info.update(i)
        return z
    zg, got = _grads(run, x, w, z0, G, "cuda")
    assert info["iterations"] == pick
    assert (zg - zr).abs().max().item() <= 5e-5
    _close(got, ref, "tol")


def test_partial_requires_grad():
    ista_conv2d, _, orc = _mods()
    x, w, z0, G, lr, stride, padding = _problem(GEOMS[3], seed=2)
    kw_ = dict(stride=stride, padding=padding, maxiter=4, lr=lr, tol=0.0)
    for need in ((False, True, False), (True, False, False), (False, False, True)):
        _, ref = _grads(lambda a, b, c: orc.conv_fista(a, b, c, 0.1, **kw_), x, w, z0, G, "cpu", need)
        _, got = _grads(lambda a, b, c: ista_conv2d(a, b, c, 0.1, **kw_), x, w, z0, G, "cuda", need)
        _close(got, ref, need)


def test_auto_lr_cpu_leaves_and_edge_cases():
    """lr='auto' with a weight that requires grad: the step is the package's detached Toeplitz bound, a constant (the
    reference raises TypeError here); CPU leaves get CPU gradients; N = 0 and maxiter = 0."""
    from lasso_amd.conv2d import lip_bound_conv2d
    ista_conv2d, _, orc = _mods()
    x, w, z0, G, _, _, _ = _problem(("", (2,), 1, 8, 5, 5, 1, 2, 10, 10), seed=4)
    lr = float(np.float32(1.0) / np.float32(lip_bound_conv2d(w.cuda(), 2).item()))
    _, ref = _grads(lambda a, b, c: orc.conv_fista(a, b, c, 0.2, padding=2, maxiter=5, lr=lr, tol=0.0), x, w, z0, G,
                    "cpu")
    xl, wl, zl = (t.clone().requires_grad_(True) for t in (x, w, z0))
    z = ista_conv2d(xl, zl, wl, 0.2, padding=2, maxiter=5, lr='auto', tol=0.0)
    assert z.device.type == "cpu"
    (z * G).sum().backward()
    got = [xl.grad, wl.grad, zl.grad]
    assert all(t.device.type == "cpu" for t in got)
    _close(got, ref, "auto")
    # N = 0: gradients of the right shapes
    xe, ze = x[:0].cuda().requires_grad_(True), z0[:0].cuda().requires_grad_(True)
    we = w.cuda().requires_grad_(True)
    ze_out = ista_conv2d(xe, ze, we, 0.2, padding=2, maxiter=5, lr=lr, tol=0.0)
    ze_out.sum().backward()
    assert xe.grad.shape == xe.shape and ze.grad.shape == ze.shape
    assert we.grad.shape == we.shape and torch.equal(we.grad, torch.zeros_like(we))
    # maxiter = 0: z0 itself
    z0d = z0.cuda().requires_grad_(True)
    assert ista_conv2d(x.cuda(), z0d, w.cuda().requires_grad_(True), padding=2, maxiter=0, lr=lr) is z0d


def test_deterministic_without_aten_convolutions(monkeypatch):
    ista_conv2d, _, _ = _mods()
    x, w, z0, G, lr, stride, padding = _problem(GEOMS[0])
    fn = lambda a, b, c: ista_conv2d(a, b, c, 0.1, stride=stride, padding=padding, maxiter=6, lr=lr, tol=0.0)  # noqa: E731
    xl, wl, zl = (t.cuda().requires_grad_(True) for t in (x, w, z0))
    z = fn(xl, zl, wl)

    def refuse(*a, **k):
        raise AssertionError("ATen convolution in the backward")
    with monkeypatch.context() as m:
        m.setattr(torch.nn.functional, "conv2d", refuse)
        m.setattr(torch.nn.functional, "conv_transpose2d", refuse)
        m.setattr(torch, "conv2d", refuse)
        (z * G.cuda()).sum().backward()
    first = [t.grad.clone() for t in (xl, wl, zl)]
    _, again = _grads(fn, x, w, z0, G, "cuda")
    for a, b in zip(first, again):
        assert torch.equal(a.cpu(), b)


def test_sgd_on_the_weight_matches_the_oracle():
    """Three SGD steps on W through the solve (learning a filter bank by back-propagating through unrolled
    convolutional sparse coding) -- the same three steps through the oracle."""
    ista_conv2d, _, orc = _mods()
    x, w, z0, _, lr, stride, padding = _problem(GEOMS[2], seed=9)
    z0 = torch.zeros_like(z0)
    F = torch.nn.functional

    def steps(fn, dev):
        wl = w.clone().to(dev).requires_grad_(True)
        xd, zd = x.to(dev), z0.to(dev)
        for _ in range(3):
            z = fn(xd, zd, wl)
            loss = ((F.conv_transpose2d(z, wl, stride=stride, padding=padding) - xd) ** 2).sum()
            wl.grad = None
            loss.backward()
            with torch.no_grad():
                wl -= 1e-3 * wl.grad
        return wl.detach().cpu()
    kw_ = dict(stride=stride, padding=padding, maxiter=8, lr=lr, tol=0.0)
    ref = steps(lambda a, b, c: orc.conv_fista(a, b, c, 0.1, **kw_), "cpu")
    got = steps(lambda a, b, c: ista_conv2d(a, b, c, 0.1, **kw_), "cuda")
    assert ((got - ref).abs().max() / ref.abs().max()).item() <= 1e-4
