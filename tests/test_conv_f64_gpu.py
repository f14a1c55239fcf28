"""float64 tensors on the convolutional path (csrc/conv_f64.hip): ista_conv2d, its gradients, conv_loss and
lip_bound_conv2d in IEEE double against the CPU oracle in double (oracle.lasso_oracle.conv_fista / conv_objective and
torch.autograd through them).

Bars: codes 9.3e-14 = 5e-5 * 2^-29, the project's float64 bar; gradients 3.7e-13 = 2e-4 * 2^-29 of each
gradient's max magnitude (the fp32 test's bar scaled the same way).  Every comparison records the deviation it measured
next to its bar (tests/margins.py, "conv_f64/...")."""
import ctypes as C
import math

import pytest
import torch

from margins import record_margins

pytestmark = pytest.mark.gpu

Z_BAR = 5e-5 * 2.0 ** -29          # 9.3e-14
G_RTOL = 2e-4 * 2.0 ** -29         # 3.7e-13
F64 = torch.float64
ALPHA = 0.1

# (N, C, K, kh, kw, stride, padding, Hz, Wz)
GEOMS = [
    (3, 1, 100, 3, 3, 1, 1, 9, 9),                    # M = 243: a ragged last row block; two atom blocks
    (3, 2, 48, 3, 3, 1, 1, 40, 24),                   # many row blocks
    (3, 8, 32, 3, 3, 1, 1, 12, 12),
    (3, 2, 24, 7, 7, 1, 3, 12, 11),                   # 98 taps
    (3, 2, 12, 3, 3, 2, 1, 6, 7),                     # stride 2
    (2, 3, 20, 3, 5, (1, 2), (1, 2), 5, 6),           # stride (1, 2), asymmetric padding, 3 x 5 kernel
    (2, 17, 8, 3, 3, 1, 1, 6, 6),                     # 153 taps
]
IDS = ["g%d-C%d-K%d" % (i + 1, g[1], g[2]) for i, g in enumerate(GEOMS)]
RUNS = [(fast, T) for fast in (True, False) for T in (1, 6, 30)]


def _mods():
    from lasso_amd import _native as nat
    from lasso_amd.conv2d import ista_conv2d, lip_bound_conv2d
    from lasso_amd.conv2d.ista import conv_loss
    from oracle import lasso_oracle as orc
    return ista_conv2d, conv_loss, lip_bound_conv2d, nat, orc


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _sizes(geom):
    N, Cc, K, kh, kw, stride, padding, Hz, Wz = geom
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    return (N, Cc, (Hz - 1) * sh - 2 * ph + kh, (Wz - 1) * sw - 2 * pw + kw, K, Hz, Wz, kh, kw, sh, sw, ph, pw)


def _problem(geom, seed=0):
    """_problem of tests/test_conv_autograd_gpu.py with its draws converted to double"""
    N, Cc, K, kh, kw, stride, padding, Hz, Wz = geom
    _, _, H, W = _sizes(geom)[:4]
    g = torch.Generator().manual_seed(seed + 7 * K + Hz)
    w = (torch.randn(K, Cc, kh, kw, generator=g) / (Cc * kh * kw) ** 0.5).double()
    x = torch.randn(N, Cc, H, W, generator=g).double()
    z0 = (torch.randn(N, K, Hz, Wz, generator=g) * 0.05).double()
    G = torch.randn(N, K, Hz, Wz, generator=g).double()
    lr = 0.3 / max(w.pow(2).sum().item(), 1e-3)
    return x, w, z0, G, lr, stride, padding


def _grads(fn, x, w, z0, G, dev, need=(True, True, True)):
    xl = x.detach().clone().to(dev).requires_grad_(need[0])
    wl = w.detach().clone().to(dev).requires_grad_(need[1])
    zl = z0.detach().clone().to(dev).requires_grad_(need[2])
    z = fn(xl, zl, wl)
    (z * G.to(dev)).sum().backward()
    return z.detach(), [t.grad for t in (xl, wl, zl)]


_REF = {}


def _reference(gi, fast, T):
    """the oracle's codes and gradients of (z G).sum() in double, computed once and shared by the tests"""
    key = (gi, fast, T)
    if key not in _REF:
        orc = _mods()[4]
        x, w, z0, G, lr, stride, padding = _problem(GEOMS[gi])
        kw_ = dict(stride=stride, padding=padding, fast=fast, maxiter=T, lr=lr, tol=0.0)
        _REF[key] = _grads(lambda a, b, c: orc.conv_fista(a, b, c, ALPHA, **kw_), x, w, z0, G, "cpu")
    return _REF[key]


def _grad_gaps(got, ref):
    """{name: (max |difference|, bar)} of gradients against the reference's"""
    out = {}
    for name, a, b in zip(("dx", "dW", "dz0"), got, ref):
        if b is None:
            assert a is None, name
            continue
        assert a is not None and a.dtype == F64 and a.shape == b.shape, name
        out[name] = ((a.cpu() - b).abs().max().item(), G_RTOL * max(b.abs().max().item(), 1e-3))
    return out


@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=IDS)
def test_codes_match_the_oracle(gi):
    ista_conv2d = _mods()[0]
    x, w, z0, _, lr, stride, padding = _problem(GEOMS[gi])
    xg, wg, zg = x.cuda(), w.cuda(), z0.cuda()
    keep = [t.clone() for t in (xg, wg, zg)]
    worst, zmax = 0.0, 0.0
    for fast, T in RUNS:
        z = ista_conv2d(xg, zg, wg, ALPHA, stride=stride, padding=padding, fast=fast, maxiter=T, lr=lr, tol=0.0)
        assert z.dtype == F64 and z.is_cuda and z.shape == z0.shape
        zr = _reference(gi, fast, T)[0]
        err = (z.cpu() - zr).abs().max().item()
        print("codes %s fast=%s T=%d: max|dz| = %.3g (bar %.3g), max|z| = %.3g" % (IDS[gi], fast, T, err, Z_BAR,
                                                                                    zr.abs().max().item()))
        worst, zmax = max(worst, err), max(zmax, zr.abs().max().item())
    record_margins("conv_f64/codes/" + IDS[gi], dict(max_abs_dz=worst, bar=Z_BAR, max_abs_z=zmax))
    assert worst <= Z_BAR
    for a, b in zip(keep, (xg, wg, zg)):
        assert torch.equal(a, b)                       # no input is modified


@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=IDS)
def test_gradients_match_autograd_through_the_oracle(gi):
    ista_conv2d = _mods()[0]
    x, w, z0, G, lr, stride, padding = _problem(GEOMS[gi])
    worst = {}
    for fast, T in RUNS:
        kw_ = dict(stride=stride, padding=padding, fast=fast, maxiter=T, lr=lr, tol=0.0)
        zg, got = _grads(lambda a, b, c: ista_conv2d(a, b, c, ALPHA, **kw_), x, w, z0, G, "cuda")
        zr, ref = _reference(gi, fast, T)
        assert all(t.is_cuda for t in got)
        assert (zg.cpu() - zr).abs().max().item() <= Z_BAR
        for name, (err, bar) in _grad_gaps(got, ref).items():
            print("gradient %s fast=%s T=%d %s: %.3g (bar %.3g)" % (IDS[gi], fast, T, name, err, bar))
            worst[name] = max(worst.get(name, 0.0), err / bar)
    record_margins("conv_f64/gradients/" + IDS[gi], dict(worst_fraction_of_bar=worst, rtol=G_RTOL))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_partial_requires_grad_and_cpu_leaves():
    ista_conv2d, _, _, _, orc = _mods()
    x, w, z0, G, lr, stride, padding = _problem(GEOMS[3], seed=2)
    kw_ = dict(stride=stride, padding=padding, maxiter=4, lr=lr, tol=0.0)
    worst = 0.0
    # each of the three alone; (True, False, False) and (False, False, True) run with a null grad_w
    for need in ((False, True, False), (True, False, False), (False, False, True)):
        _, ref = _grads(lambda a, b, c: orc.conv_fista(a, b, c, ALPHA, **kw_), x, w, z0, G, "cpu", need)
        _, got = _grads(lambda a, b, c: ista_conv2d(a, b, c, ALPHA, **kw_), x, w, z0, G, "cuda", need)
        for name, (err, bar) in _grad_gaps(got, ref).items():
            worst = max(worst, err / bar)
    # CPU leaves: staged through the device, z and the gradients arrive on the CPU in double
    _, ref = _grads(lambda a, b, c: orc.conv_fista(a, b, c, ALPHA, **kw_), x, w, z0, G, "cpu")
    zc, got = _grads(lambda a, b, c: ista_conv2d(a, b, c, ALPHA, **kw_), x, w, z0, G, "cpu")
    assert zc.device.type == "cpu" and zc.dtype == F64
    assert all(t.device.type == "cpu" and t.dtype == F64 for t in got)
    for name, (err, bar) in _grad_gaps(got, ref).items():
        worst = max(worst, err / bar)
    record_margins("conv_f64/gradients/partial_and_cpu", dict(worst_fraction_of_bar=worst, rtol=G_RTOL))
    assert worst <= 1.0


# (N, C, K, kh, kw, stride, padding, Hz, Wz): 237, 308 and 207 input elements
TINY = [(2, 1, 5, 3, 3, 1, 1, 4, 4), (2, 2, 4, 3, 3, 2, 1, 3, 4), (1, 3, 3, 3, 5, (1, 2), (1, 2), 3, 3)]


@pytest.mark.parametrize("ti", range(len(TINY)))
@pytest.mark.parametrize("T", [1, 4])
def test_gradcheck(ti, T):
    ista_conv2d, _, _, _, orc = _mods()
    N, Cc, K, kh, kw, stride, padding, Hz, Wz = TINY[ti]
    H, W = _sizes(TINY[ti])[2:4]
    g = torch.Generator().manual_seed(0)
    w = torch.randn(K, Cc, kh, kw, generator=g, dtype=F64) / math.sqrt(Cc * kh * kw)
    x = torch.randn(N, Cc, H, W, generator=g, dtype=F64)
    z0 = 0.05 * torch.randn(N, K, Hz, Wz, generator=g, dtype=F64)
    lr = 0.3 / w.pow(2).sum().item()
    assert x.numel() + w.numel() + z0.numel() == (237, 308, 207)[ti]
    kw_ = dict(stride=stride, padding=padding, fast=True, maxiter=T, lr=lr, tol=0.0)
    settings = dict(eps=1e-6, atol=1e-7, rtol=1e-5)
    # the oracle passes: no soft-threshold kink lies within the probe
    leaves = [t.clone().requires_grad_(True) for t in (x, z0, w)]
    assert torch.autograd.gradcheck(lambda a, b, c: orc.conv_fista(a, b, c, ALPHA, **kw_), leaves, **settings)
    leaves = [t.cuda().requires_grad_(True) for t in (x, z0, w)]
    assert torch.autograd.gradcheck(lambda a, b, c: ista_conv2d(a, b, c, ALPHA, **kw_), leaves, **settings)


# (geometry, fast, the iteration the oracle stops at).  The budget is sqrt(d11 d12) of the oracle's sums.  FISTA's sums
# are not monotone: on geometry 5 they rise from d2 to d8 and d1 .. d5 lie below that budget, so the oracle stops
# there at iteration 1, not 12 (d = 25.9 23.6 27.9 31.1 33.5 35.0 35.9 36.2 36.1 35.6 34.8 33.9).  The stop at 12 inside a
# speculated chunk with momentum is therefore taken on geometry 4, whose FISTA sums fall from d4 on, geometry 5 stops
# at 12 without momentum, and its FISTA run must stop where the oracle does.
STOPS = [(3, True, 12), (4, False, 12), (4, True, 1)]


@pytest.mark.parametrize("gi,fast,stop_at", STOPS, ids=["g4-fista", "g5-ista", "g5-fista"])
def test_stop_rule(gi, fast, stop_at):
    ista_conv2d, _, _, _, orc = _mods()
    x, w, z0, _, lr, stride, padding = _problem(GEOMS[gi])
    kw_ = dict(stride=stride, padding=padding, lr=lr, fast=fast, return_info=True)
    d = [orc.conv_fista(x, z0, w, ALPHA, maxiter=i, tol=0.0, **kw_)[1]["last_delta"] for i in range(1, 13)]
    budget = math.sqrt(d[10] * d[11])
    tol = budget / z0.numel()
    zr, info_r = orc.conv_fista(x, z0, w, ALPHA, maxiter=200, tol=tol, **kw_)
    assert info_r["iterations"] == stop_at, (info_r, d)
    assert all(abs(di / (z0.numel() * tol) - 1.0) >= 0.01 for di in d), d          # every sum 1 % away from the budget
    xg, wg, zg = x.cuda(), w.cuda(), z0.cuda()
    z, info = ista_conv2d(xg, zg, wg, ALPHA, maxiter=200, tol=tol, **kw_)
    err = (z.cpu() - zr).abs().max().item()
    rel = abs(info["last_delta"] - info_r["last_delta"]) / info_r["last_delta"]
    print("stop rule %s fast=%s: iterations %d, last_delta rel %.3g, max|dz| %.3g" % (IDS[gi], fast, info["iterations"],
                                                                                      rel, err))
    record_margins("conv_f64/stop_rule/%s-%s" % (IDS[gi], "fista" if fast else "ista"),
                   dict(iterations=info["iterations"], last_delta_rel=rel, last_delta_rtol=1e-12, max_abs_dz=err, bar=Z_BAR))
    assert info["iterations"] == stop_at
    assert isinstance(info["last_delta"], float) and rel <= 1e-12
    assert err <= Z_BAR
    # with grad enabled: bitwise the z, the count and the delta of the call without grad
    zq, info_q = ista_conv2d(xg, zg, wg.clone().requires_grad_(True), ALPHA, maxiter=200, tol=tol, **kw_)
    assert zq.grad_fn is not None and z.grad_fn is None
    assert torch.equal(zq.detach(), z)
    assert info_q["iterations"] == stop_at and info_q["last_delta"] == info["last_delta"]


def _bound_in_double(kernel, padding, sample=50, sqrt=False):
    """lip_const.py:96-135 restated in double, the grid 2 pi i / (sample - 1) in double"""
    ks = kernel.size(-1)
    if kernel.size(0) > kernel.size(1):
        kernel = kernel.transpose(0, 1)
    freq = 2 * math.pi * torch.arange(sample, dtype=F64) / (sample - 1)
    f0, f1 = torch.meshgrid(freq, freq, indexing="ij")
    pos = 1.0 + torch.arange(padding - ks, padding, dtype=F64)
    h0, h1 = torch.meshgrid(pos, pos, indexing="ij")
    phase = (f0.reshape(-1, 1) * h0.reshape(1, -1) + f1.reshape(-1, 1) * h1.reshape(1, -1)).T
    taps = kernel.flatten(2)
    re, im = torch.matmul(taps, torch.cos(phase)), torch.matmul(taps, torch.sin(phase))
    bound = (re.square().sum(1) + im.square().sum(1)).max(-1)[0].sum()
    return bound.sqrt() if sqrt else bound


@pytest.mark.parametrize("shape,padding", [((6, 2, 3, 3), 1), ((5, 9, 5, 5), 2), ((40, 3, 7, 7), 0)],
                         ids=["6x2x3x3", "5x9x5x5", "40x3x7x7"])
def test_bound(shape, padding):
    _, _, lip_bound_conv2d, _, _ = _mods()
    g = torch.Generator().manual_seed(3)
    k = torch.randn(*shape, generator=g, dtype=F64) / math.sqrt(shape[1] * shape[2] * shape[3])
    gaps = {}
    for sqrt in (False, True):
        got = lip_bound_conv2d(k.cuda(), padding, sqrt=sqrt)
        assert got.dtype == F64 and got.dim() == 0 and got.is_cuda
        ref = _bound_in_double(k, padding, sqrt=sqrt).item()
        f32 = lip_bound_conv2d(k.float().cuda(), padding, sqrt=sqrt)
        assert f32.dtype == torch.float32
        gaps["sqrt" if sqrt else "plain"] = dict(rel_to_double=abs(got.item() - ref) / ref, rtol=1e-12,
                                                 rel_to_fp32=abs(got.item() - f32.item()) / ref, rtol_fp32=1e-5)
    print("bound", shape, gaps)
    record_margins("conv_f64/bound/%dx%dx%dx%d" % shape, gaps)
    for v in gaps.values():
        assert v["rel_to_double"] <= 1e-12 and v["rel_to_fp32"] <= 1e-5
    on_cpu = lip_bound_conv2d(k, padding)                    # a CPU kernel: staged, the result comes back on the CPU
    assert on_cpu.device.type == "cpu" and on_cpu.dtype == F64
    assert on_cpu.item() == lip_bound_conv2d(k.cuda(), padding).item()


def test_objective_and_auto_lr():
    ista_conv2d, conv_loss, lip_bound_conv2d, _, orc = _mods()
    worst = 0.0
    for gi in (0, 4, 5):
        x, w, z0, G, lr, stride, padding = _problem(GEOMS[gi])
        for z in (z0, G):
            got = conv_loss(x.cuda(), z.cuda(), w.cuda(), ALPHA, stride=stride, padding=padding)
            assert got.dtype == F64 and got.dim() == 0 and got.is_cuda
            ref = orc.conv_objective(x, z, w, ALPHA, stride=stride, padding=padding).item()
            worst = max(worst, abs(got.item() - ref) / abs(ref))
    print("objective: rel %.3g" % worst)
    record_margins("conv_f64/objective", dict(rel=worst, rtol=1e-14))
    assert worst <= 1e-14
    # lr='auto' is 1 / the double bound, bitwise
    x, w, z0, _, _, _, _ = _problem((2, 1, 8, 5, 5, 1, 2, 10, 10), seed=4)
    xg, wg, zg = x.cuda(), w.cuda(), z0.cuda()
    bound = lip_bound_conv2d(wg, 2).item()
    auto = ista_conv2d(xg, zg, wg, 0.2, padding=2, maxiter=5, lr='auto', tol=0.0)
    explicit = ista_conv2d(xg, zg, wg, 0.2, padding=2, maxiter=5, lr=1.0 / bound, tol=0.0)
    assert torch.equal(auto, explicit)
    zr = orc.conv_fista(x, z0, w, 0.2, padding=2, maxiter=5, lr=1.0 / bound, tol=0.0)
    assert (auto.cpu() - zr).abs().max().item() <= Z_BAR
    with pytest.raises(NotImplementedError):
        ista_conv2d(xg, zg, wg, 0.2, stride=2, padding=2, maxiter=5, lr='auto')


def test_edges():
    ista_conv2d, conv_loss, _, _, _ = _mods()
    x, w, z0, G, lr, stride, padding = _problem(GEOMS[0])
    xg, wg, zg = x.cuda(), w.cuda(), z0.cuda()
    kw_ = dict(stride=stride, padding=padding, lr=lr, tol=0.0)
    # N = 0: a clone
    xe, ze = xg[:0], zg[:0]
    out = ista_conv2d(xe, ze, wg, ALPHA, maxiter=5, **kw_)
    assert out.shape == ze.shape and out.dtype == F64 and out.is_cuda and out is not ze
    xl, zl, wl = (t.clone().requires_grad_(True) for t in (xe, ze, wg))
    ista_conv2d(xl, zl, wl, ALPHA, maxiter=5, **kw_).sum().backward()
    assert xl.grad.shape == xe.shape and zl.grad.shape == ze.shape
    assert wl.grad.dtype == F64 and torch.equal(wl.grad, torch.zeros_like(wg))
    # maxiter = 0: z0 itself
    assert ista_conv2d(xg, zg, wg, ALPHA, maxiter=0, **kw_) is zg
    # two identical calls, two identical backward passes
    fn = lambda a, b, c: ista_conv2d(a, b, c, ALPHA, maxiter=6, **kw_)  # noqa: E731
    z1, g1 = _grads(fn, x, w, z0, G, "cuda")
    z2, g2 = _grads(fn, x, w, z0, G, "cuda")
    assert torch.equal(z1, z2)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    assert torch.equal(ista_conv2d(xg, zg, wg, ALPHA, maxiter=6, **kw_), z1)
    # mixed dtypes: refused, nothing written
    keep = zg.clone()
    for args in ((xg.float(), zg, wg), (xg, zg.float(), wg), (xg, zg, wg.float()), (xg.half(), zg.half(), wg.half())):
        with pytest.raises(NotImplementedError, match="float32 and for float64"):
            ista_conv2d(*args, ALPHA, maxiter=3, **kw_)
    with pytest.raises(NotImplementedError, match="float32 and for float64"):
        conv_loss(xg, zg.float(), wg, ALPHA, stride=stride, padding=padding)
    assert torch.equal(zg, keep)
    # fp32, float64, fp32 on the same engine and stream: the fp32 results are bitwise equal
    xf, zf, wf = xg.float(), zg.float(), wg.float()
    first = ista_conv2d(xf, zf, wf, ALPHA, maxiter=6, **kw_)
    ista_conv2d(xg, zg, wg, ALPHA, maxiter=6, **kw_)
    again = ista_conv2d(xf, zf, wf, ALPHA, maxiter=6, **kw_)
    assert first.dtype == torch.float32 and torch.equal(first, again)


def test_verbose_prints_the_double_objective(capsys):
    ista_conv2d, conv_loss, _, _, _ = _mods()
    x, w, z0, _, lr, stride, padding = _problem(GEOMS[4])
    xg, wg, zg = x.cuda(), w.cuda(), z0.cuda()
    kw_ = dict(stride=stride, padding=padding, lr=lr, tol=0.0, maxiter=3)
    z = ista_conv2d(xg, zg, wg, ALPHA, verbose=True, **kw_)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 3 and lines[0] == 'loss: %0.4f' % conv_loss(xg, zg, wg, ALPHA, stride, padding).item()
    assert torch.equal(z, ista_conv2d(xg, zg, wg, ALPHA, **kw_))


def test_c_abi():
    _, _, _, nat, _ = _mods()
    L = nat.lib()
    geom = GEOMS[4]
    x, w, z0, _, lr, _, _ = _problem(geom)
    xg, wg, zg = x.cuda(), w.cuda(), z0.cuda()
    sizes = _sizes(geom)
    need = L.lasso_conv_ista_workspace_bytes_f64(*sizes)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = nat.stream_ptr(xg.device)
    # a budget between the sums of iterations 11 and 12, so that the solve reports a last sum
    probe, dl = C.c_int32(0), C.c_double(0.0)
    out = torch.empty_like(zg)
    assert L.lasso_conv_ista_solve_f64(nat.ptr(xg), nat.ptr(wg), nat.ptr(zg), nat.ptr(out), *sizes, ALPHA, lr, 1, 12, 1e-300,
                                       C.byref(probe), C.byref(dl), nat.ptr(ws), need, st) == nat.LASSO_OK
    assert probe.value == 12 and dl.value > 0.0
    tol = dl.value * 1.01 / zg.numel()
    z64, z32 = torch.empty_like(zg), torch.empty_like(zg)
    it64, it32, d64, d32 = C.c_int32(0), C.c_int32(0), C.c_double(0.0), C.c_float(0.0)
    assert L.lasso_conv_ista_solve_f64(nat.ptr(xg), nat.ptr(wg), nat.ptr(zg), nat.ptr(z64), *sizes, ALPHA, lr, 1, 100, tol,
                                       C.byref(it64), C.byref(d64), nat.ptr(ws), need, st) == nat.LASSO_OK
    assert L.lasso_conv_ista_solve(nat.ptr(xg), nat.ptr(wg), nat.ptr(zg), nat.ptr(z32), *sizes, nat.LASSO_F64, ALPHA, lr, 1,
                                   100, tol, C.byref(it32), C.byref(d32), nat.ptr(ws), need, st) == nat.LASSO_OK
    torch.cuda.synchronize()
    assert torch.equal(z64, z32) and it64.value == it32.value <= 12
    assert d32.value == C.c_float(d64.value).value                       # the double rounded once
    # the objective: the float slot holds the double rounded once
    l64 = torch.zeros((), dtype=F64, device="cuda")
    l32 = torch.zeros((), dtype=torch.float32, device="cuda")
    assert L.lasso_conv_objective_f64(nat.ptr(xg), nat.ptr(wg), nat.ptr(z64), *sizes, ALPHA, nat.ptr(l64), nat.ptr(ws), need,
                                      st) == nat.LASSO_OK
    assert L.lasso_conv_objective(nat.ptr(xg), nat.ptr(wg), nat.ptr(z64), *sizes, nat.LASSO_F64, ALPHA, nat.ptr(l32),
                                  nat.ptr(ws), need, st) == nat.LASSO_OK
    assert l32.item() == C.c_float(l64.item()).value
    # a workspace one byte short: refused, z_out untouched
    mark = torch.full_like(zg, 7.0)
    assert L.lasso_conv_ista_solve_f64(nat.ptr(xg), nat.ptr(wg), nat.ptr(zg), nat.ptr(mark), *sizes, ALPHA, lr, 1, 5, 0.0,
                                       None, None, nat.ptr(ws), need - 1, st) == nat.LASSO_ERR_WORKSPACE
    assert L.lasso_conv_ista_solve(nat.ptr(xg), nat.ptr(wg), nat.ptr(zg), nat.ptr(mark), *sizes, nat.LASSO_F64, ALPHA, lr, 1,
                                   5, 0.0, None, None, nat.ptr(ws), need - 1, st) == nat.LASSO_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(mark, torch.full_like(zg, 7.0))
