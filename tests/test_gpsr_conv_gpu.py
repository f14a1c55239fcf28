"""Convolutional GPSR-Basic on the HIP path (csrc/conv_gpsr.hip) against the goldens recorded from the reference
and, for shapes that have none, against the host model (tests/gpsr_conv_model.py).

Bars: the project's GPSR rule (gpsr_conv_cases.z_bar) -- 4 x the gap between the model in float32 and in float64,
never tighter than the floors 5e-5 on z, 1e-5 relative on lambda, 1e-6 relative on the objective.  Counts (iterations,
trial lists) and warnings are exact.  Measured gaps and achieved deviations go to parity_margins.json through
tests/margins.py."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpsr_conv_cases import CASES, case_inputs, conv_inputs, load_case, max_rel, rows_of, z_bar
from margins import record_margins
from recipes import recipe_xw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(golden):
    return golden("gpsr_conv_cases")


def hip(x, w, tau, z0=None, **kw):
    from lasso_amd.conv2d import gpsr_conv2d
    return gpsr_conv2d(x.cuda(), w.cuda(), tau, z0=None if z0 is None else z0.cuda(), return_info=True, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case(cases, name):
    spec, gold = CASES[name], load_case(cases, name)
    x, w, z0 = case_inputs(spec)
    geo = dict(stride=spec["stride"], padding=spec["padding"])
    bars, gaps, _, _ = z_bar(x, w, spec["tau"], z0=z0, **geo, **spec["kwargs"])
    xg, wg, z0g = x.cuda(), w.cuda(), None if z0 is None else z0.cuda()
    keep = xg.clone(), wg.clone(), None if z0 is None else z0g.clone()
    from lasso_amd.conv2d import gpsr_conv2d
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        z, info = gpsr_conv2d(xg, wg, spec["tau"], z0=z0g, return_info=True, **geo, **spec["kwargs"])
    assert z.is_cuda and z.dtype == torch.float32 and z.shape == F.conv2d(x, w, **geo).shape
    n_main = int(gold["n_iter"])
    assert info["iterations"] == n_main + int(gold["db_iters"])
    assert list(info["trials"]) == list(gold["trials"])
    assert len(info["criterion"]) == n_main
    assert sorted(str(c.message) for c in caught) == sorted(m for m in str(gold["warnings"]).split("\n") if m)
    assert torch.equal(xg, keep[0]) and torch.equal(wg, keep[1]) and (z0 is None or torch.equal(z0g, keep[2]))
    rows = gold["z_rows"]
    dev = dict(z=float(np.abs(rows_of(z.cpu()).numpy()[rows] - gold["z"]).max()),
               lam=max_rel(info["accepted_lambda"], gold["lam"]), obj=max_rel(info["objective"], gold["objective"]))
    print(name, "gaps", gaps, "bars", bars, "hip", dev)
    record_margins("conv_gpsr/golden/" + name, dict(model_f32_f64_gap=gaps, bar=bars, hip=dev, form=info["form"]))
    for key in ("z", "lam", "obj"):
        assert dev[key] <= bars[key], (name, key, dev[key], bars[key])
    assert abs(float(z.double().abs().sum()) - float(gold["z_abssum"])) <= bars["z"] * max(1, int(gold["z_nnz"]))
    if name == "zero":
        assert not z.any()


def against_model(tag, x, w, tau, z0=None, solve=None, model=None, **kw):
    """solve: hip (the Python entry point) or a function of its arguments; model: z_bar's tuple, where it is shared"""
    bars, gaps, z_m, info_m = model or z_bar(x, w, tau, z0=z0, **kw)
    for fn, bound, f in info_m["decisions"]:          # the model's branches are not within rounding of flipping
        assert abs(fn - bound) >= 1e-4 * abs(f), (tag, fn, bound, f)
    z, info = (solve or hip)(x, w, tau, z0=z0, **kw)
    assert info["iterations"] == info_m["iterations"], tag
    assert info["trials"] == info_m["trials"], tag
    dev = dict(z=float((z.cpu() - z_m).abs().max()), lam=max_rel(info["accepted_lambda"], info_m["accepted_lambda"]),
               obj=max_rel(info["objective"], info_m["objective"]))
    print(tag, "gaps", gaps, "bars", bars, "hip", dev)
    record_margins("conv_gpsr/model/" + tag, dict(model_f32_f64_gap=gaps, bar=bars, hip=dev, form=info["form"]))
    for key in ("z", "lam", "obj"):
        assert dev[key] <= bars[key], (tag, key, dev[key], bars[key])
    assert (np.diff(np.array(info["objective"])) <= 0).all(), tag      # non-increasing over the accepted iterations
    assert z.shape == z_m.shape
    return z, info


# N, C, H, W, K, ks, stride, padding: the smallest shapes at which the kernels can go wrong
FRESH = {
    "N1": (1, 2, 9, 10, 6, 3, 1, 1),
    "K1": (2, 2, 9, 11, 1, 3, 1, 0),
    "K33": (2, 2, 9, 11, 33, 3, 1, 1),                      # atoms: not a multiple of a tile
    "K130": (2, 3, 10, 13, 130, 3, 1, 1),                   # more than one 64- / 128-atom tile
    "C1_ks1": (3, 1, 9, 7, 8, 1, 1, 0),                     # one tap
    "Hz1": (5, 2, 7, 7, 40, 7, 1, 0),                       # the kernel covers the image: one code pixel per image
    "ragged_M": (3, 2, 11, 14, 10, 3, 1, 0),                # M = 3 * 9 * 12 = 324, not a multiple of 64
    "stride2_pad": (2, 2, 13, 15, 10, 5, 2, 1),
    "stride21": (2, 2, 13, 12, 10, 3, (2, 1), (1, 0)),
    "many_blocks": (5, 3, 20, 20, 20, 5, 1, 2),             # M = 2000: several GEMM blocks along the pixels
    # one shape inside each geometry family of the implicit ISTA kernels, a handful of 12 x 12 images
    "gray_c1k7": (3, 1, 12, 12, 64, 7, 1, 3),
    "rgb_c3k5": (3, 3, 12, 12, 128, 5, 1, 2),
    "c16k3": (3, 16, 12, 12, 256, 3, 1, 1),
}


IMPLICIT_FAMILIES = ("gray_c1k7", "rgb_c3k5", "c16k3")


@pytest.mark.parametrize("tag", sorted(FRESH))
def test_fresh_shapes_against_the_model(tag):
    N, Cc, H, W, K, ks, s, p = FRESH[tag]
    x, w = conv_inputs((N, Cc, H, W), K, ks, seed=40 + len(tag) + K, unit_norm=ks * ks * Cc > 1)
    _, info = against_model(tag, x, w, 0.3, stride=s, padding=p, maxiter=5, tol=0.0)
    if tag in IMPLICIT_FAMILIES:
        assert info["form"] == "implicit"
    elif s != 1 or K % 4:                                   # outside the implicit kernels' coverage
        assert info["form"] == "patches"
    else:
        assert info["form"] in ("implicit", "patches")


@pytest.mark.parametrize("tag", IMPLICIT_FAMILIES)
def test_both_forms_agree_on_the_implicit_families(tag, monkeypatch):
    """the implicit form and the forced general form: same counts, each within the z bar of the model, and
    info['form'] says which ran"""
    N, Cc, H, W, K, ks, s, p = FRESH[tag]
    x, w = conv_inputs((N, Cc, H, W), K, ks, seed=40 + len(tag) + K)
    kw = dict(stride=s, padding=p, maxiter=5, tol=0.0)
    bars, gaps, z_m, info_m = z_bar(x, w, 0.3, **kw)
    z_i, info_i = hip(x, w, 0.3, **kw)
    monkeypatch.setenv("LASSO_CONV_GPSR_FORM", "patches")
    z_p, info_p = hip(x, w, 0.3, **kw)
    monkeypatch.delenv("LASSO_CONV_GPSR_FORM")
    assert info_i["form"] == "implicit" and info_p["form"] == "patches"
    assert info_i["iterations"] == info_p["iterations"] == info_m["iterations"]
    assert info_i["trials"] == info_p["trials"] == info_m["trials"]
    dev = dict(implicit=float((z_i.cpu() - z_m).abs().max()), patches=float((z_p.cpu() - z_m).abs().max()),
               between=float((z_i - z_p).abs().max()))
    print(tag, "bar", bars["z"], dev)
    record_margins("conv_gpsr/both_forms/" + tag, dict(bar=bars["z"], model_f32_f64_gap=gaps["z"], hip_max_dz=dev))
    assert max(dev.values()) <= bars["z"], (tag, dev, bars["z"])
    np.testing.assert_allclose(info_i["objective"], info_p["objective"], rtol=bars["obj"])


def test_starts_z0_init0_init2_continuation_and_debias():
    x, w = conv_inputs((3, 2, 13, 11), 18, 3, seed=31)
    geo = dict(stride=1, padding=1)
    against_model("init0", x, w, 0.4, init=0, maxiter=6, tol=0.0, **geo)
    against_model("init2", x, w, 0.4, init=2, maxiter=6, tol=0.0, **geo)
    z0 = 0.1 * torch.randn(3, 18, 13, 11, generator=torch.Generator().manual_seed(5))
    keep = z0.clone()
    against_model("z0", x, w, 0.4, z0=z0, maxiter=6, tol=0.0, **geo)
    assert torch.equal(z0, keep)
    against_model("cont", x, w, 0.4, continuation=True, cont_steps=2, first_tau_factor=2.0, maxiter=4, tol=0.0, **geo)
    z_main, _ = hip(x, w, 0.9, maxiter=6, tol=0.0, **geo)
    z, info = against_model("debias", x, w, 0.9, maxiter=6, tol=0.0, debias=True, maxiter_debias=5, **geo)
    assert info["iterations"] == 6 + 6                                   # the CG ran: 6 steps
    assert 0 < int((z != 0).sum()) <= x.numel()
    assert torch.equal(z != 0, z_main != 0)                             # on the support of the main phase, unchanged
    assert not torch.equal(z, z_main)


def test_init1_draws_on_the_device_and_runs():
    x, w = conv_inputs((2, 2, 9, 9), 6, 3, seed=3)
    torch.manual_seed(7)
    z, info = hip(x, w, 0.3, init=1, maxiter=3, tol=0.0)
    assert info["iterations"] == 3 and torch.isfinite(z).all() and z.shape == (2, 6, 7, 7)


def test_sufficient_decrease_holds_at_every_accepted_step():
    """F <= f + mu g, re-derived in float64 from the HIP iterates themselves (solves of 1, 2, ... iterations)"""
    mu, tau = 0.1, 0.4
    x, w = conv_inputs((3, 2, 11, 12), 10, 3, seed=57)
    x64, w64 = x.double(), w.double()
    A = lambda v: F.conv_transpose2d(v, w64, padding=1)      # noqa: E731
    AT = lambda v: F.conv2d(v, w64, padding=1)               # noqa: E731
    ay = AT(x64)
    zs, infos = [torch.zeros_like(ay)], []
    for m in range(1, 6):
        z, info = hip(x, w, tau, padding=1, maxiter=m, tol=0.0)
        zs.append(z.cpu().double())
        infos.append(info)
    last = infos[-1]
    assert len(last["objective"]) == 5
    for j in range(5):
        assert infos[j]["objective"] == last["objective"][:j + 1]        # a longer solve repeats the shorter one
        assert infos[j]["accepted_lambda"] == last["accepted_lambda"][:j + 1]
        z = zs[j]
        u, v = z.clamp(min=0), (-z).clamp(min=0)
        t = AT(A(z)) - ay
        gu, gv = t + tau, -t + tau
        lam = last["accepted_lambda"][j]
        du, dv = (u - lam * gu).clamp(min=0) - u, (v - lam * gv).clamp(min=0) - v
        g = float((gu * du).sum() + (gv * dv).sum())
        f = float(0.5 * ((x64 - A(z)) ** 2).sum() + tau * z.abs().sum())
        f_next = last["objective"][j]
        assert g < 0
        assert f_next <= f + mu * g + 1e-6 * abs(f), (j, f_next, f, g)
        assert f_next < f


def test_two_identical_calls_are_bitwise_equal_and_inputs_unchanged():
    x, w = conv_inputs((4, 3, 16, 16), 16, 5, seed=5)
    xg, wg = x.cuda(), w.cuda()
    from lasso_amd.conv2d import gpsr_conv2d
    kw = dict(maxiter=6, return_info=True, mu=0.95, lambda_backtrack=0.6)
    a, ia = gpsr_conv2d(xg, wg, 0.4, **kw)
    b, ib = gpsr_conv2d(xg, wg, 0.4, **kw)
    assert torch.equal(a, b) and ia == ib
    assert max(ia["trials"]) > 1                       # the ladder ran
    assert torch.equal(xg.cpu(), x) and torch.equal(wg.cpu(), w)
    assert a.data_ptr() not in (xg.data_ptr(), wg.data_ptr())


def test_cpu_inputs_come_back_on_the_cpu():
    from lasso_amd.conv2d import gpsr_conv2d
    x, w = conv_inputs((2, 2, 10, 10), 8, 3, seed=8)
    z_gpu = gpsr_conv2d(x.cuda(), w.cuda(), 0.3, maxiter=4)
    z_cpu = gpsr_conv2d(x, w, 0.3, maxiter=4)
    assert z_cpu.device.type == "cpu" and torch.equal(z_cpu, z_gpu.cpu())
    z, info = gpsr_conv2d(torch.empty(0, 2, 10, 10, device="cuda"), w.cuda(), 0.3, return_info=True)
    assert z.shape == (0, 8, 8, 8) and info["iterations"] == 0


def test_neighbouring_solvers_are_bitwise_what_they_are_alone():
    """a linear gpsr_basic solve and an ista_conv2d solve, before and after a gpsr_conv2d on the same stream"""
    from lasso_amd.conv2d import gpsr_conv2d, ista_conv2d
    from lasso_amd.linear.solvers import gpsr_basic
    xl, wl = recipe_xw(37, 10, 50, seed=20)
    xl, wl = xl.cuda(), wl.cuda()
    x, w = conv_inputs((3, 1, 14, 14), 16, 5, seed=9)
    xg, wg = x.cuda(), w.cuda()
    z0 = torch.zeros(3, 16, 10, 10, device="cuda")

    def others():
        a, ia = gpsr_basic(xl, wl, 0.4, maxiter=5, tol=0.0, return_info=True)
        b = ista_conv2d(xg, z0, wg, alpha=0.2, maxiter=5, lr=0.05, tol=0.0)
        return a, ia, b
    a1, i1, b1 = others()
    gpsr_conv2d(xg, wg, 0.3, maxiter=4, debias=True, maxiter_debias=3)
    a2, i2, b2 = others()
    assert torch.equal(a1, a2) and i1 == i2 and torch.equal(b1, b2)


def test_c_abi_guards_z0_untouched_and_bad_arg_writes_nothing():
    from lasso_amd import _native as nat
    L = nat.lib()
    x, w = conv_inputs((3, 2, 11, 12), 10, 3, seed=2)
    geom = (3, 2, 11, 12, 10, 11, 12, 3, 3, 1, 1, 1, 1)
    xg, wg = x.cuda(), w.cuda()
    z0 = (0.1 * torch.randn(3, 10, 11, 12, generator=torch.Generator().manual_seed(1))).cuda()
    z0_keep = z0.clone()
    nz, guard = 3 * 10 * 11 * 12, 64
    buf = torch.full((nz + 2 * guard,), 777.0, device="cuda")
    z_out = buf[guard:guard + nz]
    ws = torch.empty(L.lasso_conv_gpsr_workspace_bytes(*geom), dtype=torch.uint8, device="cuda")
    stream = nat.stream_ptr(xg.device)

    def solve(g, stop_criterion=3, reserved=0):
        opt, res = nat.GpsrOptions(), nat.GpsrResult()
        opt.reserved = reserved
        opt.stop_criterion, opt.maxiter, opt.miniter, opt.tol = stop_criterion, 4, 5, 0.0
        opt.mu, opt.lambda_backtrack, opt.first_tau_factor, opt.tol_debias = 0.1, 0.5, -1.0, 1e-4
        st = L.lasso_conv_gpsr_solve(nat.ptr(xg), nat.ptr(wg), nat.ptr(z0), z_out.data_ptr(), *g, nat.LASSO_F32, 0.3,
                                     C.byref(opt), C.byref(res), nat.ptr(ws), ws.numel(), stream)
        torch.cuda.synchronize()
        return st, res
    bad = geom[:5] + (10,) + geom[6:]
    assert solve(bad)[0] == nat.LASSO_ERR_BAD_ARG
    assert solve(geom, stop_criterion=9)[0] == nat.LASSO_ERR_BAD_ARG
    for bad in (2, 4, 0x7f00):                                          # bits 0 and 3 are the defined ones
        for defined in (0, 1, nat.FORCE_BLOCKS_128, 1 | nat.FORCE_BLOCKS_128):
            assert solve(geom, reserved=defined | bad)[0] == nat.LASSO_ERR_BAD_ARG, (defined, bad)
    assert bool((buf == 777.0).all())                                   # nothing was written
    st, res = solve(geom)
    assert st == nat.LASSO_OK and res.n_iter == 4
    assert bool((buf[:guard] == 777.0).all()) and bool((buf[guard + nz:] == 777.0).all())
    assert torch.equal(z0, z0_keep)
    z_py, info = hip(x, w, 0.3, z0=z0_keep.cpu(), padding=1, maxiter=4, tol=0.0)
    assert torch.equal(z_out.view(3, 10, 11, 12), z_py) and abs(info["final_objective"] - res.objective) == 0


def test_verbose_lines_match_the_reference_and_the_model(cases):
    import io
    from contextlib import redirect_stdout
    import gpsr_conv_model
    from gpsr_cases import same_line
    from lasso_amd.conv2d import gpsr_conv2d

    def lines(fn, spec, verbose):
        x, w, z0 = case_inputs(spec)
        out = io.StringIO()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with redirect_stdout(out):
                fn(x, w, z0, dict(stride=spec["stride"], padding=spec["padding"], verbose=verbose, **spec["kwargs"]))
        return out.getvalue().splitlines()

    def ours(x, w, z0, kw):
        gpsr_conv2d(x.cuda(), w.cuda(), spec["tau"], z0=None if z0 is None else z0.cuda(), **kw)

    def models(x, w, z0, kw):
        gpsr_conv_model.gpsr_conv2d(x, w, spec["tau"], z0=z0, **kw)
    spec = CASES["gray7"]                                   # the reference's own verbose=2 prints, recorded
    theirs = str(load_case(cases, "gray7")["stdout"]).splitlines()
    mine = lines(ours, spec, 2)
    assert len(theirs) > 30 and len(mine) == len(theirs), (len(mine), len(theirs))
    for a, b in zip(mine, theirs):
        assert same_line(a, b), (a, b)
    for name, verbose in (("search", 2), ("debias", 1), ("debias", 2), ("cont", 2)):
        spec = CASES[name]
        l1, l2 = lines(ours, spec, verbose), lines(models, spec, verbose)
        assert len(l1) == len(l2) and len(l1) > 10, (name, verbose, len(l1), len(l2))
        assert any("Iter =" in a for a in l1) == (name == "debias")
        for a, b in zip(l1, l2):
            assert same_line(a, b), (name, a, b)


# ---- the "patches" form on 128 x 128 GEMM blocks, forced (LASSO_FORCE_BLOCKS_128) -------------------------------------------
# block_side() takes 128-blocks only from 2 x CUs blocks on, far above any geometry here.  Bit 0 | bit 3 of reserved:
# the general form with both of its products -- [M, K] over the patch matrix (the epilogue modes of DESIGN 3.8) and the
# transposed STORE into COLSt [C kh kw, M] -- on Tile<128, 128>.  K130 has M = 260, K = 130, C kh kw = 27: ragged last
# blocks in both.
def abi_solve(x, w, tau, z0=None, reserved=0, stride=1, padding=0, stop_criterion=3, tol=1e-2, maxiter=1000, miniter=5,
              init=0, continuation=False, debias=False, **kwargs):
    """lasso_conv_gpsr_solve directly (`reserved` bits other than bit 0 are not reachable from Python), z between guard
    bands; the request and the report are the Python entry point's own -> (z on the CPU, info)"""
    from lasso_amd import _native as nat
    from lasso_amd.conv2d import gpsr as py
    opt = dict(py._KW_DEFAULTS, **kwargs)
    (sh, sw), (ph, pw) = py._pair(stride), py._pair(padding)
    (N, Cin, H, W), (K, _, kh, kw) = x.shape, w.shape
    Hz, Wz = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    geom = (N, Cin, H, W, K, Hz, Wz, kh, kw, sh, sw, ph, pw)
    xg, wg, z0g = x.cuda(), w.cuda(), None if z0 is None else z0.cuda()
    nz, guard = N * K * Hz * Wz, 64
    buf = torch.full((nz + 2 * guard,), 777.0, device="cuda")
    options, res, keep = py._request(stop_criterion, tol, maxiter, miniter, init, continuation, debias, opt, z0 is not None)
    options.reserved = reserved
    L = nat.lib()
    form = L.lasso_conv_gpsr_form(*geom, reserved).decode()
    ws = torch.empty(L.lasso_conv_gpsr_workspace_bytes(*geom), dtype=torch.uint8, device="cuda")
    nat.check(L.lasso_conv_gpsr_solve(nat.ptr(xg), nat.ptr(wg), nat.ptr(z0g), buf[guard:].data_ptr(), *geom, nat.LASSO_F32,
                                      float(tau), C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(),
                                      nat.stream_ptr(xg.device)))
    torch.cuda.synchronize()
    assert bool((buf[:guard] == 777.0).all()) and bool((buf[guard + nz:] == 777.0).all())
    assert torch.equal(xg.cpu(), x) and torch.equal(wg.cpu(), w) and res.flags == 0
    info = py._report(res, keep, stop_criterion, tol, debias, opt, 0)
    info["form"] = form
    return buf[guard:guard + nz].view(N, K, Hz, Wz).cpu(), info


F128 = ("K33", "K130", "stride2_pad")


@pytest.mark.parametrize("tag", F128)
def test_forced_128_blocks_patches_form_against_the_model(tag):
    from lasso_amd import _native as nat
    assert nat.FORCE_BLOCKS_128 == 8
    reserved = 1 | nat.FORCE_BLOCKS_128
    N, Cc, H, W, K, ks, s, p = FRESH[tag]
    x, w = conv_inputs((N, Cc, H, W), K, ks, seed=40 + len(tag) + K, unit_norm=ks * ks * Cc > 1)
    kw = dict(stride=s, padding=p, maxiter=5, tol=0.0)
    solve = lambda x, w, tau, z0=None, **kw: abi_solve(x, w, tau, z0=z0, reserved=reserved, **kw)      # noqa: E731
    z, info = against_model(tag + "_f128", x, w, 0.3, solve=solve, **kw)
    assert info["form"] == "patches"
    again, info2 = abi_solve(x, w, 0.3, reserved=reserved, **kw)
    assert torch.equal(z, again) and info == info2     # two forced solves are bitwise equal
    if tag == "K130":
        M, ckk = z.shape[0] * z.shape[2] * z.shape[3], Cc * ks * ks
        assert (M, K, ckk) == (260, 130, 27)
        z64, info64 = abi_solve(x, w, 0.3, reserved=1, **kw)
        print("K130: forced 128-blocks bitwise the 64-block solve:", torch.equal(z, z64),
              "max|dz| %.3g" % float((z - z64).abs().max()))


def test_forced_128_blocks_a_ladder_of_trials_continuation_and_debias():
    """rungs (blockIdx.z, a_stride) decided on 128-blocks, the continuation's steps and the debias CG: K130's geometry"""
    reserved = 9
    N, Cc, H, W, K, ks, s, p = FRESH["K130"]
    x, w = conv_inputs((N, Cc, H, W), K, ks, seed=40 + 4 + K)
    geo = dict(stride=s, padding=p)
    solve = lambda x, w, tau, z0=None, **kw: abi_solve(x, w, tau, z0=z0, reserved=reserved, **kw)      # noqa: E731
    kw = dict(maxiter=6, tol=0.0, mu=0.95, lambda_backtrack=0.6, **geo)
    model = z_bar(x, w, 0.4, **kw)
    assert max(model[3]["trials"]) > 1                 # the ladder runs
    against_model("K130_ladder_f128", x, w, 0.4, solve=solve, model=model, **kw)
    against_model("K130_cont_f128", x, w, 0.4, solve=solve, continuation=True, cont_steps=2, first_tau_factor=2.0, maxiter=4,
                  tol=0.0, **geo)
    z, info = against_model("K130_debias_f128", x, w, 1.5, solve=solve, maxiter=6, tol=0.0, debias=True, maxiter_debias=5, **geo)
    assert info["iterations"] == 6 + 6 and 0 < int((z != 0).sum()) <= x.numel()      # the CG ran: 6 steps
