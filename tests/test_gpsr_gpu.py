"""GPSR-Basic on the HIP path (csrc/gpsr.hip) against the goldens recorded from the reference and, for shapes
that have none, against the host model (tests/gpsr_model.py).

Bars.  Objective rtol 1e-6.  max|dz|: per case, 4 x the gap between the model in float32 and the model in float64
(gpsr_cases.z_bar), never tighter than 5e-5.  lambda: rtol 1e-5 on the goldens (whose generator certified that the
step trace moves by less than a quarter of that between float32 and float64); against the model on fresh shapes the
same rule as for z -- 4 x the relative gap between the model's float32 and float64 steps, never tighter than 1e-5
(the step is a ratio of two batch-wide sums over a changing support: config 2's shape at 20 iterations moves it by
1.0e-5 through rounding alone).  Measured gaps and achieved deviations go to parity_margins.json through
tests/margins.py."""
import ctypes as C
import io
import sys
import warnings
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import gpsr_model
from gpsr_cases import CASES, case_inputs, check_against_golden, load_case, same_line, z_bar
from layouts import SENTINEL, place
from margins import record_margins
from recipes import recipe_xw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(golden):
    return golden("gpsr_cases")


def hip(x, w, tau, x0=None, **kw):
    from lasso_amd.linear.solvers import gpsr_basic
    return gpsr_basic(x.cuda(), w.cuda(), tau, x0=None if x0 is None else x0.cuda(), return_info=True, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case(cases, name):
    from lasso_amd.linear import sparse_encode
    spec, gold = CASES[name], load_case(cases, name)
    x, w, z0 = case_inputs(spec)
    bar, gap, _, _ = z_bar(x, w, spec["alpha"], x0=z0, **spec["kwargs"])
    xg, wg, z0g = x.cuda(), w.cuda(), None if z0 is None else z0.cuda()
    keep = xg.clone(), wg.clone(), None if z0 is None else z0g.clone()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        z, info = sparse_encode(xg, wg, alpha=spec["alpha"], z0=z0g, algorithm="gpsr", return_info=True, **spec["kwargs"])
    assert z.is_cuda and z.dtype == torch.float32 and z.shape == (spec["n"], spec["k"])
    dz = check_against_golden(name, z.cpu(), info, gold, bar, caught)
    if spec["kwargs"].get("stop_criterion", 3) != 1:   # (criterion 1 is a difference of two objectives: its own rounding
        np.testing.assert_allclose(info["criterion"], gold["criterion"], rtol=1e-4, err_msg=name)   # is pinned by n_iter)
    assert torch.equal(xg, keep[0]) and torch.equal(wg, keep[1]) and (z0 is None or torch.equal(z0g, keep[2]))
    record_margins("gpsr/golden/" + name, dict(model_f32_f64_gap=gap, bar=bar, hip_max_dz=dz))


FRESH = [(37, 10, 50), (64, 256, 1024), (130, 128, 512), (40, 300, 70), (24, 96, 1300)]


def against_model(tag, x, w, tau, x0=None, solve=None, model=None, **kw):
    """solve: hip (the Python entry point) or a function of its arguments; model: z_bar's tuple, where it is shared"""
    bar, gap, z_m, info_m = model or z_bar(x, w, tau, x0=x0, **kw)
    for fn, bound, f in info_m["decisions"]:          # the model's branches are not within rounding of flipping
        assert abs(fn - bound) >= 1e-4 * abs(f), (tag, fn, bound, f)
    z, info = (solve or hip)(x, w, tau, x0=x0, **kw)
    assert info["iterations"] == info_m["iterations"], tag
    assert info["trials"] == info_m["trials"], tag
    np.testing.assert_allclose(info["objective"], info_m["objective"], rtol=1e-6, err_msg=tag)
    lam_bar = max(1e-5, 4.0 * info_m["lambda_sensitivity"])
    lam_dev = float(np.max(np.abs(np.array(info["accepted_lambda"]) / np.array(info_m["accepted_lambda"]) - 1.0)))
    print(tag, "lambda: model f32/f64 %.3g, bar %.3g, hip %.3g" % (info_m["lambda_sensitivity"], lam_bar, lam_dev))
    assert lam_dev <= lam_bar, (tag, lam_dev, lam_bar)
    obj = np.array(info["objective"])
    assert (np.diff(obj) <= 0).all(), tag             # non-increasing over the accepted iterations
    dz = float((z.cpu() - z_m).abs().max())
    record_margins("gpsr/model/" + tag, dict(model_f32_f64_gap=gap, bar=bar, hip_max_dz=dz, lambda_bar=lam_bar,
                                             lambda_model_f32_f64=info_m["lambda_sensitivity"], hip_lambda_dev=lam_dev))
    assert dz <= bar, (tag, dz, bar)
    return z, info


@pytest.mark.parametrize("shape", FRESH, ids=lambda s: "x".join(map(str, s)))
def test_fresh_shapes_against_the_model(shape):
    n, d, k = shape
    x, w = recipe_xw(n, d, k, seed=20 + n)
    against_model("%dx%dx%d" % shape, x, w, 0.4, maxiter=5, tol=0.0)


def test_config2_shape_against_the_model():
    x, w = recipe_xw(4096, 256, 1024, seed=0)
    against_model("c2_4096x256x1024", x, w, 0.5, maxiter=20, tol=0.0)


def test_starts_x0_init0_init2_and_continuation_debias_on_a_ragged_shape():
    x, w = recipe_xw(70, 40, 130, seed=31)
    against_model("init2", x, w, 0.5, init=2, maxiter=6, tol=0.0)
    z0 = 0.1 * torch.randn(70, 130, generator=torch.Generator().manual_seed(5))
    against_model("x0", x, w, 0.5, x0=z0, maxiter=6, tol=0.0)
    against_model("init0", x, w, 0.5, init=0, maxiter=6, tol=0.0)
    z, info = against_model("debias", x, w, 0.9, maxiter=6, tol=0.0, debias=True, maxiter_debias=5)
    assert info["iterations"] == 6 + 6 and 0 < int((z != 0).sum()) <= x.numel()      # the CG ran: 6 steps on the support


def test_sufficient_decrease_holds_at_every_accepted_step():
    """F <= f + mu g, re-derived in float64 from the HIP iterates themselves (solves of 0, 1, 2, ... iterations)"""
    mu, tau = 0.1, 0.4
    x, w = recipe_xw(37, 10, 50, seed=57)
    x64, w64 = x.double(), w.double()
    ay = x64 @ w64
    zs, infos = [torch.zeros(37, 50, dtype=torch.float64)], []
    for m in range(1, 6):
        z, info = hip(x, w, tau, maxiter=m, tol=0.0)
        zs.append(z.cpu().double())
        infos.append(info)
    last = infos[-1]
    assert len(last["objective"]) == 5
    for j in range(5):
        assert infos[j]["objective"] == last["objective"][:j + 1]        # a longer solve repeats the shorter one
        z = zs[j]
        u, v = z.clamp(min=0), (-z).clamp(min=0)
        t = (z @ w64.T) @ w64 - ay
        gu, gv = t + tau, -t + tau
        lam = last["accepted_lambda"][j]
        du, dv = (u - lam * gu).clamp(min=0) - u, (v - lam * gv).clamp(min=0) - v
        g = float((gu * du).sum() + (gv * dv).sum())
        f = float(0.5 * ((x64 - z @ w64.T) ** 2).sum() + tau * z.abs().sum())
        f_next = last["objective"][j]
        assert g < 0
        assert f_next <= f + mu * g + 1e-6 * abs(f), (j, f_next, f, g)
        assert f_next < f


def test_two_identical_calls_are_bitwise_equal_and_inputs_unchanged():
    x, w = recipe_xw(130, 128, 512, seed=3)
    xg, wg = x.cuda(), w.cuda()
    from lasso_amd.linear import sparse_encode
    a, ia = sparse_encode(xg, wg, 0.4, algorithm="gpsr", maxiter=7, return_info=True, mu=0.95, lambda_backtrack=0.6)
    b, ib = sparse_encode(xg, wg, 0.4, algorithm="gpsr", maxiter=7, return_info=True, mu=0.95, lambda_backtrack=0.6)
    assert torch.equal(a, b) and ia == ib
    assert max(ia["trials"]) > 1                       # the ladder ran
    assert torch.equal(xg.cpu(), x) and torch.equal(wg.cpu(), w)
    assert a.data_ptr() not in (xg.data_ptr(), wg.data_ptr())


def test_cpu_inputs_come_back_on_the_cpu_and_low_precision_rounds_once():
    from lasso_amd.linear import sparse_encode
    x, w = recipe_xw(33, 20, 60, seed=8)
    z_gpu = sparse_encode(x.cuda(), w.cuda(), 0.4, algorithm="gpsr", maxiter=5)
    z_cpu = sparse_encode(x, w, 0.4, algorithm="gpsr", maxiter=5)
    assert z_cpu.device.type == "cpu" and torch.equal(z_cpu, z_gpu.cpu())
    xb, wb = x.bfloat16(), w.bfloat16()
    zb = sparse_encode(xb.cuda(), wb.cuda(), 0.4, algorithm="gpsr", maxiter=5)
    z32 = sparse_encode(xb.float().cuda(), wb.float().cuda(), 0.4, algorithm="gpsr", maxiter=5)
    assert zb.dtype == torch.bfloat16 and torch.equal(zb, z32.bfloat16())


def test_empty_batch():
    from lasso_amd.linear import sparse_encode
    w = recipe_xw(1, 12, 30, seed=1)[1].cuda()
    z, info = sparse_encode(torch.empty(0, 12, device="cuda"), w, 0.3, algorithm="gpsr", return_info=True)
    assert z.shape == (0, 30) and z.is_cuda and info["iterations"] == 0


def test_zero_vector_early_return_warns():
    from lasso_amd.linear import sparse_encode
    x, w = recipe_xw(16, 16, 40, seed=11)
    with pytest.warns(UserWarning, match="tau is too small; solution is zero vector"):
        z = sparse_encode(x.cuda(), w.cuda(), alpha=50.0, algorithm="gpsr", maxiter=5)
    assert z.shape == (16, 40) and not z.any()


def test_verbose_lines_match_the_reference(cases):
    from lasso_amd.linear import sparse_encode
    spec, gold = CASES["default"], load_case(cases, "default")
    x, w, _ = case_inputs(spec)
    out = io.StringIO()
    with redirect_stdout(out):
        sparse_encode(x.cuda(), w.cuda(), alpha=spec["alpha"], algorithm="gpsr", verbose=2, **spec["kwargs"])
    ours, theirs = out.getvalue().splitlines(), str(gold["stdout"]).splitlines()
    assert len(ours) == len(theirs), (len(ours), len(theirs))
    for a, b in zip(ours, theirs):
        assert same_line(a, b), (a, b)
    # verbose=2 with a line search that reduces lambda, and verbose=1, against the model's prints
    for name, verbose in (("search", 2), ("debias", 1), ("debias", 2), ("cont", 2)):
        spec = CASES[name]
        x, w, _ = case_inputs(spec)
        o1, o2 = io.StringIO(), io.StringIO()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with redirect_stdout(o1):
                sparse_encode(x.cuda(), w.cuda(), alpha=spec["alpha"], algorithm="gpsr", verbose=verbose, **spec["kwargs"])
            with redirect_stdout(o2):
                gpsr_model.gpsr_basic(x, w, spec["alpha"], verbose=verbose, **spec["kwargs"])
        l1, l2 = o1.getvalue().splitlines(), o2.getvalue().splitlines()
        assert len(l1) == len(l2) and len(l1) > 10, (name, verbose, len(l1), len(l2))
        assert any("Iter =" in a for a in l1) == (name == "debias")
        for a, b in zip(l1, l2):
            assert same_line(a, b), (name, a, b)


def test_dict_learning_with_a_gpsr_e_step():
    from lasso_amd.linear import dict_learning
    from oracle import lasso_oracle as orc
    torch.manual_seed(0)
    data = torch.randn(100, 10)
    torch.manual_seed(1)
    weight, losses = dict_learning(data, 50, alpha=0.5, algorithm="gpsr", steps=5, progbar=False)
    torch.manual_seed(1)
    wm = torch.nn.functional.normalize(torch.nn.init.orthogonal_(torch.empty(10, 50)), dim=0)
    ref = torch.zeros(5)
    for i in range(5):
        z = gpsr_model.gpsr_basic(data, wm, 0.5)
        ref[i] = orc.lasso_objective(data, z, wm, 0.5)
        wm = orc.update_dict(wm, data, z)
    print("losses", losses.tolist(), "model", ref.tolist())
    record_margins("gpsr/dict_learning", dict(max_loss_diff=float((losses.cpu() - ref).abs().max())))
    assert torch.allclose(losses.cpu(), ref, atol=1e-5, rtol=0)
    assert weight.shape == (10, 50)


def test_float64_and_requires_grad_are_refused_by_name():
    from lasso_amd.linear import sparse_encode
    x, w = recipe_xw(8, 6, 20, seed=2)
    with pytest.raises(NotImplementedError, match="float64"):
        sparse_encode(x.double().cuda(), w.double().cuda(), 0.3, algorithm="gpsr")
    with pytest.raises(NotImplementedError, match="requires_grad"):
        sparse_encode(x.cuda(), w.cuda().requires_grad_(), 0.3, algorithm="gpsr")
    with torch.no_grad():                              # no graph is asked for: runs
        z = sparse_encode(x.cuda(), w.cuda().requires_grad_(), 0.3, algorithm="gpsr", maxiter=3)
    assert not z.requires_grad


def test_line_search_that_cannot_succeed_ends_with_a_warning():
    """the documented extension: a non-finite objective ends the solve (the reference would loop for ever) and the
    last accepted code -- here the start -- comes back"""
    from lasso_amd.linear import sparse_encode
    x, w = recipe_xw(20, 12, 30, seed=4)
    x[3, 5] = float("nan")
    with pytest.warns(UserWarning, match="line search failed"):
        z, info = sparse_encode(x.cuda(), w.cuda(), 0.1, algorithm="gpsr", maxiter=5, return_info=True)
    assert info["iterations"] == 0 and info["trials"] == [] and not z.any()
    with pytest.warns(UserWarning, match="line search failed"):
        z_m, info_m = gpsr_model.gpsr_basic(x, w, 0.1, maxiter=5, return_info=True)
    assert info_m["iterations"] == 0 and not z_m.any()


# ---- the C ABI directly: 128 x 128 GEMM blocks, forced (LASSO_FORCE_BLOCKS_128) and chosen ----------------------------------
# block_side() takes 128-blocks only from 2 x CUs blocks on (256 CUs: 8.4 M elements of the product), far above the
# shapes of this file.  The bit runs every product of the solve -- and so every epilogue mode of DESIGN 3.8, the ladder's
# rungs in blockIdx.z included -- on Tile<128, 128> at shapes with more than one 128-block in a dimension and a nearly
# empty last one; the contraction lengths give the three operand forms (a multiple of 32: LDS-DMA, of 4: 16-byte loads,
# odd: scalar loads) of both product kinds.
def abi_solve(x, w, tau, x0=None, reserved=0, layout="natural", refused=None, stop_criterion=3, tol=1e-2, maxiter=1000,
              miniter=5, init=0, continuation=False, debias=False, **kwargs):
    """lasso_gpsr_solve directly: `reserved` and pitched / offset operands are not reachable from Python.  The request
    and the report are the Python entry point's own -> (z on the CPU, info).  refused: the status a refusal must have;
    nothing may have been written then"""
    from lasso_amd import _native as nat
    from lasso_amd.linear.solvers import gpsr as py
    opt = dict(py._KW_DEFAULTS, **kwargs)
    n, d = x.shape
    k = w.shape[1]
    nan = float("nan")
    ops = [place(t, layout, nan, "cuda", nm) for t, nm in ((x, "x"), (w, "w")) + (((x0, "z0"),) if x0 is not None else ())]
    out = place(torch.zeros(n, k), layout, SENTINEL, "cuda", "z", fill=SENTINEL)
    options, res, keep = py._request(stop_criterion, tol, maxiter, miniter, init, continuation, debias, opt, x0 is not None)
    options.reserved = reserved
    L = nat.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = torch.empty(L.lasso_gpsr_workspace_bytes(n, d, k, nat.LASSO_F32), dtype=torch.uint8, device="cuda")
    z0p = ops[2] if x0 is not None else None
    status = L.lasso_gpsr_solve(nat.ptr(ops[0].view), ops[0].ld, nat.ptr(ops[1].view), ops[1].ld,
                                nat.ptr(z0p.view) if z0p else None, z0p.ld if z0p else 0, nat.ptr(out.view), out.ld, n, d, k,
                                nat.LASSO_F32, float(tau), C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(),
                                nat.stream_ptr(dev))
    torch.cuda.synchronize()
    for p in ops:
        p.check()
    if refused is not None:
        assert status == refused, (status, refused)
        out.check(written=False)
        return out.view.cpu(), None
    nat.check(status)
    out.check(written=True)
    assert res.flags == 0, res.flags
    return out.view.cpu(), py._report(res, keep, stop_criterion, tol, debias, opt, 0)


def forced(reserved, layout="natural"):
    return lambda x, w, tau, x0=None, **kw: abi_solve(x, w, tau, x0=x0, reserved=reserved, layout=layout, **kw)


F128 = [(130, 64, 288), (259, 36, 132), (131, 37, 131), (40, 200, 136), (1, 40, 24)]
F128_KW = dict(maxiter=5, tol=0.0)
_F128_MODEL = {}


def f128_problem(shape, tau=0.4, **kw):
    """a problem of this section and its model (z_bar), computed once -> (x, w, model)"""
    key = (shape, tau, tuple(sorted(kw.items())))
    if key not in _F128_MODEL:
        n, d, k = shape
        x, w = recipe_xw(n, d, k, seed=20 + n)
        _F128_MODEL[key] = (x, w, z_bar(x, w, tau, **kw))
    return _F128_MODEL[key]


@pytest.mark.parametrize("reserved", [8, 0], ids=["f128", "s64"])
@pytest.mark.parametrize("shape", F128, ids=lambda s: "x".join(map(str, s)))
def test_forced_128_blocks_against_the_model(shape, reserved):
    from lasso_amd import _native as nat
    assert nat.FORCE_BLOCKS_128 == 8
    x, w, model = f128_problem(shape, **F128_KW)
    against_model("%dx%dx%d_%s" % (shape + ("f128" if reserved else "s64",)), x, w, 0.4, solve=forced(reserved), model=model,
                  **F128_KW)


@pytest.mark.parametrize("reserved", [8, 0], ids=["f128", "s64"])
def test_forced_128_blocks_continuation_debias_and_a_ladder_of_trials(reserved):
    """the epilogue modes of the continuation steps and of the debias CG, and a line search whose rungs (blockIdx.z,
    a_stride) are decided on 128-blocks"""
    sfx = "_f128" if reserved else "_s64"
    # (two solves: a tau at which the continuation's first steps still decrease the objective by more than rounding
    # leaves more nonzeros than debias accepts)
    kw = dict(maxiter=6, tol=0.0, continuation=True, cont_steps=3, first_tau_factor=3.0)
    x, w, model = f128_problem((131, 37, 131), tau=0.5, **kw)
    z, info = against_model("cont_131x37x131" + sfx, x, w, 0.5, solve=forced(reserved), model=model, **kw)
    assert info["iterations"] == len(info["objective"]) == 8       # steps of 1, 1 and 6 iterations
    kw = dict(maxiter=6, tol=0.0, debias=True, maxiter_debias=5)
    x, w, model = f128_problem((131, 37, 131), tau=1.2, **kw)
    z, info = against_model("debias_131x37x131" + sfx, x, w, 1.2, solve=forced(reserved), model=model, **kw)
    assert info["iterations"] == 6 + 6 and 0 < int((z != 0).sum()) <= x.numel()      # the CG ran: 6 steps on the support
    kw = dict(maxiter=7, tol=0.0, mu=0.95, lambda_backtrack=0.6)
    x, w, model = f128_problem((259, 36, 132), **kw)
    assert max(model[3]["trials"]) > 1                 # the ladder runs
    against_model("ladder_259x36x132" + sfx, x, w, 0.4, solve=forced(reserved), model=model, **kw)


def test_forced_128_blocks_pitched_repeatable_and_refused():
    from lasso_amd import _native as nat
    force = nat.FORCE_BLOCKS_128
    shape = (259, 36, 132)
    x, w, model = f128_problem(shape, **F128_KW)
    a, ia = abi_solve(x, w, 0.4, reserved=force, **F128_KW)
    b, ib = abi_solve(x, w, 0.4, reserved=force, **F128_KW)
    assert torch.equal(a, b) and ia == ib              # two forced solves are bitwise equal
    p, ip = abi_solve(x, w, 0.4, reserved=force, layout="pitched", **F128_KW)
    assert torch.equal(p, a) and ip == ia              # the same kernels on another pitch: not a bit moves
    for layout in ("odd", "offset"):                   # the scalar loads: another order in the contraction
        z, _ = against_model("259x36x132_%s_f128" % layout, x, w, 0.4, solve=forced(force, layout), model=model, **F128_KW)
        print(layout, "bitwise the natural forced solve:", torch.equal(z, a))
    for bad in (force | 1, force | 2, force | 4, force | 0x7f00, 1):     # dense GPSR defines no other bit
        z, _ = abi_solve(x, w, 0.4, reserved=bad, refused=nat.LASSO_ERR_BAD_ARG, **F128_KW)
        assert (z == SENTINEL).all(), bad


def device_cus():
    from lasso_amd import _native as nat
    cus = C.c_int(0)
    nat.check(nat.lib().lasso_hip_device_cus(C.byref(cus)))
    return cus.value


def test_block_side_rule_at_its_threshold():
    """the smallest [n, 260] product that takes 128-blocks by itself: 3 column blocks, ceil(2 CUs / 3) row blocks, the
    last of them 91 rows; its [n, 32] products stay on 64-blocks (the mixed case).  The solve is unforced."""
    from lasso_amd import _native as nat
    L = nat.lib()
    cus = device_cus()
    d, k = 32, 260
    rb = -(-2 * cus // 3)
    n = 128 * (rb - 1) + 91
    ldmax_k, ldmax_d = max(d, k, d), max(d, k, d, k)   # as csrc/gpsr.hip takes them: ldx = d, ldw = k
    assert L.lasso_solver_block_side(n, k, ldmax_k) == 128
    assert L.lasso_solver_block_side(n - 128, k, ldmax_k) == 64
    assert L.lasso_solver_block_side(n, d, ldmax_d) == 64
    assert L.lasso_solver_block_side(n, k, 1 << 22) == 64                 # a row pitch beyond the 32-bit block offsets
    print("block_side threshold: %d CUs, n = %d" % (cus, n))
    x, w = recipe_xw(n, d, k, seed=41)
    against_model("threshold_%dx%dx%d" % (n, d, k), x, w, 0.4, solve=forced(0), maxiter=3, tol=0.0)
