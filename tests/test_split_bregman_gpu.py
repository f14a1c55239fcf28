"""split_bregman on the GPU against the reference's recorded runs (tests/golden/split_bregman_cases.npz) and the host
model (tests/split_bregman_model.py).

Bars.  x: max|x - x_ref32| <= max(5e-5, 4 x spread_z), where spread_z is how far "another correct float32
implementation" (the model with a row-major state, a double Hinv and permuted summation orders) moved x when the
fixture was made; the factor 4 and the 5e-5 floor are the project's rule (tests/test_gpsr_gpu.py, tests/test_own_gpu.py).
A case is admitted only with spread_z <= 2.5e-3, so the bar never exceeds 1e-2.  The update sequence: relative
max(1e-5, 4 x spread_update).  itn, iterations and stopped are equal to the fixture's: the generator refused every case
with an update within 1 % of tol.  Fresh shapes take the same rule with the spread measured here, from the same
variants of the model."""
import contextlib
import ctypes as C
import io
import re
import warnings

import numpy as np
import pytest
import torch

import split_bregman_model as model
from layouts import SENTINEL, place, plans
from margins import record_margins
from split_bregman_cases import CASES, ORDER_SEEDS, SPREAD_F_CAP, bar_z, case_inputs, load_case, rtol_update
from recipes import recipe_xw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(golden):
    return golden("split_bregman_cases")


def run(A, y, x0=None, **kw):
    """-> (x on the CPU, itn, info, warnings, printed text); inputs go to the GPU and must come back bitwise unchanged"""
    from lasso_amd.linear.solvers import split_bregman
    Ag, yg, x0g = A.cuda(), y.cuda(), None if x0 is None else x0.cuda()
    out = io.StringIO()
    with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(out):
        warnings.simplefilter("always")
        x, itn, info = split_bregman(Ag, yg, x0g, return_info=True, **kw)
    assert x.is_cuda and x.dtype == torch.float32 and x.shape == (y.shape[0], A.shape[1])
    assert x.data_ptr() not in (Ag.data_ptr(), yg.data_ptr()) and (x0g is None or x.data_ptr() != x0g.data_ptr())
    for dev, host in ((Ag, A), (yg, y), (x0g, x0)):           # (bit for bit: an operand may hold a NaN)
        assert host is None or torch.equal(dev.cpu().view(torch.int32), host.view(torch.int32))
    return x.cpu(), itn, info, [str(c.message) for c in caught], out.getvalue()


def abi_solve(A, y, x0, alpha, plan=None, reserved=0, cost=False, maxiter=20, niter_inner=5, lambd=1.0, tol=1e-10, tau=1.0,
              ld_override=None, expect=None):
    """lasso_split_bregman_solve directly: `reserved` and pitched / odd / offset operands are not reachable from Python.
    plan: {operand: layout} over x (the data y), w (A), x0, z (tests/layouts.py); -> (z on the CPU, result struct,
    updates, costs, the placed operands)"""
    from lasso_amd import _native as nat
    n, d = y.shape
    k = A.shape[1]
    plan = plan or {}
    ops = dict(x=place(y, plan.get("x", "natural"), float("nan"), "cuda", "x"),
               w=place(A, plan.get("w", "natural"), float("nan"), "cuda", "w"),
               z=place(torch.zeros(n, k), plan.get("z", "natural"), SENTINEL, "cuda", "z", fill=SENTINEL))
    if x0 is not None:
        ops["x0"] = place(x0, plan.get("x0", "natural"), float("nan"), "cuda", "x0")
    ld = {name: p.ld for name, p in ops.items()}
    ld.setdefault("x0", k)
    ld.update(ld_override or {})
    upd, cst = (C.c_double * maxiter)(), (C.c_double * maxiter)()
    trace = nat.SplitBregmanTrace(maxiter, 0, upd, cst if cost else None)
    opts = nat.SplitBregmanOptions(maxiter, niter_inner, reserved, 0, lambd, tol, tau)
    res = nat.SplitBregmanResult()
    res.trace = C.pointer(trace)
    L = nat.lib()
    ws = torch.empty(L.lasso_split_bregman_workspace_bytes(n, d, k, nat.LASSO_F32), dtype=torch.uint8, device="cuda")
    status = L.lasso_split_bregman_solve(
        C.c_void_p(ops["x"].view.data_ptr()), ld["x"], C.c_void_p(ops["w"].view.data_ptr()), ld["w"],
        C.c_void_p(ops["x0"].view.data_ptr()) if x0 is not None else None, ld["x0"], C.c_void_p(ops["z"].view.data_ptr()),
        ld["z"], n, d, k, nat.LASSO_F32, alpha, C.byref(opts), C.byref(res), nat.ptr(ws), ws.numel(),
        nat.stream_ptr(torch.device("cuda", 0)))
    torch.cuda.synchronize()
    if expect is None:
        nat.check(status)
    else:
        assert status == expect, (status, expect)
    its = res.n_iter
    return ops["z"].view.cpu(), res, list(upd[:its]), list(cst[:its]) if cost else None, ops


def rel_updates(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / np.abs(want)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case(cases, name):
    spec, g = CASES[name], load_case(cases, name)
    A, y, x0 = case_inputs(spec)
    x, itn, info, caught, text = run(A, y, x0, alpha=spec["alpha"], **spec["kwargs"])
    assert not caught and text == ""
    dx = float((x - torch.from_numpy(g["x32"])).abs().max())
    ru = rel_updates(info["update"], g["update32"]) if info["iterations"] == int(g["iterations"]) else float("inf")
    print("%s: max|dx| = %.3g (bar %.3g), update rel %.3g (rtol %.3g), itn %d iterations %d" %
          (name, dx, bar_z(g), ru, rtol_update(g), itn, info["iterations"]))
    record_margins("split_bregman/" + name, dict(dx=dx, bar=bar_z(g), update_rel=ru, update_rtol=rtol_update(g), itn=itn))
    assert torch.isfinite(x).all()
    assert itn == int(g["itn"]) and info["iterations"] == int(g["iterations"]) and info["stopped"] == bool(g["stopped"])
    assert bar_z(g) <= 1e-2
    assert dx <= bar_z(g), (name, dx, bar_z(g))
    assert ru <= rtol_update(g), (name, ru, rtol_update(g))
    assert "cost" not in info


@pytest.mark.parametrize("name", ["n40_d32_k257", "n16_d48_k1030"])
def test_forced_128_blocks_through_the_abi(cases, name):
    spec, g = CASES[name], load_case(cases, name)
    A, y, x0 = case_inputs(spec)
    z, res, upd, _, _ = abi_solve(A, y, x0, spec["alpha"], reserved=1, **spec["kwargs"])
    dx = float((z - torch.from_numpy(g["x32"])).abs().max())
    ru = rel_updates(upd, g["update32"])
    print("%s (128 x 128): max|dx| = %.3g (bar %.3g), update rel %.3g (rtol %.3g)" % (name, dx, bar_z(g), ru, rtol_update(g)))
    record_margins("split_bregman/%s_r1" % name, dict(dx=dx, bar=bar_z(g), update_rel=ru, update_rtol=rtol_update(g)))
    assert res.itn == int(g["itn"]) and res.n_iter == int(g["iterations"]) and bool(res.stopped) == bool(g["stopped"])
    assert res.cholesky_info == 0
    assert dx <= bar_z(g) and ru <= rtol_update(g)


# shapes the fixture does not hold: more than one block of rows, the 16-byte-load operand form (k % 4 == 0, k % 32 != 0)
# and the LDS-DMA form (k % 32 == 0), each with both block sizes
FRESH = [(130, 40, 96, 0), (130, 40, 96, 1), (70, 24, 68, 0), (70, 24, 68, 1), (131, 36, 30, 0)]


@pytest.mark.parametrize("n,d,k,reserved", FRESH)
def test_fresh_shape_against_the_model(n, d, k, reserved):
    y, A = recipe_xw(n, d, k, seed=22)
    kw = dict(maxiter=6, niter_inner=3)
    x32, itn32, i32 = model.split_bregman(A, y, alpha=0.3, **kw)
    spread_z, spread_u = 0.0, 0.0
    for knobs in model.variants(ORDER_SEEDS):
        xm, _, im = model.split_bregman(A, y, alpha=0.3, **knobs, **kw)
        spread_z = max(spread_z, float((xm - x32).abs().max()))
        spread_u = max(spread_u, rel_updates(im["update"], i32["update"]))
    bar, rtol = max(5e-5, 4.0 * spread_z), max(1e-5, 4.0 * spread_u)
    z, res, upd, _, _ = abi_solve(A, y, None, 0.3, reserved=reserved, **kw)
    dx, ru = float((z - x32).abs().max()), rel_updates(upd, i32["update"])
    print("fresh %s reserved=%d: max|dx| = %.3g (bar %.3g), update rel %.3g (rtol %.3g)" % ((n, d, k), reserved, dx, bar, ru, rtol))
    record_margins("split_bregman/fresh_%dx%dx%d_r%d" % (n, d, k, reserved), dict(dx=dx, bar=bar, update_rel=ru, update_rtol=rtol))
    assert res.n_iter == 6 and res.itn == itn32 == 5 and not res.stopped
    assert dx <= bar and ru <= rtol


def test_two_identical_calls_are_bitwise_equal():
    y, A = recipe_xw(70, 48, 64, seed=3)
    a = run(A, y, alpha=0.3, maxiter=4, verbose=True)
    b = run(A, y, alpha=0.3, maxiter=4, verbose=True)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and a[4] == b[4]
    assert a[2]["iterations"] == 4 and len(a[2]["update"]) == 4


def test_x0_only_moves_the_first_update():
    spec = CASES["n37_d19_k70"]
    A, y, _ = case_inputs(spec)
    g = torch.Generator().manual_seed(11)
    xa, ia, fa, _, _ = run(A, y, torch.randn(37, 70, generator=g), alpha=0.3, maxiter=4)
    xb, ib, fb, _, _ = run(A, y, torch.randn(37, 70, generator=g), alpha=0.3, maxiter=4)
    xn, _, fn, _, _ = run(A, y, None, alpha=0.3, maxiter=4)
    assert torch.equal(xa, xb) and torch.equal(xa, xn) and ia == ib == 3
    assert fa["update"][1:] == fb["update"][1:] == fn["update"][1:]
    assert len({fa["update"][0], fb["update"][0], fn["update"][0]}) == 3


def test_stop_rule_ends():
    spec = CASES["n37_d19_k70"]
    A, y, _ = case_inputs(spec)
    # a large tol: iteration 0 runs (update starts at +inf), the stop fires at the top of iteration 1
    x, itn, info, _, _ = run(A, y, alpha=0.3, tol=1e6)
    assert itn == 1 and info["iterations"] == 1 and info["stopped"] and len(info["update"]) == 1
    x1, itn1, info1, _, _ = run(A, y, alpha=0.3, maxiter=1)
    assert torch.equal(x, x1) and itn1 == 0 and not info1["stopped"] and info["update"] == info1["update"]
    # a negative tol never stops
    x, itn, info, _, _ = run(A, y, alpha=0.3, tol=-1.0, maxiter=7)
    assert itn == 6 and info["iterations"] == 7 and not info["stopped"] and len(info["update"]) == 7
    x7, itn7, info7, _, _ = run(A, y, alpha=0.3, maxiter=7)
    assert torch.equal(x, x7) and info["update"] == info7["update"]


def test_verbose_lines_and_costs(cases):
    name = "n37_d19_k70"
    spec, g = CASES[name], load_case(cases, name)
    A, y, x0 = case_inputs(spec)
    x, itn, info, _, text = run(A, y, x0, alpha=spec["alpha"], verbose=True)
    xq, _, infoq, _, _ = run(A, y, x0, alpha=spec["alpha"])
    assert torch.equal(x, xq) and info["update"] == infoq["update"]          # the cost product changes nothing else
    lines = text.strip().split("\n")
    assert len(lines) == info["iterations"] == len(info["cost"]) == 20
    for i, (line, cost) in enumerate(zip(lines, info["cost"])):
        m = re.fullmatch(r"iter +(\d+) - cost: (-?\d+\.\d{4})", line)
        assert m and int(m.group(1)) == i and line == 'iter %3d - cost: %0.4f' % (i, cost), line
        assert abs(float(m.group(2)) - cost) <= 0.5e-4 * (1 + 1e-9)
    # the float64 objective of the model's iterates: the iterates agree to the case's bar, the objective is smooth, and
    # the relative cap is the one tests/own_cases.py admits an objective comparison under
    _, _, i64 = model.split_bregman(A, y, x0, alpha=spec["alpha"], dtype=torch.float64, iterates=True)
    want = np.array([model.objective64(A, y, xi, spec["alpha"]) for xi in i64["iterates"]])
    rel = float(np.max(np.abs(np.array(info["cost"]) - want) / want))
    print("verbose: cost rel %.3g (cap %.3g)" % (rel, SPREAD_F_CAP))
    record_margins("split_bregman/verbose_cost", dict(rel=rel, cap=SPREAD_F_CAP))
    assert rel <= SPREAD_F_CAP
    assert abs(info["cost"][-1] - model.objective64(A, y, x, spec["alpha"])) <= 1e-6 * want[-1]      # ... and of x itself


def test_nan_in_y_is_an_ordinary_operand_and_nan_in_A_raises():
    from lasso_amd.linear.solvers import split_bregman
    A, y, _ = case_inputs(CASES["n37_d19_k70"])
    bad = y.clone()
    bad[5, 3] = float("nan")
    xc, _, ic, _, _ = run(A, y, alpha=0.3, maxiter=3)
    x, itn, info, caught, _ = run(A, bad, alpha=0.3, maxiter=3)
    assert not caught
    assert info["iterations"] == 3 and itn == 2 and not info["stopped"] and all(np.isnan(u) for u in info["update"])
    assert torch.isnan(x[5]).all()
    keep = torch.arange(37) != 5
    assert torch.equal(x[keep], xc[keep])
    bad_a = A.clone()
    bad_a[2, 7] = float("nan")
    with pytest.raises(torch.linalg.LinAlgError):
        split_bregman(bad_a.cuda(), y.cuda(), alpha=0.3, maxiter=3)


def test_layouts_through_the_c_abi():
    from lasso_amd import _native as nat
    n, d, k = 37, 32, 64
    y, A = recipe_xw(n, d, k, seed=21)
    x0 = torch.randn(n, k, generator=torch.Generator().manual_seed(3))
    kw = dict(maxiter=3, niter_inner=2, cost=True)
    anchor = None
    for tag, plan in plans(("x", "w", "x0", "z")):
        z, res, upd, cst, ops = abi_solve(A, y, x0, 0.3, plan=plan, **kw)
        for name, p in ops.items():
            p.check(written=(name == "z"))                     # guard bands intact, inputs only read
        assert res.n_iter == 3 and torch.isfinite(z).all(), tag
        if anchor is None:
            anchor = (z, upd, cst)                             # (what a solve is held to: test_golden_case)
        else:
            assert torch.equal(z, anchor[0]) and upd == anchor[1] and cst == anchor[2], tag
    # refusals: LASSO_ERR_BAD_ARG with nothing written
    for bad in (dict(ld_override=dict(x=d - 1)), dict(ld_override=dict(w=k - 1)), dict(ld_override=dict(x0=k - 1)),
                dict(ld_override=dict(z=k - 1)), dict(reserved=0x7f00), dict(lambd=0.0)):
        z, res, _, _, ops = abi_solve(A, y, x0, 0.3, plan=dict(z="pitched"), expect=nat.LASSO_ERR_BAD_ARG, maxiter=3, **bad)
        assert (ops["z"].buffer == SENTINEL).all(), bad
        for name, p in ops.items():
            p.check(written=False)


def test_cpu_tensors_in_cpu_tensors_out():
    from lasso_amd.linear.solvers import split_bregman
    A, y, _ = case_inputs(CASES["n8_d6_k10"])
    x, itn = split_bregman(A, y, alpha=0.3, maxiter=3)
    xg, itng = split_bregman(A.cuda(), y.cuda(), alpha=0.3, maxiter=3)
    assert x.device.type == "cpu" and xg.is_cuda and itn == itng == 2 and torch.equal(x, xg.cpu())
    x0 = torch.zeros(0, 10)
    xe, itne, infoe = split_bregman(A.cuda(), y[:0].cuda(), x0.cuda(), return_info=True)
    assert xe.shape == (0, 10) and xe.is_cuda and itne == 1 and infoe["stopped"]
