"""``ista_nl`` on the GPU, against the reference's recorded runs (tests/golden/ista_nl_cases.npz) and the host model
(tests/ista_nl_model.py).

Bars: the project's standing ones.  Codes: max|z - z_ref32| <= max(5e-5, 4 x spread_z), with spread_z how far "another
correct float32 implementation" moved the codes when the fixture was made (permuted summation orders, the normalisation
folded behind the product, the link in float64 rounded once); every case was admitted with spread_z <= 2.5e-3.  The
per-row L of 'auto' against the model: rtol = 4 x the model's float32 / float64 gap (test_auto_L_...).  The recorded
cases also hold L of the last step against the reference's float64 L: rtol = 4 x max(the reference's own float32 /
float64 gap, spread_L), but never below sqrt(k) 2^-23 -- the rounding a float32 sum of k terms carries whatever its
order; the host model's products are torch's blocked sums, so at k = 4100 its gap (3.6e-7) says little about another
order (sqrt(k) 2^-23 = 7.6e-6 there, 5.2e-7 at k = 19)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ista_nl_model as model
import test_workspace_gpu as wsg
from ista_nl_cases import CASES, SPREAD_Z_CAP, case_inputs, load_case, run_model
from layouts import SENTINEL, place, plans
from margins import record_margins

pytestmark = pytest.mark.gpu
ACT = dict(identity=0, sigmoid=1, tanh=2, relu=3)
_MODULES = dict(identity=torch.nn.Identity, sigmoid=torch.nn.Sigmoid, tanh=torch.nn.Tanh, relu=torch.nn.ReLU)


@pytest.fixture(scope="module")
def cases(golden):
    return golden("ista_nl_cases")


def bar_of(g):
    assert float(g["spread_z"]) <= SPREAD_Z_CAP
    return max(5e-5, 4.0 * float(g["spread_z"]))


def run(spec, decoder="affine", **more):
    """-> (z on the CPU, info, printed text); inputs go to the GPU and must come back bitwise unchanged"""
    from lasso_amd.nonlinear import affine, ista_nl
    x, w, b, z0, u0 = case_inputs(spec)
    xg, wg, zg, ug = x.cuda(), w.cuda(), z0.cuda(), u0.cuda()
    bg = b.cuda() if b is not None else None
    if decoder == "affine":
        dec = affine(wg, bg, spec["activation"])
    else:
        lin = torch.nn.Linear(spec["k"], spec["d"], bias=b is not None).cuda()
        with torch.no_grad():
            lin.weight.copy_(wg)
            if b is not None:
                lin.bias.copy_(bg)
        dec = lin if decoder == "linear" else torch.nn.Sequential(lin, _MODULES[spec["activation"]]())
    kw = dict(spec["kwargs"], alpha=spec["alpha"], power_init=ug, return_info=True)
    kw.update(more)
    with wsg._quiet() as said:
        z, info = ista_nl(xg, zg, dec, **kw)
    assert said[0] == []                                                          # no warning
    assert z.is_cuda and z.dtype == torch.float32 and z.data_ptr() != zg.data_ptr() and not z.requires_grad
    assert wsg._same(xg.cpu(), x) and wsg._same(wg.cpu(), w) and wsg._same(zg.cpu(), z0) and wsg._same(ug.cpu(), u0)
    assert b is None or wsg._same(bg.cpu(), b)
    return z.cpu(), info, said[1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case(cases, name):
    spec, g = CASES[name], load_case(cases, name)
    z, info, _ = run(spec, decoder="sequential" if spec["seed"] == 0 and spec["n"] == 24 else "affine")
    want, bar = torch.from_numpy(g["z32"]), bar_of(g)
    dz = float((z - want).abs().max())
    print("%s: iterations %d (golden %d), max|dz| = %.3g (bar %.3g)" % (name, info["iterations"], len(g["deltas32"]), dz, bar))
    assert torch.isfinite(z).all()
    assert info["iterations"] == len(g["deltas32"]) and info["stopped"] == bool(g["stopped"])
    assert dz <= bar, (name, dz, bar)
    rel = float(np.max(np.abs(np.array(info["deltas"]) - g["deltas32"]) / np.abs(g["deltas32"])))
    print("%s: per-iteration sums rel %.3g" % (name, rel))
    margins = dict(dz=dz, bar=bar, deltas_rel=rel)
    if spec["kwargs"]["lr"] == "auto":
        l64 = torch.from_numpy(g["L64"])
        gap = float(((torch.from_numpy(g["L32"]).double() - l64).abs() / l64.abs()).max())
        err = float(((info["L"].cpu().double() - l64).abs() / l64.abs()).max())
        rtol = max(4.0 * max(gap, float(g["spread_L"])), spec["k"] ** 0.5 * 2.0 ** -23)
        print("%s: L rel %.3g (rtol %.3g)" % (name, err, rtol))
        assert info["L"].shape == (spec["n"],) and err <= rtol
        margins.update(L_rel=err, L_rtol=rtol)
    else:
        assert info["L"] is None
    record_margins("ista_nl/" + name, margins)


def test_the_stop_rule_fires_where_the_reference_s_does(cases):
    spec, g = CASES["sigmoid_mid_stop"], load_case(cases, "sigmoid_mid_stop")
    assert spec["kwargs"]["maxiter"] == 200 and bool(g["stopped"]) and 8 < len(g["deltas32"]) < 200
    z, info, text = run(spec, verbose=2)
    budget = spec["n"] * spec["k"] * spec["kwargs"]["tol"]
    assert info["stopped"] and info["iterations"] == len(g["deltas32"])
    assert info["deltas"][-1] <= budget and all(dl > budget for dl in info["deltas"][:-1])
    assert float((z - torch.from_numpy(g["z32"])).abs().max()) <= bar_of(g)
    # the reference's three kinds of lines; the iteration that stops prints none
    got, want = text.strip().split("\n"), str(g["stdout"]).strip().split("\n")
    assert len(got) == len(want) == info["iterations"] + 1
    for a, b in zip(got, want):
        assert a.split(":")[0] == b.split(":")[0]
        assert abs(float(a.split(":")[1]) - float(b.split(":")[1])) <= 2e-4 + 1e-5 * abs(float(b.split(":")[1])), (a, b)


@pytest.mark.parametrize("name", ["tanh_small_fixed", "relu_mid_auto"])
def test_no_iteration_returns_z0_and_no_tolerance_runs_them_all(name):
    spec = dict(CASES[name], start="warm")
    z0 = case_inputs(spec)[3]
    z, info, _ = run(spec, maxiter=0)
    assert torch.equal(z, z0) and info == dict(iterations=0, deltas=[], stopped=False, L=None)
    z, info, _ = run(spec, maxiter=7, tol=0.0)
    assert info["iterations"] == 7 and len(info["deltas"]) == 7 and not info["stopped"]
    zm, im = run_model(spec, maxiter=7, tol=0.0)
    assert float((z - zm).abs().max()) <= 5e-5
    # without a trace there is nothing to read: the same codes
    from lasso_amd.nonlinear import affine, ista_nl
    x, w, b, _, u0 = case_inputs(spec)
    z2 = ista_nl(x.cuda(), z0.cuda(), affine(w.cuda(), None if b is None else b.cuda(), spec["activation"]),
                 **dict(spec["kwargs"], alpha=spec["alpha"], power_init=u0.cuda(), maxiter=7, tol=0.0))
    assert torch.equal(z2.cpu(), z)


@pytest.mark.parametrize("activation", model.ACTIVATIONS)
def test_auto_L_against_the_model_and_the_largest_eigenvalue(activation):
    spec = CASES["%s_small_auto" % activation]
    x, w, b, z0, u0 = case_inputs(spec)
    z, info, _ = run(spec, maxiter=1)
    _, i32 = run_model(spec, maxiter=1)
    _, i64 = run_model(spec, maxiter=1, dtype=torch.float64)
    gap = float(((i32["L"].double() - i64["L"]).abs() / i64["L"].abs()).max())
    err = float(((info["L"].cpu().double() - i64["L"]).abs() / i64["L"].abs()).max())
    rtol = 4.0 * gap
    print("%s: L rel %.3g (rtol %.3g, model gap %.3g)" % (activation, err, rtol, gap))
    assert err <= rtol
    # a Rayleigh quotient of unit vectors never exceeds the largest eigenvalue (the first step's point is y = z0)
    lam = torch.linalg.eigvalsh(model.row_hessians(x, w, b, activation, z0))[:, -1]
    assert (info["L"].cpu().double() <= lam * (1 + 1e-5)).all() and (info["L"].cpu() > 0).all()
    record_margins("ista_nl/L_%s" % activation, dict(rel=err, rtol=rtol, gap=gap))


@pytest.mark.parametrize("name", ["sigmoid_blocks_auto", "relu_ragged_auto", "tanh_small_stop_auto", "identity_mid_fixed"])
def test_two_identical_solves_are_bitwise_equal(name):
    a, b = run(CASES[name]), run(CASES[name])
    assert torch.equal(a[0], b[0]) and a[1]["deltas"] == b[1]["deltas"] and a[1]["iterations"] == b[1]["iterations"]
    if a[1]["L"] is not None:
        assert torch.equal(a[1]["L"], b[1]["L"])
    assert set(a[1]) == {"iterations", "deltas", "stopped", "L"}


def test_the_three_decoder_forms_and_a_drawn_start_and_cpu_tensors(cases):
    from lasso_amd.nonlinear import affine, ista_nl
    spec, g = CASES["identity_small_fixed"], load_case(cases, "identity_small_fixed")
    za, zl, zs = run(spec)[0], run(spec, decoder="linear")[0], run(spec, decoder="sequential")[0]
    assert torch.equal(za, zl) and torch.equal(za, zs)
    x, w, b, z0, u0 = case_inputs(spec)
    zc = ista_nl(x, z0, affine(w, b), alpha=spec["alpha"], **spec["kwargs"])      # staged through the device
    assert zc.device.type == "cpu" and torch.equal(zc, za)
    zg = ista_nl(x.cuda().requires_grad_(), z0.cuda().requires_grad_(), affine(w.cuda().requires_grad_(), b.cuda()),
                 alpha=spec["alpha"], **spec["kwargs"])
    assert not zg.requires_grad and torch.equal(zg.cpu(), za)
    assert ista_nl(x[:0].cuda(), z0[:0].cuda(), affine(w.cuda(), b.cuda()), lr=0.1).shape == (0, 19)
    # power_init=None draws a start on the device: another estimate of the same L, so nearby codes
    auto = CASES["identity_small_auto"]
    z1, i1, _ = run(auto, power_init=None)
    z2 = run(auto)[0]
    assert torch.isfinite(z1).all() and i1["L"].shape == (5,) and float((z1 - z2).abs().max()) < 0.2


# ---- the C ABI directly: pitched, odd-pitch and offset operands, 128 x 128 blocks, the refusals --------------------------
def abi_solve(spec, plan=None, reserved=0, activation=None, null_u0=False, dtype=0, check=True):
    """-> (z on the CPU, result, status); every placed operand is checked: inputs and padding untouched"""
    from lasso_amd import _native as nat
    x, w, b, z0, u0 = case_inputs(spec)
    n, d, k = spec["n"], spec["d"], spec["k"]
    kw = spec["kwargs"]
    auto = kw["lr"] == "auto"
    plan = plan or {}
    ops = {nm: place(t, plan.get(nm, "natural"), float("nan"), "cuda", nm) for nm, t in (("x", x), ("w", w), ("z0", z0), ("u0", u0))}
    out = place(torch.zeros(n, k), plan.get("z", "natural"), SENTINEL, "cuda", "z", fill=SENTINEL)
    bg = b.cuda() if b is not None else None
    opts = nat.IstaNlOptions(kw["maxiter"], int(kw["fast"]), int(auto), kw["power_iters"], 0.0 if auto else kw["lr"], kw["tol"], reserved)
    res = nat.IstaNlResult()
    L = nat.lib()
    ws = torch.empty(max(L.lasso_ista_nl_workspace_bytes(n, d, k, nat.LASSO_F32, int(auto)), 1), dtype=torch.uint8, device="cuda")
    status = L.lasso_ista_nl_solve(nat.ptr(ops["x"].view), ops["x"].ld, nat.ptr(ops["w"].view), ops["w"].ld, nat.ptr(bg),
                                   nat.ptr(ops["z0"].view), ops["z0"].ld, nat.ptr(out.view), out.ld,
                                   None if null_u0 else nat.ptr(ops["u0"].view), ops["u0"].ld, n, d, k, dtype, spec["alpha"],
                                   ACT[spec["activation"]] if activation is None else activation, C.byref(opts), C.byref(res),
                                   None, nat.ptr(ws), ws.numel(), nat.stream_ptr(torch.device("cuda", 0)))
    torch.cuda.synchronize()
    if check:
        nat.check(status)
    for p in ops.values():
        p.check()
    out.check(written=True)
    return out.view.cpu(), res, status


_PLAN_NAMES = ("x", "w", "z0", "z", "u0")


@pytest.mark.parametrize("tag,plan", plans(_PLAN_NAMES)[1:])
def test_pitched_odd_and_offset_operands_through_the_c_abi(cases, tag, plan):
    name = "relu_ragged_auto"
    spec, g = CASES[name], load_case(cases, name)
    z, res, _ = abi_solve(spec, plan)
    dz = float((z - torch.from_numpy(g["z32"])).abs().max())
    print("%s %s: max|dz| = %.3g" % (name, tag, dz))
    assert res.n_iter == len(g["deltas32"]) and dz <= bar_of(g)


@pytest.mark.parametrize("name", ["sigmoid_small_fixed", "tanh_small_auto", "identity_ragged_fixed", "relu_ragged_auto",
                                  "relu_blocks_fixed", "sigmoid_blocks_auto", "tanh_blocks_auto", "identity_blocks_fixed"])
def test_forced_128_blocks(cases, name):
    spec, g = CASES[name], load_case(cases, name)
    z, res, _ = abi_solve(spec, reserved=1)
    dz = float((z - torch.from_numpy(g["z32"])).abs().max())
    print("%s with 128 x 128 blocks: max|dz| = %.3g (bar %.3g)" % (name, dz, bar_of(g)))
    assert res.n_iter == len(g["deltas32"]) and dz <= bar_of(g)
    record_margins("ista_nl/blocks128_" + name, dict(dz=dz, bar=bar_of(g)))


def test_refusals_write_nothing():
    from lasso_amd import _native as nat
    spec = CASES["sigmoid_small_auto"]
    for kw, status, word in ((dict(activation=4), nat.LASSO_ERR_UNSUPPORTED, "activation"),
                             (dict(activation=-1), nat.LASSO_ERR_UNSUPPORTED, "activation"),
                             (dict(null_u0=True), nat.LASSO_ERR_BAD_ARG, "u0"),
                             (dict(dtype=nat.LASSO_F64), nat.LASSO_ERR_UNSUPPORTED, "dtype"),
                             (dict(reserved=2), nat.LASSO_ERR_BAD_ARG, "reserved")):
        z, res, got = abi_solve(spec, check=False, **kw)
        assert got == status and word in nat.lib().lasso_hip_last_error().decode(), kw
        assert (z == SENTINEL).all()
    assert nat.lib().lasso_ista_nl_workspace_bytes(5, 7, 19, nat.LASSO_F64, 0) == 0
    assert nat.lib().lasso_ista_nl_workspace_bytes(5, 7, 19, nat.LASSO_F32, 1) > nat.lib().lasso_ista_nl_workspace_bytes(5, 7, 19, nat.LASSO_F32, 0) > 0
