"""owlqn on the logistic objective ``bernoulli(x, weight)`` on the GPU, against the reference's recorded runs
(tests/golden/owlqn_glm_cases.npz) and the host model (tests/owlqn_glm_model.py).

Bars: those of tests/test_owlqn_gpu.py, unchanged.  Codes: max|z - z_ref32| <= max(5e-5, 4 x spread_z), with spread_z
how far "another correct float32 implementation" moved the codes when the fixture was made (permuted summation orders,
the vector-free direction, either objective fold, and the link in float64 rounded once against torch's float32
operations); a case is compared by its codes only if spread_z <= 2.5e-3.  Objective-only cases: max(1e-6, 4 x spread_f)
against the float64 run.  Per-iteration records: ``rtol_of``.  Fresh shapes take 4 x the model's float32 / float64 gap,
after asserting that no decision of the model is close enough to its threshold for rounding to flip it."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import owlqn_glm_model as model
import test_workspace_gpu as wsg
from margins import record_margins
from owlqn_glm_cases import CASES, admitted_f, admitted_z, case_inputs, load_case, recipe, rtol_of, warm_start
from test_owlqn_gpu import MODES, pitched, same_line

pytestmark = pytest.mark.gpu
NONFINITE = "owlqn: the objective is not finite; returning the last accepted iterate"


@pytest.fixture(scope="module")
def cases(golden):
    return golden("owlqn_glm_cases")


def run(w, x, z0, **kw):
    """-> (z on the CPU, info, warnings, printed text); inputs go to the GPU and must come back bitwise unchanged"""
    from lasso_amd.nonlinear import bernoulli, owlqn
    wg, xg, zg = w.cuda(), x.cuda(), z0.cuda()
    with wsg._quiet() as said:
        z, info = owlqn(bernoulli(xg, wg), zg, return_info=True, **kw)
    assert z.is_cuda and z.dtype == x.dtype and z.data_ptr() != zg.data_ptr()
    assert wsg._same(wg.cpu(), w) and wsg._same(xg.cpu(), x) and wsg._same(zg.cpu(), z0)
    return z.cpu(), info, said[0], said[1]


def abi_solve(w, x, z0, alpha, line_search, max_iter, lr=1.0, xtol=1e-5, history_size=100, reserved=0, pitches=None, family=1,
              check=True):
    """lasso_owlqn_glm_solve directly: `family`, `reserved` and pitched / offset operands are not reachable from Python.
    pitches = (ldx, ldw, ldz0, ldz) or None (packed) -> (z on the CPU, result struct, trace lists, the buffers, status)"""
    from lasso_amd import _native as nat
    n, d = x.shape
    k = w.shape[1]
    ls = model.LS_DEFAULTS
    ldx, ldw, ldz0, ldz = pitches or (d, k, k, k)
    (xv, xb), (wv, wb), (z0v, z0b) = pitched(x, ldx), pitched(w, ldw), pitched(z0, ldz0)
    zv, zb = pitched(torch.zeros(n, k), ldz)
    zb.fill_(-555.0)
    cap = max(max_iter, 1)
    t_arr, f_arr, dx_arr, h_arr = ((C.c_double * cap)() for _ in range(4))
    ls_arr, p_arr, s_arr = ((C.c_int32 * cap)() for _ in range(3))
    trace = nat.OwlqnTrace(cap, 0, t_arr, ls_arr, f_arr, dx_arr, p_arr, s_arr, h_arr, None, None, None, 0)
    opts = nat.OwlqnOptions(max_iter, MODES[line_search], int(ls["maxiter"]), history_size, lr, xtol, ls["tol"], ls["decay"],
                            reserved)
    res = nat.OwlqnResult()
    res.trace = C.pointer(trace)
    L = nat.lib()
    pairs = max(0, min(history_size, max_iter - 1))
    ws = torch.empty(L.lasso_owlqn_workspace_bytes(n, d, k, nat.LASSO_F32, pairs), dtype=torch.uint8, device="cuda")
    status = L.lasso_owlqn_glm_solve(C.c_void_p(xv.data_ptr()), ldx, C.c_void_p(wv.data_ptr()), ldw, C.c_void_p(z0v.data_ptr()),
                                     ldz0, C.c_void_p(zv.data_ptr()), ldz, n, d, k, nat.LASSO_F32, alpha, family,
                                     C.byref(opts), C.byref(res), nat.ptr(ws), ws.numel(),
                                     nat.stream_ptr(torch.device("cuda", 0)))
    if check:
        nat.check(status)
    torch.cuda.synchronize()
    its = res.n_iter
    lists = dict(ls_iters=list(ls_arr[:its]), pairs=list(p_arr[:its]), skipped=[bool(v) for v in s_arr[:its]],
                 objective=list(f_arr[:its]))
    return zv.cpu(), res, lists, dict(x=(xb, x, ldx), w=(wb, w, ldw), z0=(z0b, z0, ldz0), z=(zb, None, ldz)), status


def model_pair(w, x, z0, alpha, **kw):
    """the model in float32 and float64 -> (z32, info32, z64, info64, gap); asserts its decisions are robust"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z32, i32 = model.owlqn(w, x, z0, alpha=alpha, **kw)
        z64, i64 = model.owlqn(w, x, z0, alpha=alpha, dtype=torch.float64, **kw)
    for info in (i32, i64):
        model.assert_robust(info)
    assert i32["ls_iters"] == i64["ls_iters"] and i32["iterations"] == i64["iterations"]
    assert i32["skipped"] == i64["skipped"] and i32["pairs"] == i64["pairs"]
    return z32, i32, z64, i64, float((z32.double() - z64).abs().max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case(cases, name):
    spec, g = CASES[name], load_case(cases, name)
    x, w, z0 = case_inputs(spec)
    kw = spec["kwargs"]
    brent = kw["line_search"] == "brent"
    z, info, caught, text = run(w, x, z0, alpha=spec["alpha"], verbose=2, **kw)
    assert torch.isfinite(z).all()
    assert caught == sorted(m for m in str(g["warnings"]).split("\n") if m)           # (so: no non-finite warning)
    assert info["iterations"] == len(g["f32"])
    # the memory held and dropped what the reference's did
    assert info["pairs"] == list(g["pairs"]) and [int(s) for s in info["skipped"]] == list(g["skipped"])
    f_z = model.objective64(w, x, z, spec["alpha"])
    f_last = info["objective"][-1] if info["objective"] else float(text.split("\n")[0].split(":")[1])
    print("%s: reported objective %.9g, objective of z %.9g" % (name, f_last, f_z))
    assert np.isfinite(f_last)
    assert abs(f_last - f_z) <= (1e-6 if info["objective"] else 1e-4) * f_z     # ('initial f: %0.4f' is all max_iter = 0 says)
    if spec["start"] == "saturated":
        assert float((z0 @ w.T).abs().max()) >= 100.0
        f0 = float(text.split("\n")[0].split(":")[1])
        assert abs(f0 - float(g["f0"])) <= 1e-4 * float(g["f0"]) + 1e-4
    margins = {}
    if spec["compare"] == "z":
        assert admitted_z(g)
        bar = max(5e-5, 4.0 * float(g["spread_z"]))
        assert bar <= 1e-2
        dz = float((z - torch.from_numpy(g["z32"])).abs().max())
        print("%s: max|dz| = %.3g (bar %.3g)" % (name, dz, bar))
        if not brent:
            assert info["ls_iters"] == list(g["ls32"])
        rel = {}
        for key, got, want in (("t", info["t"], g["t32"]), ("objective", info["objective"], g["f32"]),
                               ("delta", info["delta_x"], g["dx32"])):
            if len(want) and (np.abs(want) > 0).all():
                rel[key] = float(np.max(np.abs(np.array(got) - want) / np.abs(want)))
                print("%s: %s rel %.3g (rtol %.3g)" % (name, key, rel[key], rtol_of(g, key)))
            else:
                assert list(got) == list(want)                        # (no iteration, or a step of length 0)
        assert dz <= bar, (name, dz, bar)
        for key in rel:
            assert rel[key] <= rtol_of(g, key), (name, key, rel[key], rtol_of(g, key))
        if kw["max_iter"] > 0:                                         # (the reference's closing print needs an iteration)
            got_lines, want_lines = text.strip().split("\n"), str(g["stdout"]).strip().split("\n")
            assert len(got_lines) == len(want_lines)
            if not brent:                                             # (Brent's evaluation count is not pinned)
                for a, b in zip(got_lines, want_lines):
                    assert same_line(a, b, max(rtol_of(g, key) for key in ("t", "objective", "delta"))), (a, b)
        margins = dict(dz=dz, bar=bar, **rel)
    else:
        f_ref = float(g["f64"][-1])
        err = abs(info["objective"][-1] - f_ref) / f_ref
        bar = max(1e-6, 4.0 * float(g["spread_f"]))
        print("%s: objective rel %.3g (bar %.3g, admitted %s)" % (name, err, bar, admitted_f(g)))
        objs = [float(text.split("\n")[0].split(":")[1])] + info["objective"]
        if kw["line_search"] == "backtrack":                           # an accepted trial passed the sufficient-decrease test
            assert all(b <= a * (1 + 1e-6) for a, b in zip(objs, objs[1:])), objs
        if brent:
            # a bounded Brent search on (0, 10) promises no descent -- the reference's own runs of brent8_wide rise at the
            # fourth iteration, in float32 and in float64 -- but the step it returns is the best abscissa it saw
            for it in range(1, info["iterations"] + 1):
                seen = [f for i, _, f in info["evaluations"] if i == it]
                assert len(seen) == info["ls_iters"][it - 1] and abs(info["objective"][it - 1] - min(seen)) <= 1e-6 * min(seen)
        if spec["compare"] == "f":
            assert admitted_f(g)
        if admitted_f(g):
            assert err <= bar, (name, err, bar)
        margins = dict(objective_rel=err, bar=bar, admitted=bool(admitted_f(g)))
    record_margins("owlqn_glm/" + name, margins)


@pytest.mark.parametrize("name", ["brent_small", "brent_ragged"])
def test_brent_evaluations_are_the_line_objective(name):
    spec = CASES[name]
    x, w, z0 = case_inputs(spec)
    z, info, _, _ = run(w, x, z0, alpha=spec["alpha"], **spec["kwargs"])
    evals = info["evaluations"]
    assert len(evals) == info["ls_iters"][0] and 5 <= len(evals) <= 60 and all(e[0] == 1 for e in evals)
    assert all(0.0 < e[1] < 10.0 for e in evals)
    line64 = model.first_line_objective(w, x, z0, spec["alpha"], torch.float64)
    line32 = model.first_line_objective(w, x, z0, spec["alpha"], torch.float32, accurate_f=False)
    want = np.array([line64(float(np.float32(t))) for _, t, _ in evals])      # (the step is applied as a float32)
    gap = float(np.max(np.abs(np.array([line32(float(np.float32(t))) for _, t, _ in evals]) - want) / want))
    rtol = max(1e-6, 4.0 * gap)
    err = float(np.max(np.abs(np.array([f for _, _, f in evals]) - want) / want))
    print("%s: %d evaluations, rel %.3g (rtol %.3g, model gap %.3g)" % (name, len(evals), err, rtol, gap))
    assert err <= rtol
    best = min(reversed(evals), key=lambda e: e[2])          # (a tie goes to the later evaluation)
    assert info["t"][0] == best[1]
    record_margins("owlqn_glm/evaluations_" + name, dict(rel=err, rtol=rtol, count=len(evals)))


# (n, d, k, reserved, seed, line_search): an odd everything, 128-blocks forced, d and k multiples of 32 (the LDS-DMA operand
# form) with more than one block, a ragged one, one row, one feature, one atom, k beyond 4096.  A fixed step only: four
# backtracking iterations from t = 1 are chaotic on this objective even at (37, 50, 30) and (13, 10, 1) -- the model with an
# order_seed ends 1.3e-2 and 8.7e-4 from the model while its float32 / float64 gap is 1.5e-3 and 1e-5, so that gap is no bar
# there (tests/test_owlqn_gpu.py found the same for rss); the recorded backtracking cases carry a measured spread instead.
FRESH = [(37, 50, 30, 0, 22, "none"), (37, 50, 30, 1, 22, "none"), (40, 64, 320, 0, 22, "none"), (40, 64, 320, 1, 22, "none"),
         (130, 24, 100, 0, 23, "none"), (130, 24, 100, 1, 23, "none"), (3, 12, 4101, 0, 22, "none"),
         (1, 9, 21, 0, 24, "none"), (1, 9, 21, 1, 24, "none"), (11, 1, 6, 0, 25, "none"), (11, 1, 6, 1, 25, "none"),
         (13, 10, 1, 0, 26, "none"), (13, 10, 1, 1, 26, "none")]


@pytest.mark.parametrize("n,d,k,reserved,seed,line_search", FRESH)
def test_fresh_shape_against_the_model(n, d, k, reserved, seed, line_search):
    x, w = recipe(n, d, k, seed=seed)
    z0 = torch.zeros(n, k)
    kw = dict(line_search=line_search, max_iter=4, history_size=2, lr=1.0 if line_search == "backtrack" else 0.05)
    z32, i32, z64, i64, gap = model_pair(w, x, z0, 0.1, **kw)
    bar = max(5e-5, 4.0 * gap)
    z, res, got, _, _ = abi_solve(w, x, z0, 0.1, line_search, 4, lr=kw["lr"], history_size=2, reserved=reserved)
    dz = float((z - z32).abs().max())
    print("fresh %s %s reserved=%d: max|dz| = %.3g (bar %.3g), ls_iters %s" % ((n, d, k), line_search, reserved, dz, bar,
                                                                             got["ls_iters"]))
    assert res.flags == 0
    assert res.n_iter == i32["iterations"] and got["ls_iters"] == i32["ls_iters"]
    assert got["pairs"] == i32["pairs"] and got["skipped"] == i32["skipped"]
    assert dz <= bar
    f64 = i64["objective"][-1]
    assert abs(res.f_final - f64) / f64 <= max(1e-6, 4.0 * abs(i32["objective"][-1] - f64) / f64)
    assert abs(res.f_final - model.objective64(w, x, z, 0.1)) <= 1e-6 * f64      # no padding lane's log 2 in the sum
    record_margins("owlqn_glm/fresh_%dx%dx%d_%s_r%d" % (n, d, k, line_search, reserved), dict(dz=dz, bar=bar, gap=gap))


@pytest.mark.parametrize("line_search", ["brent", "backtrack", "none"])
def test_two_identical_calls_are_bitwise_equal(line_search):
    x, w = recipe(33, 48, 130, seed=3)
    z0 = torch.zeros(33, 130)
    kw = dict(alpha=0.1, line_search=line_search, max_iter=5, history_size=2, lr=0.05 if line_search == "none" else 1)
    a = run(w, x, z0, **kw)
    b = run(w, x, z0, **kw)
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    assert a[1]["iterations"] == 5 and a[1]["pairs"][-1] == 2
    assert set(a[1]) == {"iterations", "t", "ls_iters", "objective", "delta_x", "evaluations", "pairs", "skipped", "H_diag"}


def test_pitched_and_offset_operands_through_the_c_abi():
    n, d, k = 37, 50, 30
    x, w = recipe(n, d, k, seed=21)
    z0 = torch.zeros(n, k)
    z32, i32, _, _, gap = model_pair(w, x, z0, 0.1, line_search="none", lr=0.05, max_iter=4, history_size=2)
    z, res, got, bufs, _ = abi_solve(w, x, z0, 0.1, "none", 4, lr=0.05, history_size=2, pitches=(d + 3, k + 1, k + 5, k + 7))
    assert got["ls_iters"] == i32["ls_iters"] and got["pairs"] == i32["pairs"]
    assert float((z - z32).abs().max()) <= max(5e-5, 4.0 * gap)
    for key, (buf, src, ld) in bufs.items():                  # inputs and every padding word are as they were
        rows = n if key != "w" else d
        cols = d if key == "x" else k
        host = buf.cpu()
        body = host[1:1 + rows * ld].view(rows, ld)
        if src is not None:
            assert torch.equal(body[:, :cols], src), key
            assert (body[:, cols:] == 777.0).all() and host[0] == 777.0 and (host[1 + rows * ld:] == 777.0).all(), key
        else:
            assert (body[:, cols:] == -555.0).all() and host[0] == -555.0 and (host[1 + rows * ld:] == -555.0).all(), key


@pytest.mark.parametrize("family", [0, 2])
def test_an_unknown_family_is_unsupported(family):
    from lasso_amd import _native as nat
    x, w = recipe(5, 7, 19, seed=0)
    z, res, _, bufs, status = abi_solve(w, x, torch.zeros(5, 19), 0.1, "none", 2, family=family, check=False)
    assert status == nat.LASSO_ERR_UNSUPPORTED and "family" in nat.lib().lasso_hip_last_error().decode()
    assert (bufs["z"][0].cpu() == -555.0).all()                                    # nothing was written


# ---- the scratch and stream contract (tests/ws_poison.py, the harness of tests/test_workspace_gpu.py) ----
# one Brent iteration; a backtracking and a fixed step with a memory that overflows, over several segments; k beyond 4096;
# a saturated start
WS_NAMES = ("brent_ragged", "bt_mid", "none_tall", "bt_wide", "sat_bt")
_WS_CASES, _WS_ANCHORS = {}, {}


def _ws_case(cases, name):
    if name not in _WS_CASES:
        spec, g = CASES[name], load_case(cases, name)
        x, w, z0 = case_inputs(spec)
        assert spec["compare"] == "z" and admitted_z(g)

        def call(ops):
            from lasso_amd.nonlinear import bernoulli, owlqn
            with wsg._quiet() as said:
                z, report = owlqn(bernoulli(ops["x"], ops["w"]), ops["z0"], alpha=spec["alpha"], return_info=True,
                                  **spec["kwargs"])
            return dict(z=z), dict(report=report, said=said)

        def verify(out, host):
            bar = max(5e-5, 4.0 * float(g["spread_z"]))
            dz = float((out["z"] - torch.from_numpy(g["z32"])).abs().max())
            assert torch.isfinite(out["z"]).all() and bar <= 1e-2 and dz <= bar, (dz, bar)
            return dict(dz=dz, bar=bar)
        _WS_CASES[name] = wsg.Case(dict(x=x, w=w, z0=z0), call, verify, "lasso_owlqn_glm_solve")
    return _WS_CASES[name]


def _ws_anchor(cases, name):
    if name not in _WS_ANCHORS:
        _WS_ANCHORS[name] = wsg._run(_ws_case(cases, name), "zero")
    return _WS_ANCHORS[name]


@pytest.mark.parametrize("name", WS_NAMES)
def test_workspace_anchor_meets_the_recorded_run(cases, name):
    margins = _ws_case(cases, name).verify(*_ws_anchor(cases, name))
    record_margins("owlqn_glm/workspace_" + name, margins)


@pytest.mark.parametrize("mode", ["ones", "fives", "roomy", "stream"])
@pytest.mark.parametrize("name", WS_NAMES)
def test_same_bits_whatever_the_scratch_held(cases, name, mode):
    case, want = _ws_case(cases, name), _ws_anchor(cases, name)
    got = wsg._run_late(case.call, case.operands) if mode == "stream" else wsg._run(case, mode)
    bad = wsg._differences(got, want)
    assert not bad, "%s on %s differs from the anchor: %s" % (
        name, "a late side stream" if mode == "stream" else "scratch of mode '%s'" % mode, "; ".join(bad))
    assert torch.isfinite(got[0]["z"]).all()


# ---- NaN and Inf operand VALUES inside valid buffers: nothing here is meant to fault or hang.  No index or trip count of
# csrc/owlqn.hip derives from a floating value; the Brent search is capped at 500 evaluations and the ladder at ls_maxiter
# trials, and both end at the first non-finite objective.  The model says what comes back: its objective of such a start
# is not finite, so the solve ends before its first iteration with z0 as it came.
@pytest.mark.parametrize("line_search", ["brent", "backtrack", "none"])
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("where", ["x", "w", "z0"])
def test_a_poison_from_the_start_returns_z0(where, poison, line_search):
    n, d, k = 33, 48, 130
    x, w = recipe(n, d, k, seed=2)
    z0 = 0.1 * torch.randn(n, k, generator=torch.Generator().manual_seed(3)) * (torch.arange(k) % 3 == 0)
    {"x": x, "w": w, "z0": z0}[where][7, 5] = poison                     # one element of one row
    assert not np.isfinite(float(model.Model(w, x, 0.1).evaluate(z0)[0]))
    assert not np.isfinite(float(model.Model(w, x, 0.1, accurate_f=True, link64=True).evaluate(z0)[0]))
    z, info, said, _ = run(w, x, z0, alpha=0.1, line_search=line_search, max_iter=4, history_size=2, lr=0.05)
    assert said == [NONFINITE]
    assert info["iterations"] == 0 and info["objective"] == [] and info["evaluations"] == []
    assert torch.equal(z.view(torch.int32), z0.view(torch.int32))          # z0 as it came, its poison included


def test_the_clean_batch_is_untouched_by_the_checks_above():
    x, w = recipe(33, 48, 130, seed=2)
    z, info, said, _ = run(w, x, torch.zeros(33, 130), alpha=0.1, line_search="none", max_iter=4, history_size=2, lr=0.05)
    assert said == [] and info["iterations"] == 4 and torch.isfinite(z).all()


def test_logits_beyond_the_range_of_exp_stay_finite():
    """logits of +-1000: exp(|u|) is inf in float32 and in the naive float64 formula's float32 twin; the loss is
    max(u, 0) - x u to the last bit and the residual {0, 1} - x"""
    n, d, k = 9, 20, 12
    x, w = recipe(n, d, k, seed=5)
    z0 = warm_start(n, k, 5)
    z0 = z0 * (1000.0 / float((z0 @ w.T).abs().max()))
    z, res, got, _, _ = abi_solve(w, x, z0, 0.1, "none", 1, lr=1e-3)
    want = model.objective64(w, x, z0, 0.1)
    assert res.flags == 0 and np.isfinite(res.f0) and abs(res.f0 - want) <= 1e-6 * want
    assert torch.isfinite(z).all() and np.isfinite(res.f_final)
    assert abs(res.f_final - model.objective64(w, x, z, 0.1)) <= 1e-6 * res.f_final


def test_edges_no_rows_cpu_tensors_and_grad_inputs():
    from lasso_amd.nonlinear import bernoulli, owlqn
    x, w = recipe(33, 40, 24, seed=1)
    z0 = torch.randn(33, 24, generator=torch.Generator().manual_seed(5))
    z = owlqn(bernoulli(x[:0].cuda(), w.cuda()), z0[:0].cuda())
    assert z.shape == (0, 24) and z.is_cuda
    z, info, _, _ = run(w, x, z0, alpha=0.3, max_iter=0)
    assert torch.equal(z, z0) and info["iterations"] == 0
    # CPU tensors are staged; the result comes back on the device of x0
    zc = owlqn(bernoulli(x, w), torch.zeros(33, 24), alpha=0.3, line_search="none", max_iter=2, lr=0.05)
    assert zc.device.type == "cpu"
    zd = owlqn(bernoulli(x.cuda(), w.cuda()), torch.zeros(33, 24).cuda(), alpha=0.3, line_search="none", max_iter=2, lr=0.05)
    assert torch.equal(zd.cpu(), zc)
    # requires_grad inputs are accepted; the result carries no graph
    zg = owlqn(bernoulli(x.cuda(), w.cuda().requires_grad_()), torch.zeros(33, 24).cuda().requires_grad_(), alpha=0.3,
               line_search="none", max_iter=1)
    assert not zg.requires_grad
