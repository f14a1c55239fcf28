"""owlqn on the GPU against the reference's recorded runs (tests/golden/owlqn_cases.npz) and the host model
(tests/owlqn_model.py).

Bars.  Codes: max|z - z_ref32| <= max(5e-5, 4 x spread_z), where spread_z is how far "another correct float32
implementation" (the model with permuted summation orders, the vector-free direction and either objective fold) moved
the codes when the fixture was made; the factor 4 and the 5e-5 floor are the project's rule (tests/test_own_gpu.py).  A
case is compared by its codes only if spread_z <= 2.5e-3, so the bar never exceeds 1e-2.  Several Brent iterations and
a dozen backtracking ones are compared by objective only, max(1e-6, 4 x spread_f) against the float64 run
(tests/owlqn_cases.py says why).  Fresh shapes take 4 x the model's float32 / float64 gap instead, after asserting that
no decision of the model -- backtracking or y.s against 1e-10 -- is close enough to its threshold for rounding to flip it."""
import contextlib
import ctypes as C
import io
import re
import warnings

import numpy as np
import pytest
import torch

import owlqn_model
from margins import record_margins
from owlqn_cases import CASES, admitted_f, admitted_z, case_inputs, load_case, recipe, rtol_of

pytestmark = pytest.mark.gpu
MODES = {"brent": 0, "backtrack": 1, "none": 2}


@pytest.fixture(scope="module")
def cases(golden):
    return golden("owlqn_cases")


def run(w, x, z0, **kw):
    """-> (z on the CPU, info, warnings, printed text); inputs go to the GPU and must come back bitwise unchanged"""
    from lasso_amd.nonlinear import owlqn, rss
    wg, xg, zg = w.cuda(), x.cuda(), z0.cuda()
    out = io.StringIO()
    with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(out):
        warnings.simplefilter("always")
        z, info = owlqn(rss(xg, wg), zg, return_info=True, **kw)
    assert z.is_cuda and z.dtype == x.dtype and z.data_ptr() != zg.data_ptr()
    assert torch.equal(wg.cpu(), w) and torch.equal(xg.cpu(), x) and torch.equal(zg.cpu(), z0)
    return z.cpu(), info, [str(c.message) for c in caught], out.getvalue()


def same_line(a, b, rtol):
    """the same text, integers equal, and every printed number within rtol (the bar of the record it prints) or one unit
    of its last printed digit"""
    num = r"[-+]?\d+\.\d+e[-+]\d+|[-+]?\d+\.\d+|[-+]?\d+"
    if re.sub(num, "#", a) != re.sub(num, "#", b):
        return False
    for u, v in zip(re.findall(num, a), re.findall(num, b)):
        if "." not in v:
            if u != v:
                return False
            continue
        mantissa, _, exponent = v.partition("e")
        unit = 10.0 ** (int(exponent or 0) - len(mantissa.split(".")[1]))
        if abs(float(u) - float(v)) > rtol * abs(float(v)) + 1.001 * unit:
            return False
    return True


def pitched(t, ld, fill=777.0):
    """a device copy of t [rows, cols] with row pitch ld, 4 bytes off a 16-byte boundary -> (view, buffer)"""
    rows, cols = t.shape
    buf = torch.full((rows * ld + 5,), fill, dtype=torch.float32, device="cuda")
    view = buf[1:1 + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view, buf


def abi_solve(w, x, z0, alpha, line_search, max_iter, lr=1.0, xtol=1e-5, history_size=100, ls_options=None, reserved=0,
              pitches=None):
    """lasso_owlqn_solve directly: `reserved` and pitched / offset operands are not reachable from Python.
    pitches = (ldx, ldw, ldz0, ldz) or None (packed) -> (z on the CPU, result struct, trace lists, the buffers)"""
    from lasso_amd import _native as nat
    n, d = x.shape
    k = w.shape[1]
    ls = dict(owlqn_model.LS_DEFAULTS, **(ls_options or {}))
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
    nat.check(L.lasso_owlqn_solve(C.c_void_p(xv.data_ptr()), ldx, C.c_void_p(wv.data_ptr()), ldw, C.c_void_p(z0v.data_ptr()),
                                  ldz0, C.c_void_p(zv.data_ptr()), ldz, n, d, k, nat.LASSO_F32, alpha, C.byref(opts),
                                  C.byref(res), nat.ptr(ws), ws.numel(), nat.stream_ptr(torch.device("cuda", 0))))
    torch.cuda.synchronize()
    its = res.n_iter
    lists = dict(ls_iters=list(ls_arr[:its]), pairs=list(p_arr[:its]), skipped=[bool(v) for v in s_arr[:its]],
                 objective=list(f_arr[:its]))
    return zv.cpu(), res, lists, dict(x=(xb, x, ldx), w=(wb, w, ldw), z0=(z0b, z0, ldz0), z=(zb, None, ldz))


def model_pair(w, x, z0, alpha, **kw):
    """the model in float32 and float64 -> (z32, info32, z64, info64, gap); asserts its decisions are robust"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z32, i32 = owlqn_model.owlqn(w, x, z0, alpha=alpha, **kw)
        z64, i64 = owlqn_model.owlqn(w, x, z0, alpha=alpha, dtype=torch.float64, **kw)
    for info in (i32, i64):
        owlqn_model.assert_robust(info)
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
    assert sorted(caught) == sorted(m for m in str(g["warnings"]).split("\n") if m)
    assert info["iterations"] == len(g["f32"])
    # the memory held and dropped what the reference's did
    assert info["pairs"] == list(g["pairs"]) and [int(s) for s in info["skipped"]] == list(g["skipped"])
    f_z = owlqn_model.objective64(w, x, z, spec["alpha"])
    f_last = info["objective"][-1] if info["objective"] else float(text.split("\n")[0].split(":")[1])
    print("%s: reported objective %.9g, objective of z %.9g" % (name, f_last, f_z))
    assert abs(f_last - f_z) <= (1e-6 if info["objective"] else 1e-4) * f_z     # ('initial f: %0.4f' is all max_iter = 0 says)
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
        if brent or kw["line_search"] == "backtrack":                  # (a fixed step promises no descent)
            assert all(b <= a * (1 + 1e-6) for a, b in zip(objs, objs[1:])), objs
        if spec["compare"] == "f":
            assert admitted_f(g)
        if admitted_f(g):
            assert err <= bar, (name, err, bar)
        margins = dict(objective_rel=err, bar=bar, admitted=bool(admitted_f(g)))
    record_margins("owlqn/" + name, margins)


@pytest.mark.parametrize("name", ["brent_small", "brent_ragged"])
def test_brent_evaluations_are_the_line_objective(cases, name):
    spec = CASES[name]
    x, w, z0 = case_inputs(spec)
    z, info, _, _ = run(w, x, z0, alpha=spec["alpha"], **spec["kwargs"])
    evals = info["evaluations"]
    assert len(evals) == info["ls_iters"][0] and 5 <= len(evals) <= 60 and all(e[0] == 1 for e in evals)
    assert all(0.0 < e[1] < 10.0 for e in evals)
    line64 = owlqn_model.first_line_objective(w, x, z0, spec["alpha"], torch.float64)
    line32 = owlqn_model.first_line_objective(w, x, z0, spec["alpha"], torch.float32, accurate_f=False)
    want = np.array([line64(float(np.float32(t))) for _, t, _ in evals])      # (the step is applied as a float32)
    gap = float(np.max(np.abs(np.array([line32(float(np.float32(t))) for _, t, _ in evals]) - want) / want))
    rtol = max(1e-6, 4.0 * gap)
    err = float(np.max(np.abs(np.array([f for _, _, f in evals]) - want) / want))
    print("%s: %d evaluations, rel %.3g (rtol %.3g, model gap %.3g)" % (name, len(evals), err, rtol, gap))
    assert err <= rtol
    # the accepted t is the best abscissa the search saw
    best = min(reversed(evals), key=lambda e: e[2])          # (a tie goes to the later evaluation)
    assert info["t"][0] == best[1]
    record_margins("owlqn/evaluations_" + name, dict(rel=err, rtol=rtol, count=len(evals)))


# (n, d, k, reserved, seed, line_search): an odd everything, 128-blocks forced, d and k multiples of 32 (the LDS-DMA operand
# form) with more than one segment and a ragged one, k beyond 4096.  Backtracking from t = 1 is compared on the shapes where
# it is not chaotic: on the larger ones "another correct implementation" (the model with an order_seed) already ends 1e-2
# from the model after three iterations while its float32 / float64 gap stays at 1e-4, so that gap is no bar there; the
# recorded cases bt_ragged, bt_ladder and bt_12 cover backtracking over several segments with a measured spread.
FRESH = [(37, 50, 30, 0, 22, "none"), (37, 50, 30, 1, 22, "none"), (40, 64, 320, 0, 22, "none"), (40, 64, 320, 1, 22, "none"),
         (96, 64, 96, 0, 22, "none"), (130, 24, 100, 0, 23, "none"), (3, 12, 4101, 0, 22, "none"),
         (37, 50, 30, 0, 22, "backtrack"), (37, 50, 30, 1, 22, "backtrack"), (3, 12, 4101, 0, 22, "backtrack")]


@pytest.mark.parametrize("n,d,k,reserved,seed,line_search", FRESH)
def test_fresh_shape_against_the_model(n, d, k, reserved, seed, line_search):
    x, w = recipe(n, d, k, seed=seed)
    z0 = torch.zeros(n, k)
    kw = dict(line_search=line_search, max_iter=4, history_size=2, lr=1.0 if line_search == "backtrack" else 0.05)
    z32, i32, z64, i64, gap = model_pair(w, x, z0, 0.1, **kw)
    bar = max(5e-5, 4.0 * gap)
    z, res, got, _ = abi_solve(w, x, z0, 0.1, line_search, 4, lr=kw["lr"], history_size=2, reserved=reserved)
    dz = float((z - z32).abs().max())
    print("fresh %s %s reserved=%d: max|dz| = %.3g (bar %.3g), ls_iters %s" % ((n, d, k), line_search, reserved, dz, bar,
                                                                             got["ls_iters"]))
    assert res.n_iter == i32["iterations"] and got["ls_iters"] == i32["ls_iters"]
    assert got["pairs"] == i32["pairs"] and got["skipped"] == i32["skipped"]
    assert dz <= bar
    f64 = i64["objective"][-1]
    assert abs(res.f_final - f64) / f64 <= max(1e-6, 4.0 * abs(i32["objective"][-1] - f64) / f64)
    record_margins("owlqn/fresh_%dx%dx%d_%s_r%d" % (n, d, k, line_search, reserved), dict(dz=dz, bar=bar, gap=gap))


@pytest.mark.parametrize("line_search", ["brent", "backtrack", "none"])
def test_two_identical_calls_are_bitwise_equal(line_search):
    x, w = recipe(33, 48, 130, seed=3)
    z0 = torch.zeros(33, 130)
    kw = dict(alpha=0.1, line_search=line_search, max_iter=5, history_size=2, lr=0.05 if line_search == "none" else 1)
    a = run(w, x, z0, **kw)
    b = run(w, x, z0, **kw)
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    assert a[1]["iterations"] == 5 and a[1]["pairs"][-1] == 2


def test_info_is_consistent_with_the_model():
    """pairs / skipped / H_diag are the model's, and the reported objective is the objective of z"""
    n, d, k = 33, 48, 130
    x, w = recipe(n, d, k, seed=4)
    z0 = torch.zeros(n, k)
    kw = dict(line_search="none", lr=0.05, max_iter=6, history_size=3)
    z32, i32, _, i64, gap = model_pair(w, x, z0, 0.1, **kw)
    z, info, _, _ = run(w, x, z0, alpha=0.1, **kw)
    assert info["pairs"] == i32["pairs"] == [1, 2, 3, 3, 3, 3] and info["skipped"] == i32["skipped"]
    assert abs(info["objective"][-1] - owlqn_model.objective64(w, x, z, 0.1)) <= 1e-6 * info["objective"][-1]
    h_rel = max(abs(a - b) / b for a, b in zip(info["H_diag"], i64["H_diag"]))
    h_gap = max(abs(a - b) / b for a, b in zip(i32["H_diag"], i64["H_diag"]))
    print("H_diag rel %.3g (model float32 / float64 gap %.3g)" % (h_rel, h_gap))
    assert h_rel <= max(1e-5, 4.0 * h_gap)
    assert float((z - z32).abs().max()) <= max(5e-5, 4.0 * gap)
    assert set(info) == {"iterations", "t", "ls_iters", "objective", "delta_x", "evaluations", "pairs", "skipped", "H_diag"}


def test_pitched_and_offset_operands_through_the_c_abi():
    n, d, k = 37, 50, 30
    x, w = recipe(n, d, k, seed=21)
    z0 = torch.zeros(n, k)
    z32, i32, _, _, gap = model_pair(w, x, z0, 0.1, line_search="backtrack", max_iter=4, history_size=2)
    z, res, got, bufs = abi_solve(w, x, z0, 0.1, "backtrack", 4, history_size=2, pitches=(d + 3, k + 1, k + 5, k + 7))
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


def test_edges_no_rows_cpu_tensors_and_grad_inputs():
    from lasso_amd.nonlinear import owlqn, rss
    x, w = recipe(33, 40, 24, seed=1)
    z0 = torch.randn(33, 24, generator=torch.Generator().manual_seed(5))
    z = owlqn(rss(x[:0].cuda(), w.cuda()), z0[:0].cuda())
    assert z.shape == (0, 24) and z.is_cuda
    z, info, _, _ = run(w, x, z0, alpha=0.3, max_iter=0)
    assert torch.equal(z, z0) and info["iterations"] == 0
    # CPU tensors are staged; the result comes back on the device of x0
    zc = owlqn(rss(x, w), torch.zeros(33, 24), alpha=0.3, line_search="none", max_iter=2, lr=0.05)
    assert zc.device.type == "cpu"
    # requires_grad inputs are accepted; the result carries no graph
    zg = owlqn(rss(x.cuda(), w.cuda().requires_grad_()), torch.zeros(33, 24).cuda().requires_grad_(), alpha=0.3,
               line_search="none", max_iter=1)
    assert not zg.requires_grad
