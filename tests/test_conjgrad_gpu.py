"""lasso_amd.conjgrad on the GPU against the reference's recorded runs (tests/golden/conjgrad_cases.npz) and the host
model (tests/conjgrad_model.py).

Bars.  x: max|x - x_ref32| <= max(5e-5, 4 x spread_x), where spread_x is how far "another correct implementation" (the
model with permuted summation orders and with sums folded in double) moved x when the fixture was made; the factor 4
and the 5e-5 floor are the project's rule (bar_z of tests/split_bregman_cases.py).  A case is admitted only with
spread_x <= 2.5e-3.  float64 cases take the same rule with the double spread and a floor of 1e-12.  The three recorded
sequences (sum|r|, curv_sum, sqrt(sum rs)): relative max(1e-5, 4 x spread_seq).  status and iterations are equal to the
fixture's: the generator refused every case with a sum within 1 % of its threshold.  Fresh shapes take the same rule with
the spread measured here, from the same variants of the model."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import conjgrad_model as model
from conjgrad_cases import (CONV, DENSE, ORDER_SEEDS, VERBOSE_CASE, bar_x, conv_inputs, conv_kwargs, dense_inputs,
                            load_case, rel, rtol_seq)
from layouts import SENTINEL, place, plans
from margins import record_margins

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(golden):
    return golden("conjgrad_cases")


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def run(fn, *tensors, **kw):
    """-> (x on the CPU, info, printed text); the tensors go to the GPU and must come back bitwise unchanged"""
    dev = [t.cuda() for t in tensors]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        x, info = fn(*dev, return_info=True, **kw)
    assert x.is_cuda and x.dtype == tensors[1].dtype and x.shape == tensors[1].shape
    assert x.data_ptr() not in [t.data_ptr() for t in dev]
    for d, h in zip(dev, tensors):                                # (bit for bit: an operand may hold a NaN)
        assert torch.equal(bits(d.cpu()), bits(h))
    return x.cpu(), info, out.getvalue()


def seq_rel(info, g):
    return max(rel(info["r_abs"], g["r_abs"]), rel(info["curv_sum"], g["curv_sum"]), rel(info["rs"], g["rs"]))


def check_golden(name, g, x, info, want_key="x32", floor=5e-5, tag=""):
    dx = float((x.double() - torch.from_numpy(g[want_key]).double()).abs().max())
    bar, rs, rtol = bar_x(g, floor), seq_rel(info, g), rtol_seq(g)
    print("%s%s: max|dx| = %.3g (bar %.3g), sequences rel %.3g (rtol %.3g), status %d at %d, %d host reads, %s"
          % (name, tag, dx, bar, rs, rtol, info["status"], info["iterations"], info["host_reads"], info["form"]))
    record_margins("conjgrad/" + name + tag, dict(dx=dx, bar=bar, seq_rel=rs, seq_rtol=rtol, status=info["status"],
                                                  iterations=info["iterations"], host_reads=info["host_reads"]))
    assert info["status"] == int(g["status"]) and info["iterations"] == int(g["iterations"])
    assert abs(info["termcond"] - float(g["termcond"])) <= rtol * abs(float(g["termcond"]))
    assert bar <= 1e-2
    assert dx <= bar, (name, dx, bar)
    assert rs <= rtol, (name, rs, rtol)


@pytest.mark.parametrize("name", sorted(n for n, s in DENSE.items() if not s.get("f64_only")))
def test_dense_golden_case(cases, name):
    from lasso_amd.conjgrad import batch_cg, cg
    spec, g = DENSE[name], load_case(cases, name)
    A, b = dense_inputs(spec)
    x, info, text = run(cg if spec.get("vector") else batch_cg, A, b, **spec["kwargs"])
    assert text == "" and info["form"] == "fused"
    check_golden(name, g, x, info)


@pytest.mark.parametrize("name", ["n37_k70_rtol1em4", "n130_k129_rtol1em4", "n16_k1030_rtol1em4", "n3_k1_rtol1"])
def test_dense_plain_form_through_the_abi(cases, name):
    """bit 0 of reserved: the product stores Ap and a pass of its own takes curv"""
    spec, g = DENSE[name], load_case(cases, name)
    A, b = dense_inputs(spec)
    x, res, info, _ = abi_dense(A, b, reserved=1, **spec["kwargs"])
    assert info["form"] == "unfused"
    check_golden(name, g, x, info, tag="_plain")


@pytest.mark.parametrize("name", sorted(n for n, s in DENSE.items() if s.get("f64_only")))
def test_dense_float64_golden_case(cases, name):
    from lasso_amd.conjgrad import batch_cg
    spec, g = DENSE[name], load_case(cases, name)
    A, b = dense_inputs(spec, torch.float64)
    x, info, _ = run(batch_cg, A, b, **spec["kwargs"])
    assert x.dtype == torch.float64
    check_golden(name, g, x, info, want_key="x64", floor=1e-12)


def test_float64_runs_of_the_float32_cases_stay_within_their_distance(cases):
    """the float32 cases in double: the same exit, and x as far from the float32 reference as the double reference was"""
    from lasso_amd.conjgrad import batch_cg
    for name in ("n37_k70_rtol1em4", "n130_k129_rtol1", "n40_k257_rtol1em4"):
        spec, g = DENSE[name], load_case(cases, name)
        A, b = dense_inputs(spec, torch.float64)
        x, info, _ = run(batch_cg, A, b, **spec["kwargs"])
        dx = float((x - torch.from_numpy(g["x32"]).double()).abs().max())
        print("%s in double: max|x - x_ref32| = %.3g (the double reference: %.3g)" % (name, dx, float(g["gap_x"])))
        assert info["status"] == int(g["status"]) and info["iterations"] == int(g["iterations"])
        assert dx <= float(g["gap_x"]) + 1e-9


@pytest.mark.parametrize("name", sorted(CONV))
def test_conv_golden_case(cases, name):
    from lasso_amd.conjgrad import batch_cg_conv2d
    spec, g = CONV[name], load_case(cases, name)
    kernel, b = conv_inputs(spec)
    x, info, text = run(batch_cg_conv2d, kernel, b, tik=spec["tik"], **spec["kwargs"], **conv_kwargs(spec))
    assert text == ""
    # the forms the implementation dispatches, each reached by a named case
    assert info["form"] == ("conv-implicit" if name.startswith("grey") else "conv-patches")
    check_golden(name, g, x, info)


@pytest.mark.parametrize("name", ["grey_tik0p5", "grey_tik0"])
def test_conv_plain_form_where_an_implicit_kernel_covers(cases, name):
    import lasso_amd.conjgrad as cgm
    spec, g = CONV[name], load_case(cases, name)
    kernel, b = conv_inputs(spec)
    cgm._FORCE_PLAIN[0] = True
    try:
        x, info, _ = run(cgm.batch_cg_conv2d, kernel, b, tik=spec["tik"], **spec["kwargs"], **conv_kwargs(spec))
    finally:
        cgm._FORCE_PLAIN[0] = False
    assert info["form"] == "conv-patches"
    check_golden(name, g, x, info, tag="_plain")


# shapes the fixture does not hold: the 16-byte-load operand form (k % 4 == 0, k % 32 != 0), the LDS-DMA form
# (k % 32 == 0), scalar loads (k odd), more than one block of rows; a group longer than a wave owns (k > 2048)
FRESH = [(130, 96), (70, 68), (131, 31), (9, 2100)]


def spread_against(run_model, x, info):
    sx, ss = 0.0, 0.0
    for knobs in model.variants(ORDER_SEEDS):
        xm, im = run_model(**knobs)
        assert (im["status"], im["iterations"]) == (info["status"], info["iterations"])
        sx = max(sx, float((xm - x).abs().max()))
        ss = max(ss, rel(im["r_abs"], info["r_abs"]), rel(im["curv_sum"], info["curv_sum"]), rel(im["rs"], info["rs"]))
    return max(5e-5, 4.0 * sx), max(1e-5, 4.0 * ss)


@pytest.mark.parametrize("n,k", FRESH)
def test_fresh_shape_against_the_model(n, k):
    from lasso_amd.conjgrad import batch_cg
    spec = dict(n=n, k=k, d=max(4, k // 4), seed=40)
    A, b = dense_inputs(spec)
    kw = dict(maxiter=6, rtol=0.0, tol=0.0)
    xm, im = model.batch_cg(A, b, **kw)
    bar, rtol = spread_against(lambda **knobs: model.batch_cg(A, b, **kw, **knobs), xm, im)
    x, info, _ = run(batch_cg, A, b, **kw)
    dx, rs = float((x - xm).abs().max()), seq_rel(info, im)
    print("fresh %s: max|dx| = %.3g (bar %.3g), sequences rel %.3g (rtol %.3g)" % ((n, k), dx, bar, rs, rtol))
    record_margins("conjgrad/fresh_%dx%d" % (n, k), dict(dx=dx, bar=bar, seq_rel=rs, seq_rtol=rtol))
    assert info["status"] == 4 and info["iterations"] == 6 and len(info["rs"]) == 6
    assert dx <= bar and rs <= rtol


def test_fresh_conv_shape_against_the_model():
    """an image longer than a wave owns (K Hz Wz > 2048), two images"""
    from lasso_amd.conjgrad import batch_cg_conv2d
    spec = dict(N=2, C=2, K=12, ks=(3, 3), H=16, W=17, stride=1, padding=1, seed=41)
    kernel, b = conv_inputs(spec)
    kw = dict(tik=0.25, maxiter=5, rtol=0.0, tol=0.0, **conv_kwargs(spec))
    xm, im = model.batch_cg_conv2d(kernel, b, **kw)
    bar, rtol = spread_against(lambda **knobs: model.batch_cg_conv2d(kernel, b, **kw, **knobs), xm, im)
    x, info, _ = run(batch_cg_conv2d, kernel, b, **kw)
    dx, rs = float((x - xm).abs().max()), seq_rel(info, im)
    print("fresh conv: max|dx| = %.3g (bar %.3g), sequences rel %.3g (rtol %.3g)" % (dx, bar, rs, rtol))
    record_margins("conjgrad/fresh_conv", dict(dx=dx, bar=bar, seq_rel=rs, seq_rtol=rtol))
    assert b[0].numel() > 2048 and info["status"] == 4 and info["iterations"] == 5
    assert dx <= bar and rs <= rtol


def test_two_identical_calls_are_bitwise_equal():
    from lasso_amd.conjgrad import batch_cg, batch_cg_conv2d
    A, b = dense_inputs(DENSE["n130_k129_rtol1em4"])
    a1, i1, _ = run(batch_cg, A, b, rtol=1e-4)
    a2, i2, _ = run(batch_cg, A, b, rtol=1e-4)
    assert torch.equal(bits(a1), bits(a2)) and i1 == i2
    spec = CONV["rgb_tik0p5"]
    kernel, bc = conv_inputs(spec)
    c1, j1, _ = run(batch_cg_conv2d, kernel, bc, tik=0.5, rtol=1e-2, **conv_kwargs(spec))
    c2, j2, _ = run(batch_cg_conv2d, kernel, bc, tik=0.5, rtol=1e-2, **conv_kwargs(spec))
    assert torch.equal(bits(c1), bits(c2)) and j1 == j2


def test_cpu_tensors_in_cpu_tensors_out():
    from lasso_amd.conjgrad import batch_cg, batch_cg_conv2d, cg
    A, b = dense_inputs(DENSE["n8_k10_rtol1"])
    x = batch_cg(A, b)
    xg = batch_cg(A.cuda(), b.cuda())
    assert x.device.type == "cpu" and xg.is_cuda and torch.equal(x, xg.cpu())
    v = cg(A, b[0], rtol=1e-4)
    assert v.shape == (10,) and v.device.type == "cpu"
    assert torch.equal(v, batch_cg(A, b[:1], rtol=1e-4, maxiter=200)[0])         # cg is the n = 1 batch
    spec = CONV["rgb_tik0p5"]
    kernel, bc = conv_inputs(spec)
    z = batch_cg_conv2d(kernel, bc, 0.5, **conv_kwargs(spec))
    assert z.device.type == "cpu" and z.shape == bc.shape
    e = batch_cg(A.cuda(), b[:0].cuda())
    assert e.shape == (0, 10) and e.is_cuda


def test_exits_on_zero_and_on_negative_curvature():
    from lasso_amd.conjgrad import batch_cg
    g = torch.Generator().manual_seed(5)
    A = torch.eye(12) * 2.0
    x, info, _ = run(batch_cg, A, torch.zeros(5, 12))
    assert torch.equal(x, torch.zeros(5, 12)) and info["status"] == 1 and info["iterations"] == 0
    assert info["r_abs"] == [0.0] and info["curv_sum"] == [] and info["rs"] == [] and info["termcond"] == 0.0
    b = torch.randn(5, 12, generator=g)
    x, info, _ = run(batch_cg, -torch.eye(12), b)
    assert info["status"] == 3 and info["iterations"] == 0 and len(info["curv_sum"]) == 1 and info["rs"] == []
    assert info["curv_sum"][0] < 0
    xm, im = model.batch_cg(-torch.eye(12), b)
    assert im["status"] == 3 and float((x - xm).abs().max()) <= 1e-6 and float((x - b).abs().max()) <= 1e-6
    # negative curvature later than iteration 0 leaves x where it was
    A = torch.diag(torch.tensor([1.0] * 11 + [-2.0]))
    A[0, 1] = A[1, 0] = 0.3
    A[2, 5] = A[5, 2] = -0.4
    xm, im = model.batch_cg(A, b, rtol=0.0)                                      # curv_sum: 67.3, then -21.5
    x, info, _ = run(batch_cg, A, b, rtol=0.0)
    assert im["status"] == 3 and im["iterations"] > 0
    assert (info["status"], info["iterations"]) == (im["status"], im["iterations"])
    assert float((x - xm).abs().max()) <= 5e-5 * max(1.0, float(xm.abs().max()))
    # maxiter = 0: nothing runs
    x, info, _ = run(batch_cg, torch.eye(12), b, maxiter=0)
    assert torch.equal(x, torch.zeros(5, 12)) and info["status"] == 4 and info["iterations"] == 0


def test_verbose_2_prints_the_fixtures_text(cases):
    from lasso_amd.conjgrad import batch_cg
    spec = DENSE[VERBOSE_CASE]
    A, b = dense_inputs(spec)
    want = str(cases["verbose2_text"])
    x, info, text = run(batch_cg, A, b, verbose=2, **spec["kwargs"])
    xq, _, textq = run(batch_cg, A, b, **spec["kwargs"])
    assert torch.equal(x, xq) and textq == ""
    assert want.endswith("Relative tolerance reached.\n") and want.count("\n") == info["iterations"] + 1
    assert text == want
    _, _, text1 = run(batch_cg, A, b, verbose=True, **spec["kwargs"])
    assert text1 == "Relative tolerance reached.\n"


def test_nan_in_one_row_is_an_ordinary_operand():
    from lasso_amd.conjgrad import batch_cg
    A, b = dense_inputs(DENSE["n37_k70_rtol1"])
    kw = dict(maxiter=5, rtol=0.0, tol=0.0)
    bad = b.clone()
    bad[5, 3] = float("nan")
    xc, ic, _ = run(batch_cg, A, b, **kw)
    x, info, _ = run(batch_cg, A, bad, **kw)
    assert info["status"] == 4 and info["iterations"] == 5 and ic["status"] == 4
    assert torch.isnan(x[5]).all() and all(np.isnan(v) for v in info["r_abs"])
    keep = torch.arange(37) != 5
    assert torch.equal(bits(x[keep]), bits(xc[keep]))
    # ... and with the default tolerances no exit fires either: maxiter iterations run
    x, info, _ = run(batch_cg, A, bad, maxiter=9)
    assert info["status"] == 4 and info["iterations"] == 9


def test_host_reads():
    from lasso_amd.conjgrad import batch_cg, batch_cg_conv2d
    A, b = dense_inputs(DENSE["n37_k70_rtol1"])
    x, info, _ = run(batch_cg, A, b, rtol=0.0, tol=0.0, maxiter=8)
    assert info["host_reads"] <= 1 and info["status"] == 4 and len(info["rs"]) == 8
    spec = CONV["rgb_tik0p5"]
    kernel, bc = conv_inputs(spec)
    z, info, _ = run(batch_cg_conv2d, kernel, bc, tik=0.5, rtol=0.0, tol=0.0, maxiter=8, **conv_kwargs(spec))
    assert info["host_reads"] <= 1 and info["status"] == 4
    # with exits that can fire: one read per chunk of iterations, not one per iteration
    x, info, _ = run(batch_cg, A, b, rtol=1e-4)
    assert info["iterations"] == 11 and info["host_reads"] <= 3


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def abi_dense(A, b, plan=None, reserved=0, maxiter=None, tol=1e-10, rtol=1.0, tik=0.0, ld_override=None, expect=None,
              short_workspace=0):
    """lasso_cg_solve directly: `reserved` and pitched / odd / offset operands are not reachable from Python.
    plan: {operand: layout} over a, b, x (tests/layouts.py); -> (x on the CPU, result struct, info, the placed operands)"""
    from lasso_amd import _native as nat
    import lasso_amd.conjgrad as cgm
    n, k = b.shape
    maxiter = 20 * k if maxiter is None else maxiter
    plan = plan or {}
    ops = dict(a=place(A, plan.get("a", "natural"), float("nan"), "cuda", "a"),
               b=place(b, plan.get("b", "natural"), float("nan"), "cuda", "b"),
               x=place(torch.zeros(n, k, dtype=b.dtype), plan.get("x", "natural"), SENTINEL, "cuda", "x", fill=SENTINEL))
    ld = {name: p.ld for name, p in ops.items()}
    ld.update(ld_override or {})
    options, res, traces, _trace = cgm._request(maxiter, tol, rtol, tik, True, False)
    options.reserved = reserved
    L = nat.lib()
    dt = nat.DT[b.dtype]
    ws = torch.empty(L.lasso_cg_workspace_bytes(n, k, dt) - short_workspace, dtype=torch.uint8, device="cuda")
    status = L.lasso_cg_solve(C.c_void_p(ops["a"].view.data_ptr()), ld["a"], C.c_void_p(ops["b"].view.data_ptr()), ld["b"],
                              C.c_void_p(ops["x"].view.data_ptr()), ld["x"], n, k, dt, C.byref(options), C.byref(res),
                              nat.ptr(ws), ws.numel(), nat.stream_ptr(torch.device("cuda", 0)))
    torch.cuda.synchronize()
    if expect is None:
        nat.check(status)
    else:
        assert status == expect, (status, expect)
        return ops["x"].view.cpu(), res, None, ops
    return ops["x"].view.cpu(), res, cgm._finish(res, traces, True), ops


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_layouts_through_the_c_abi(dtype):
    from lasso_amd import _native as nat
    A, b = dense_inputs(dict(n=37, k=64, d=24, seed=21), dtype)
    kw = dict(maxiter=4, rtol=0.0, tol=0.0)
    anchor = None
    for tag, plan in plans(("a", "b", "x")):
        x, res, info, ops = abi_dense(A, b, plan=plan, **kw)
        for name, p in ops.items():
            p.check(written=(name == "x"))                     # guard bands intact, inputs only read
        assert res.n_iter == 4 and res.status == 4 and torch.isfinite(x).all(), tag
        if anchor is None:
            anchor = (x, info)                                 # (what a solve is held to: the golden cases)
        else:
            assert torch.equal(bits(x), bits(anchor[0])) and info == anchor[1], tag
    # refusals with nothing written
    for bad in (dict(ld_override=dict(a=63)), dict(ld_override=dict(b=63)), dict(ld_override=dict(x=63)),
                dict(reserved=0x7f00), dict(reserved=2), dict(tik=0.5), dict(rtol=-1.0), dict(maxiter=-1)):
        args = dict(kw)
        args.update(bad)
        x, res, _, ops = abi_dense(A, b, plan=dict(x="pitched"), expect=nat.LASSO_ERR_BAD_ARG, **args)
        assert (ops["x"].buffer == SENTINEL).all(), bad
        for name, p in ops.items():
            p.check(written=False)
    x, res, _, ops = abi_dense(A, b, expect=nat.LASSO_ERR_WORKSPACE, short_workspace=1, **kw)
    assert (ops["x"].buffer == SENTINEL).all()


def test_conv_abi_refusals():
    from lasso_amd import _native as nat
    import lasso_amd.conjgrad as cgm
    spec = CONV["rgb_tik0p5"]
    kernel, b = conv_inputs(spec)
    N, K, Hz, Wz = b.shape
    geom = (N, 3, 9, 9, K, Hz, Wz, 3, 3, 1, 1, 1, 1)
    L = nat.lib()
    need = L.lasso_conv_cg_workspace_bytes(*geom)
    assert need > 0
    wg, bg = kernel.cuda(), b.cuda()

    def call(reserved=0, short=0, dtype=nat.LASSO_F32, tik=0.5, geometry=geom):
        z = torch.full(b.shape, SENTINEL, device="cuda")
        options, res, _, _trace = cgm._request(3, 0.0, 0.0, tik, True, False)
        options.reserved = reserved
        ws = torch.empty(need - short, dtype=torch.uint8, device="cuda")
        status = L.lasso_conv_cg_solve(nat.ptr(wg), nat.ptr(bg), nat.ptr(z), *geometry, dtype, C.byref(options), C.byref(res),
                                       nat.ptr(ws), ws.numel(), nat.stream_ptr(torch.device("cuda", 0)))
        torch.cuda.synchronize()
        return status, z.cpu(), res

    status, z, res = call()
    assert status == nat.LASSO_OK and res.status == 4 and res.n_iter == 3 and torch.isfinite(z).all()
    for kw, want in ((dict(short=1), nat.LASSO_ERR_WORKSPACE), (dict(reserved=6), nat.LASSO_ERR_BAD_ARG),
                     (dict(tik=-1.0), nat.LASSO_ERR_BAD_ARG), (dict(dtype=nat.LASSO_F64), nat.LASSO_ERR_UNSUPPORTED),
                     (dict(geometry=(N, 3, 10, 9, K, Hz, Wz, 3, 3, 1, 1, 1, 1)), nat.LASSO_ERR_BAD_ARG)):
        status, z, _ = call(**kw)
        assert status == want and (z == SENTINEL).all(), kw


def test_ridge_code_satisfies_the_normal_equations():
    """batch_cg_conv2d(w, conv2d(x, w), tik) at rtol = 1e-6: |Adot(z) - b|_inf, formed with torch.nn.functional on the
    CPU, stays below 4 x the same quantity for the model's result"""
    from lasso_amd.conjgrad import batch_cg_conv2d
    for name in ("grey_tik0p5", "rgb_tik0p5", "stride2_tik0p5"):
        spec = CONV[name]
        kernel, b = conv_inputs(spec)
        ck = conv_kwargs(spec)
        z, info, _ = run(batch_cg_conv2d, kernel, b, tik=0.5, rtol=1e-6, **ck)
        zm, im = model.batch_cg_conv2d(kernel, b, tik=0.5, rtol=1e-6, **ck)

        def resid(v):
            return float((model.adot_conv2d(kernel.double(), v.double(), 0.5, **ck) - b.double()).abs().max())

        print("%s: |Adot(z) - b|_inf = %.3g (the model: %.3g), status %d at %d (the model: %d at %d)"
              % (name, resid(z), resid(zm), info["status"], info["iterations"], im["status"], im["iterations"]))
        record_margins("conjgrad/normal_equations_" + name, dict(resid=resid(z), model=resid(zm)))
        # (at this rtol float32 ends on the residual or, as the reference does, on curv_sum <= 3 eps: both mean converged)
        assert info["status"] in (1, 2) and im["status"] in (1, 2)
        assert resid(z) <= 4.0 * resid(zm)


# ---- 128 x 128 GEMM blocks, forced (LASSO_FORCE_BLOCKS_128) and chosen -------------------------------------------------------
# block_side() takes 128-blocks only from 2 x CUs blocks on (256 CUs: 8.4 M elements of the product), far above the
# shapes of this file.  The bit runs the product p A^T on Tile<128, 128>: CurvEpi (its per-row slots, one per column
# block, and skip()) in the fused form, StoreEpi in the plain one.  Shapes: more than one 128-block in a dimension and a
# nearly empty last one; k a multiple of 32 (LDS-DMA), of 4 (16-byte loads), odd (scalar loads); nine rows under three
# column blocks.
F128 = [(130, 96), (259, 132), (131, 31), (9, 288)]
F128_KW = dict(maxiter=6, rtol=0.0, tol=0.0)
_F128_MODEL = {}


def f128_model(n, k, maxiter=6):
    """the fresh-shape construction above, computed once per shape -> (A, b, xm, im, bar, rtol)"""
    key = (n, k, maxiter)
    if key not in _F128_MODEL:
        A, b = dense_inputs(dict(n=n, k=k, d=max(4, k // 4), seed=40))
        kw = dict(F128_KW, maxiter=maxiter)
        xm, im = model.batch_cg(A, b, **kw)
        bar, rtol = spread_against(lambda **knobs: model.batch_cg(A, b, **kw, **knobs), xm, im)
        _F128_MODEL[key] = (A, b, xm, im, bar, rtol)
    return _F128_MODEL[key]


def check_f128(tag, x, info, reference, iterations=6):
    A, b, xm, im, bar, rtol = reference
    dx, rs = float((x - xm).abs().max()), seq_rel(info, im)
    print("fresh %s: max|dx| = %.3g (bar %.3g), sequences rel %.3g (rtol %.3g)" % (tag, dx, bar, rs, rtol))
    record_margins("conjgrad/fresh_" + tag, dict(dx=dx, bar=bar, seq_rel=rs, seq_rtol=rtol))
    assert info["status"] == 4 and info["iterations"] == iterations and len(info["rs"]) == iterations
    assert dx <= bar and rs <= rtol


@pytest.mark.parametrize("force", [8, 0], ids=["f128", "s64"])
@pytest.mark.parametrize("plain", [0, 1], ids=["fused", "plain"])
@pytest.mark.parametrize("n,k", F128)
def test_forced_128_blocks_against_the_model(n, k, plain, force):
    from lasso_amd import _native as nat
    assert nat.FORCE_BLOCKS_128 == 8 and nat.CG_PLAIN_FORM == 1
    reference = f128_model(n, k)
    x, res, info, _ = abi_dense(reference[0], reference[1], reserved=force | plain, **F128_KW)
    assert info["form"] == ("unfused" if plain else "fused")
    check_f128("%dx%d_%s_%s" % (n, k, "plain" if plain else "fused", "f128" if force else "s64"), x, info, reference)


@pytest.mark.parametrize("plain", [0, 1], ids=["fused", "plain"])
def test_forced_128_blocks_pitched_repeatable_and_refused(plain):
    from lasso_amd import _native as nat
    force = nat.FORCE_BLOCKS_128 | plain
    A, b = f128_model(259, 132)[:2]
    x0, _, i0, _ = abi_dense(A, b, reserved=force, **F128_KW)
    x1, _, i1, _ = abi_dense(A, b, reserved=force, **F128_KW)
    assert torch.equal(bits(x0), bits(x1)) and i0 == i1        # two forced solves are bitwise equal
    for tag, plan in plans(("a", "b", "x")):                   # as at 64: the layout does not change a bit
        if tag == "natural" or not (tag.startswith("all-") or tag.endswith("-pitched")):
            continue
        x, res, info, ops = abi_dense(A, b, plan=plan, reserved=force, **F128_KW)
        for name, p in ops.items():
            p.check(written=(name == "x"))
        assert torch.equal(bits(x), bits(x0)) and info == i0, tag
    for bad in (force | 2, force | 4, force | 0x7f00):
        x, res, _, ops = abi_dense(A, b, plan=dict(x="pitched"), reserved=bad, expect=nat.LASSO_ERR_BAD_ARG, **F128_KW)
        assert (ops["x"].buffer == SENTINEL).all(), bad
        for name, p in ops.items():
            p.check(written=False)


def test_block_side_rule_at_its_threshold():
    """the smallest [n, 260] product that takes 128-blocks by itself: 3 column blocks, ceil(2 CUs / 3) row blocks, the
    last of them 91 rows.  The solve is unforced."""
    from lasso_amd import _native as nat
    L = nat.lib()
    cus = C.c_int(0)
    nat.check(L.lasso_hip_device_cus(C.byref(cus)))
    k = 260
    rb = -(-2 * cus.value // 3)
    n = 128 * (rb - 1) + 91
    ldmax = max(k, k)                                          # as csrc/conjgrad.hip takes it: lda = k
    assert L.lasso_solver_block_side(n, k, ldmax) == 128
    assert L.lasso_solver_block_side(n - 128, k, ldmax) == 64
    assert L.lasso_solver_block_side(n, k, 1 << 22) == 64      # a row pitch beyond the 32-bit block offsets
    print("block_side threshold: %d CUs, n = %d" % (cus.value, n))
    reference = f128_model(n, k, maxiter=3)
    for plain in (0, 1):
        x, res, info, _ = abi_dense(reference[0], reference[1], reserved=plain, **dict(F128_KW, maxiter=3))
        check_f128("threshold_%dx%d_%s" % (n, k, "plain" if plain else "fused"), x, info, reference, iterations=3)
