"""coord_descent_mod on the GPU (csrc/cd_mod.hip behind lasso_cd_mod_solve) against the fixture recorded from the
reference and its host model (tests/golden/cd_mod_cases.npz, tests/cd_mod_cases.py).

Per fixture case, with tol_row = tol * ||x_row||^2:
  (a) converged <=> reported gap < tol_row;
  (b) the reference's gap formula recomputed in float64 from the returned z differs from the reported gap by at most
      0.05 tol_row -- the margin the fixture's certification leaves, so no certified decision can flip;
  (c) rows reported unconverged ran max_iter sweeps;
  (d) on certified rows the sweeps equal the fixture's and |z - z32| <= 10 x the case's certified-row spread
      max|z32 - z64| (floored at 1e-6 max|z|; the all-zero case exactly zero) -- the factor covers the other summation
      order of the covariance form; the achieved ratio is recorded with tests/margins.py.  "Certified" here is the
      fixture's `decisive` flag: certified as to the gap's decision AND as to the check rule of :132, whose ratio
      max|change| / max|z| carries a relative rounding error of up to 5e-3 at tol = 1e-4 -- on the certified rows that
      are not decisive (1 of 64, 26 of 262, 9 of 300 ...) two runs of the float32 host model on different CPUs already
      stop a sweep apart, and so did the kernel (first GPU run: k1030 89 against 90 sweeps);
  (e) on all converged rows the float64 gap of the returned z is < 1.05 tol_row.
Every solve here is a fraction of a second; each case runs once and is shared by the checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import cd_mod_model
import layouts
from cd_mod_cases import CASES, MAX_ITER, TOL, case_inputs, gap_f64, load_case, tol_row
from margins import record_margins

pytestmark = pytest.mark.gpu


def solver():
    from lasso_amd.linear.solvers import coord_descent_mod
    return coord_descent_mod


@pytest.fixture(scope="module")
def cases(golden):
    return golden("cd_mod_cases")


@pytest.fixture(scope="module")
def solved():
    """every fixture case solved once on the GPU: name -> (x, w, z, gap, info), all on the CPU"""
    out = {}
    for name, spec in CASES.items():
        x, w = case_inputs(spec)
        z, gap, info = solver()(x.cuda(), w.cuda(), alpha=spec["alpha"], max_iter=MAX_ITER, tol=TOL, return_info=True)
        out[name] = (x, w, z.cpu(), gap.cpu(), {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in info.items()})
    return out


def gap_error(z, gap, x, w, alpha):
    """max over rows of (|reported gap - float64 gap of z| / tol_row), rows with tol_row == 0 by absolute difference"""
    tr = tol_row(x).double()
    diff = (gap.double() - gap_f64(z, x, w, alpha)).abs()
    rel = torch.where(tr > 0, diff / tr.clamp_min(1e-300), diff)
    return float(rel.max()) if rel.numel() else 0.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_fixture(cases, solved, name):
    spec, g = CASES[name], load_case(cases, name)
    x, w, z, gap, info = solved[name]
    n, k = spec["n"], spec["k"]
    assert z.shape == (n, k) and gap.shape == (n,) and gap.dtype == torch.float32
    assert info["sweeps"].dtype == torch.int32 and info["converged"].dtype == torch.bool
    tr = tol_row(x)
    conv = info["converged"]
    # (a)
    assert torch.equal(conv, gap < tr), name
    # (b)
    err = gap_error(z, gap, x, w, spec["alpha"])
    print("%s: |gap - gap64| / tol_row = %.4f" % (name, err))
    assert err <= 0.05, (name, err)
    # (c)
    assert (info["sweeps"][~conv] == MAX_ITER).all(), name
    # (d)
    c = torch.from_numpy(g["decisive"])
    assert torch.equal(info["sweeps"][c], torch.from_numpy(g["sweeps32"])[c]), name
    assert conv[c].all(), name
    spread = float(g["spread"][g["decisive"]].max())
    dz = float((z - torch.from_numpy(g["z32"]))[c].abs().max())
    zmax = float(np.abs(g["z32"]).max())
    bar = max(10.0 * spread, 1e-6 * zmax)
    ratio = dz / spread if spread > 0 else (0.0 if dz == 0 else float("inf"))
    print("%s: max|dz| = %.3e on certified rows, spread %.3e, ratio %.2f, bar %.3e" % (name, dz, spread, ratio, bar))
    record_margins("cd_mod/" + name, dict(dz=dz, spread=spread, ratio=ratio, bar=bar, gap_err_over_tol_row=err,
                                           certified_rows=int(c.sum()), rows=n))
    assert dz <= bar, (name, dz, bar)
    if name == "sq24_all_zero":
        assert not z.any()
    # (e)
    g64 = gap_f64(z, x, w, spec["alpha"])
    assert (g64[conv] < 1.05 * tr.double()[conv]).all(), name
    if "z_ref" in g:      # the reference's own float32 run, where it can run (n == d)
        assert float((z - torch.from_numpy(g["z_ref"]))[c].abs().max()) <= bar


def test_warm_start_in_place_and_zero_atom(solved):
    spec = CASES["sq48_zero_atom"]
    x, w = case_inputs(spec)
    n, k = spec["n"], spec["k"]
    gen = torch.Generator().manual_seed(5)
    start = 0.1 * torch.randn(n, k, generator=gen)
    start[:, 3] = 0.5                                   # atom 3 has zero norm: never visited, keeps its start
    sweeps = 60                                         # (no row converges, below: both sides run exactly these)
    want, _, winfo = cd_mod_model.coord_descent_mod(x, w, z0=start.clone(), alpha=spec["alpha"], max_iter=sweeps, tol=TOL)

    def check(z0, z, gap):
        assert z is z0                                               # the caller's tensor, updated in place
        zc = z.cpu()
        assert (zc[:, 3] == 0.5).all()
        assert gap_error(zc, gap.cpu(), x, w, spec["alpha"]) <= 0.05
        # the same 60 sweeps from the same start in another summation order: rounding only.  1e-4 is 20 x the largest
        # float32-float64 spread of the fixture's decisive rows (5e-6), and 1000 x below an error in the start's residual
        assert float((zc - want).abs().max()) <= 1e-4
        assert not torch.equal(zc, start)

    xg, wg = x.cuda(), w.cuda()
    z0 = start.clone().cuda()
    ptr = z0.data_ptr()
    z, gap = solver()(xg, wg, z0=z0, alpha=spec["alpha"], max_iter=sweeps)
    assert z.data_ptr() == ptr and gap.is_cuda
    check(z0, z, gap)
    first = z.cpu().clone()
    # a z0 on the CPU: staged, copied back, returned on the CPU with its gap
    z0 = start.clone()
    z, gap = solver()(xg, wg, z0=z0, alpha=spec["alpha"], max_iter=sweeps)
    assert not z.is_cuda and not gap.is_cuda
    check(z0, z, gap)
    assert torch.equal(z, first)
    # a column-strided z0 on the device
    z0 = start.T.contiguous().cuda().T
    assert z0.stride(1) != 1
    z, gap = solver()(xg, wg, z0=z0, alpha=spec["alpha"], max_iter=sweeps)
    check(z0, z, gap)
    assert torch.equal(z.cpu(), first)
    # the start value on the zero atom counts in alpha * ||z||_1 of the gap (:96) like any other: 0.5 * 0.2 is far above
    # the threshold, so these rows never converge -- in the reference's arithmetic and here
    assert (winfo["sweeps"] == sweeps).all() and not winfo["converged"].any()
    # a warm start at the cold start's solution needs fewer sweeps than the cold start did
    cold_z, cold = solved["sq48_zero_atom"][2], solved["sq48_zero_atom"][4]["sweeps"]
    _, _, info = solver()(xg, wg, z0=cold_z.clone().cuda(), alpha=spec["alpha"], return_info=True)
    assert info["sweeps"].float().mean() < cold.float().mean()


def test_sweep_limits(solved):
    spec = CASES["sq32"]
    x, w = case_inputs(spec)
    xg, wg = x.cuda(), w.cuda()
    z, gap, info = solver()(xg, wg, alpha=spec["alpha"], max_iter=0, tol=TOL, return_info=True)
    assert not z.any() and torch.equal(gap.cpu(), torch.full((32,), TOL + 1.0)) and not info["sweeps"].any()
    assert not info["converged"].any() and info["committed"] == 0
    z0 = torch.full((32, 80), 0.125).cuda()
    z, gap = solver()(xg, wg, z0=z0, alpha=spec["alpha"], max_iter=0)
    assert z is z0 and (z == 0.125).all() and torch.equal(gap.cpu(), torch.full((32,), TOL + 1.0))
    # one sweep: every row is checked once (:132, the last sweep) and reports the gap of what it holds
    z, gap, info = solver()(xg, wg, alpha=spec["alpha"], max_iter=1, tol=TOL, return_info=True)
    assert (info["sweeps"] == 1).all()
    assert gap_error(z.cpu(), gap.cpu(), x, w, spec["alpha"]) <= 0.05
    want, _, _ = cd_mod_model.coord_descent_mod(x, w, alpha=spec["alpha"], max_iter=1, tol=TOL)
    assert float((z.cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert torch.equal(info["converged"].cpu(), gap.cpu() < tol_row(x))


def test_cut_off_rows_report_their_gap():
    spec = CASES["sq32"]
    x, w = case_inputs(spec)
    z, gap, info = solver()(x.cuda(), w.cuda(), alpha=spec["alpha"], max_iter=5, tol=TOL, return_info=True)
    z, gap, conv, sweeps = z.cpu(), gap.cpu(), info["converged"].cpu(), info["sweeps"].cpu()
    assert (~conv).sum() >= 16                      # the fixture's rows need 31 .. 166 sweeps
    assert (sweeps[~conv] == 5).all() and (sweeps <= 5).all()
    assert gap_error(z, gap, x, w, spec["alpha"]) <= 0.05
    assert torch.equal(conv, gap < tol_row(x)) and (gap[~conv] != TOL + 1.0).all()


def test_zero_row():
    spec = CASES["tiny"]
    x, w = case_inputs(spec)
    x[3] = 0.0
    z, gap, info = solver()(x.cuda(), w.cuda(), alpha=spec["alpha"], max_iter=200, tol=TOL, return_info=True)
    assert not z[3].any() and float(gap[3]) == 0.0
    assert not bool(info["converged"][3]) and int(info["sweeps"][3]) == 200        # 0 < 0 never holds
    want, wgap, winfo = cd_mod_model.coord_descent_mod(x, w, alpha=spec["alpha"], max_iter=200, tol=TOL)
    assert int(winfo["sweeps"][3]) == 200 and float(wgap[3]) == 0.0
    assert gap_error(z.cpu(), gap.cpu(), x, w, spec["alpha"]) <= 0.05


def test_row_wrap_and_determinism():
    """more rows than one pass of the grid (4 waves x 8 workgroups per compute unit): a wave takes a second row, and a
    row's result does not depend on which wave solved it"""
    from lasso_amd import _native as nat
    cus = C.c_int(0)
    assert nat.lib().lasso_hip_device_cus(C.byref(cus)) == 0 and cus.value > 0
    spec = CASES["tiny"]
    x, w = case_inputs(spec)
    n = 32 * cus.value + 37
    xb = x.repeat((n + 39) // 40, 1)[:n].contiguous().cuda()
    wg = w.cuda()
    small = solver()(x.cuda(), wg, alpha=spec["alpha"], return_info=True)
    big = solver()(xb, wg, alpha=spec["alpha"], return_info=True)
    again = solver()(xb, wg, alpha=spec["alpha"], return_info=True)
    idx = torch.arange(n, device="cuda") % 40
    assert torch.equal(big[0], small[0][idx]) and torch.equal(big[1], small[1][idx])
    assert torch.equal(big[2]["sweeps"], small[2]["sweeps"][idx])
    assert torch.equal(big[2]["converged"], small[2]["converged"][idx])
    # two identical calls: the same bits
    assert torch.equal(big[0], again[0]) and torch.equal(big[1], again[1])
    assert torch.equal(big[2]["sweeps"], again[2]["sweeps"]) and big[2]["committed"] == again[2]["committed"]


def test_return_info_counts(cases, solved):
    # a sparse case: far fewer coordinate updates than k per sweep -- the skipping is live
    spec = CASES["sq64"]
    info = solved["sq64"][4]
    total = spec["k"] * int(info["sweeps"].sum())
    assert 0 < info["committed"] < total // 4, (info["committed"], total)
    # the all-zero case: the model's count (no update changes a value)
    assert solved["sq24_all_zero"][4]["committed"] == int(cases["sq24_all_zero/committed32"]) == 0
    assert (solved["sq24_all_zero"][4]["sweeps"] == 1).all()
    # without return_info: two values
    x, w = case_inputs(CASES["k1"])
    out = solver()(x.cuda(), w.cuda(), alpha=0.1)
    assert isinstance(out, tuple) and len(out) == 2


def test_refusals_on_the_device():
    x, w = torch.randn(4, 3).cuda(), torch.randn(3, 5).cuda()
    with pytest.raises(NotImplementedError, match="float64"):
        solver()(x.double(), w.double())
    with pytest.raises(NotImplementedError, match="4096"):
        solver()(x, torch.randn(3, 5000).cuda())


# ---- the C ABI directly, on pitched, odd-pitch and offset operands --------------------------------------------------
N, D, K, ALPHA = 37, 19, 70, 0.25


def _abi_call(px, pw, pz, gap, sweeps, conv, ldx=None, ldw=None, ldz=None, max_iter=300):
    from lasso_amd import _native as nat
    L = nat.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = nat.workspace(dev, L.lasso_cd_mod_workspace_bytes(N, D, K, nat.LASSO_F32), "cd_mod_test")
    unconv, committed = C.c_int32(-1), C.c_int64(-1)
    st = L.lasso_cd_mod_solve(nat.ptr(px.view), px.ld if ldx is None else ldx, nat.ptr(pw.view),
                              pw.ld if ldw is None else ldw, nat.ptr(pz.view), pz.ld if ldz is None else ldz, 1,
                              nat.ptr(gap), nat.ptr(sweeps), nat.ptr(conv), N, D, K, nat.LASSO_F32, ALPHA, max_iter, TOL,
                              C.byref(unconv), C.byref(committed), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
    torch.cuda.synchronize()
    return st, unconv.value, committed.value


def test_c_abi_layouts():
    from lasso_amd import _native as nat
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(N, D, generator=gen)
    w = torch.nn.functional.normalize(torch.randn(D, K, generator=gen), dim=0) * (0.5 + torch.rand(K, generator=gen))
    z0 = 0.05 * torch.randn(N, K, generator=gen)
    anchor = None
    for tag, plan in layouts.plans(["x", "w", "z"]):
        px = layouts.place(x, plan["x"], float("nan"), "cuda", "x")
        pw = layouts.place(w, plan["w"], float("nan"), "cuda", "w")
        pz = layouts.place(z0, plan["z"], layouts.SENTINEL, "cuda", "z")
        gap = torch.full((N + 2,), layouts.SENTINEL, device="cuda")
        sweeps = torch.full((N + 2,), -7, dtype=torch.int32, device="cuda")
        conv = torch.full((N + 2,), 9, dtype=torch.uint8, device="cuda")
        st, unconv, committed = _abi_call(px, pw, pz, gap[1:], sweeps[1:], conv[1:])
        assert st == nat.LASSO_OK, (tag, nat.lib().lasso_hip_last_error())
        px.check(); pw.check(); pz.check(written=True)
        assert float(gap[0]) == layouts.SENTINEL and float(gap[-1]) == layouts.SENTINEL
        assert int(sweeps[0]) == -7 and int(sweeps[-1]) == -7 and int(conv[0]) == 9 and int(conv[-1]) == 9
        got = (pz.view.clone(), gap[1:-1].clone(), sweeps[1:-1].clone(), conv[1:-1].clone(), unconv, committed)
        assert not torch.isnan(got[0]).any() and not torch.isnan(got[1]).any(), tag
        if anchor is None:
            anchor = got
            assert unconv == int((got[3] == 0).sum()) and committed > 0
            assert gap_error(got[0].cpu(), got[1].cpu(), x, w, ALPHA) <= 0.05
        else:
            for a, b in zip(anchor[:4], got[:4]):
                assert torch.equal(a, b), tag
            assert got[4:] == anchor[4:], tag
    # a leading dimension below the row length: refused, nothing enqueued, nothing written
    for bad in (dict(ldx=D - 1), dict(ldw=K - 1), dict(ldz=K - 1)):
        px = layouts.place(x, "natural", float("nan"), "cuda", "x")
        pw = layouts.place(w, "natural", float("nan"), "cuda", "w")
        pz = layouts.place(z0, "pitched", layouts.SENTINEL, "cuda", "z")
        gap = torch.full((N,), layouts.SENTINEL, device="cuda")
        st, unconv, committed = _abi_call(px, pw, pz, gap, None, None, **bad)
        assert st == nat.LASSO_ERR_BAD_ARG, bad
        pz.check(); px.check(); pw.check()
        assert (gap == layouts.SENTINEL).all() and (unconv, committed) == (-1, -1)
