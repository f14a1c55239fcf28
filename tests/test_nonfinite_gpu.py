"""NaN and Inf operand values through every solver on the HIP path, against the CPU oracle (tests/nonfinite_cases.py is
the case table, tests/test_nonfinite_cpu.py pins what the oracle does with each case).  Per entry point:

* containment -- rows (images) whose own inputs are finite are ``torch.equal`` to the same call on the clean batch;
* visibility  -- on the poisoned rows (images) the map {finite, NaN, +Inf, -Inf} is the oracle's, element for element,
  and what stays finite there meets the entry point's usual bar (Z_ATOL, F64_BAR);
* bookkeeping -- with tol > 0 the solve runs the oracle's iteration count (maxiter), reports a NaN last sum and warns
  only where the reference warns.

The poisons are VALUES inside valid buffers; nothing here is meant to fault or hang.  Read for bounds before the first
run -- every index or trip count that derives from a floating value stays in range for NaN / +-Inf, and every loop whose
exit is a float comparison is also counted:

* fista_tile_sp / fista_splitk (fused fp32 FISTA): no index from data; the in-kernel stop rule compares a sum with the
  budget (NaN: no stop) inside ``it < iters``; the handshake spins are on integer epochs, capped by kStopSpinLimit.
* gemm_nt + prox epilogue (general GEMM path), gemm_f64 / conv_f64 (float64): no index from data; the host loops are
  ``it < maxiter`` and speculate_stop_rule (tests/test_stoprule_host_cpu.py: NaN and Inf sums, chunk sizes in [1, 64]).
* bt16_persist / bt_iter / backtrack (line search, fp32 and bf16): a NaN objective rejects every trial; the trials are
  counted (kBtMaxTrials = kMaxTrials = 1000, ista.py:17), the last one is forced; spins are on integer epochs, capped.
* cd_rows_kernel: the argmax column comes from a ballot of lanes whose key equals the wave maximum, so it is < KP
  whatever the data (and guarded); ``steps < iters`` counts the loop.
* cd_mod_rows_kernel: the cursor of a sweep only moves forward over column indices < KP (integers, never a float); the
  sweeps are counted by ``sweeps < max_iter``; rebuild_q's loop is the same cursor.
* conv_fused / conv_synth / conv_synth_few / conv_grad_prox / explicit conv: geometry alone indexes; the float -> int
  casts of conv.hip and conv_fused.hip divide integer offsets by image sizes, never data.
* conv_lip_kernel, lipschitz (squarings): loops over the frequency grid / a fixed number of squarings with an early
  exit on a float test inside the count.
* M-step (gram, sweep, degenerate fix-up, ridge): ``ss < eps2`` is False for NaN (not degenerate); the degenerate list
  is built from integer flags, at most k entries; a NaN pivot of the Cholesky factor is reported (ridge.hip:122).
* autograd (bw_prox and the GEMMs), patches: elementwise / geometry-indexed.
"""
import math
import os
import warnings

import pytest
import torch

import bf16_model
import cd_mod_model
import nonfinite_cases as nf
from nonfinite_cases import FINITE, IS_NAN, NAN, PINF, classes, poison

pytestmark = pytest.mark.gpu

Z_ATOL = 5e-5                           # tests/test_fista_gpu.py, test_conv_gpu.py, test_cd_gpu.py
F64_BAR = 5e-5 * 2.0 ** -29             # tests/test_layouts_gpu.py
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def _mods():
    from lasso_amd import _native as nat
    from lasso_amd.linear.solvers import ista, coord_descent, coord_descent_mod
    from oracle import lasso_oracle as orc
    return nat, ista, coord_descent, coord_descent_mod, orc


def _rest(n, bad):
    return torch.tensor([i for i in range(n) if i not in set(bad)], dtype=torch.long)


def _held(got, clean_got, ref, bad, atol, what):
    """containment and visibility of one poisoned call: got / clean_got from the HIP path, ref from the oracle"""
    got, clean_got = got.cpu(), clean_got.cpu()
    rest, badt = _rest(got.shape[0], bad), torch.tensor(sorted(bad), dtype=torch.long)
    assert torch.equal(got[rest], clean_got[rest]), (what, "a clean row moved")
    cg, cr = classes(got[badt]), classes(ref[badt])
    assert torch.equal(cg, cr), (what, "class map", int((cg != cr).sum()), cg[cg != cr][:8].tolist(), cr[cg != cr][:8].tolist())
    fin = cr == FINITE
    if fin.any():
        err = (got[badt].double() - ref[badt].double())[fin].abs().max().item()
        assert err <= atol, (what, err)


def _x_cases(X, z0, W, n, d, k):
    """name -> (x, z0, W, poisoned rows or None for all)"""
    pos = nf.row_positions(n, d)
    bad = [r for r, _ in pos]
    out = {name: (poison(X, pos, value), z0, W, bad) for name, value in nf.X_POISONS}
    out["z0"] = (X, poison(z0, [(r, k - 1) for r in bad], NAN), W, bad)
    out["w"] = (X, z0, poison(W, (d - 1, k - 1), NAN), list(range(n)))
    return out


# ---- ista, fp32 ---------------------------------------------------------------------------------------------------
FP32_CASES = ([(s, "auto") for s in nf.LINEAR_FUSED[:2]] + [(nf.LINEAR_FUSED[2], "tile"), (nf.LINEAR_FUSED[2], "splitk")]
              + [(s, "auto") for s in nf.LINEAR_GENERAL])


def _fp32_name(nat, n, d, k, kernel):
    name = nat.lib().lasso_fista_kernel_name(n, d, k, nat.LASSO_F32, 0).decode()
    if (n, d, k) in nf.LINEAR_GENERAL:
        assert "unfused" in name, name
    else:
        assert "fista_tile_sp" in name or "splitk" in name, name
    return name


@pytest.mark.parametrize("T", nf.ITERS)
@pytest.mark.parametrize("fast", [True, False], ids=["fista", "ista"])
@pytest.mark.parametrize("shape,kernel", FP32_CASES, ids=["%dx%dx%d-%s" % (s + (kn,)) for s, kn in FP32_CASES])
def test_ista_fp32(shape, kernel, fast, T):
    nat, ista, _, _, orc = _mods()
    n, d, k = shape
    _fp32_name(nat, n, d, k, kernel)
    X, W, z0, lr = nf.linear_problem(n, d, k)
    kw = dict(fast=fast, lr=lr, maxiter=T, tol=0.0, kernel=kernel)
    clean = ista(X.cuda(), z0.cuda(), W.cuda(), nf.ALPHA, **kw)
    assert classes(clean).eq(FINITE).all()
    for name, (xp, zp, wp, bad) in _x_cases(X, z0, W, n, d, k).items():
        ref = orc.fista(xp, zp, wp, nf.ALPHA, fast=fast, lr=lr, maxiter=T, tol=0.0)
        got = ista(xp.cuda(), zp.cuda(), wp.cuda(), nf.ALPHA, **kw)
        assert not classes(ref[torch.tensor(bad)]).eq(FINITE).any()            # (the poison fills its rows)
        _held(got, clean, ref, bad, Z_ATOL, (name, shape, kernel, fast, T))


@pytest.mark.parametrize("stop_mode", ["global", "chunked"])
@pytest.mark.parametrize("shape,kernel", FP32_CASES, ids=["%dx%dx%d-%s" % (s + (kn,)) for s, kn in FP32_CASES])
def test_ista_fp32_bookkeeping(shape, kernel, stop_mode):
    nat, ista, _, _, orc = _mods()
    n, d, k = shape
    X, W, z0, lr = nf.linear_problem(n, d, k)
    pos = nf.row_positions(n, d)[1:2]
    for name, value in nf.X_POISONS:
        xp = poison(X, pos, value)
        tr = orc.FistaTrace()
        ref = orc.fista(xp, z0, W, nf.ALPHA, lr=lr, maxiter=12, tol=1e-4, trace=tr)
        assert tr.iterations == 12 and math.isnan(tr.delta[-1])
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got, info = ista(xp.cuda(), z0.cuda(), W.cuda(), nf.ALPHA, lr=lr, maxiter=12, tol=1e-4, return_info=True,
                             stop_mode=stop_mode, kernel=kernel)
        assert info["iterations"] == tr.iterations, (name, info)
        assert math.isnan(info["last_delta"]), (name, info)
        assert torch.equal(classes(got), classes(ref)), name
        # the rows beside it: those of 12 plain iterations of the clean batch
        plain = ista(X.cuda(), z0.cuda(), W.cuda(), nf.ALPHA, lr=lr, maxiter=12, tol=0.0, kernel=kernel)
        rest = _rest(n, [pos[0][0]])
        assert torch.equal(got.cpu()[rest], plain.cpu()[rest]), name


# ---- ista, bf16 native path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", nf.ITERS)
@pytest.mark.parametrize("n,d,k", nf.LINEAR_BF16)
def test_ista_bf16(n, d, k, T):
    nat, ista, _, _, _ = _mods()
    assert "bt16" in nat.lib().lasso_fista_kernel_name(n, d, k, nat.LASSO_BF16, 0).decode()
    X, W, z0, lr = nf.linear_problem(n, d, k)
    X, W, z0 = X.to(BF16), W.to(BF16), z0.to(BF16)
    clean = ista(X.cuda(), z0.cuda(), W.cuda(), nf.ALPHA, lr=lr, maxiter=T, tol=0.0)
    assert clean.dtype == BF16 and classes(clean).eq(FINITE).all()
    for name, (xp, zp, wp, bad) in _x_cases(X, z0, W, n, d, k).items():
        ref, _ = bf16_model.solve(xp, zp, wp, nf.ALPHA, lr, T, tol=0.0, backtrack=False)
        got = ista(xp.cuda(), zp.cuda(), wp.cuda(), nf.ALPHA, lr=lr, maxiter=T, tol=0.0)
        assert not classes(ref[torch.tensor(bad)]).eq(FINITE).any()
        _held(got.float(), clean.float(), ref.float(), bad, 0.0, (name, n, d, k, T))
    xp = poison(X, nf.row_positions(n, d)[:1], NAN)
    _, minfo = bf16_model.solve(xp, z0, W, nf.ALPHA, lr, 12, tol=1e-4, backtrack=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _, info = ista(xp.cuda(), z0.cuda(), W.cuda(), nf.ALPHA, lr=lr, maxiter=12, tol=1e-4, return_info=True)
    assert info["iterations"] == minfo["iterations"] == 12 and math.isnan(info["last_delta"]) and math.isnan(minfo["last_delta"])


# ---- ista, float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", nf.ITERS)
@pytest.mark.parametrize("auto", [False, True], ids=["lr", "auto"])
@pytest.mark.parametrize("n,d,k", nf.LINEAR_F64)
def test_ista_f64(n, d, k, auto, T):
    """A NaN row must come back NaN: the ternary softshrink of the float64 kernels sent it to an all-zero code."""
    nat, ista, _, _, orc = _mods()
    assert nat.lib().lasso_fista_kernel_name(n, d, k, nat.LASSO_F64, 0).decode() != ""
    X, W, z0, lr = nf.linear_problem(n, d, k, dtype=F64)
    step = "auto" if auto else lr
    ref_lr = 1.0 / orc.lipschitz_constant(W, "exact") if auto else lr
    clean = ista(X.cuda(), z0.cuda(), W.cuda(), nf.ALPHA, lr=step, maxiter=T, tol=0.0)
    assert clean.dtype == F64 and classes(clean).eq(FINITE).all()
    for name, (xp, zp, wp, bad) in _x_cases(X, z0, W, n, d, k).items():
        if auto and name == "w":
            continue                                   # (the step of a NaN dictionary: test_lipschitz_and_auto_step)
        ref = orc.fista(xp, zp, wp, nf.ALPHA, lr=ref_lr, maxiter=T, tol=0.0)
        got = ista(xp.cuda(), zp.cuda(), wp.cuda(), nf.ALPHA, lr=step, maxiter=T, tol=0.0)
        assert not classes(ref[torch.tensor(bad)]).eq(FINITE).any()
        _held(got, clean, ref, bad, F64_BAR, (name, n, d, k, auto, T))
    for stop_mode in ("global", "chunked"):
        xp = poison(X, nf.row_positions(n, d)[2:], NAN)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            _, info = ista(xp.cuda(), z0.cuda(), W.cuda(), nf.ALPHA, lr=step, maxiter=12, tol=1e-4, return_info=True,
                           stop_mode=stop_mode)
        assert info["iterations"] == 12 and math.isnan(info["last_delta"]), info


# ---- ista(backtrack=True) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16, F64], ids=["fp32", "bf16", "f64"])
def test_ista_backtrack(dtype):
    """oracle.backtracking_step on a NaN objective (ista.py:45: F <= Q is False): all 1000 trials of every outer
    iteration, the warning, the step back at lr0 (:48-52) -- so the clean rows are those of the FIXED-step solve of the
    clean batch.  The HIP paths cap the trials at the same 1000 (lasso_hip.hip kBtMaxTrials, bt16_persist.hip and
    gemm_f64.hip kMaxTrials) and follow the reference on this path: no extension to document."""
    nat, ista, _, _, orc = _mods()
    n, d, k = nf.LINEAR_FUSED[0]
    X, W, z0, lr = nf.linear_problem(n, d, k, dtype=F64 if dtype == F64 else F32)
    X, W, z0 = X.to(dtype), W.to(dtype), z0.to(dtype)
    pos = nf.row_positions(n, d)
    bad = [r for r, _ in pos]
    xp = poison(X, pos, NAN)
    if dtype == BF16:
        ref, rinfo = bf16_model.solve(xp, z0, W, nf.ALPHA, lr, 2, tol=0.0, backtrack=True)
        trials, lrs = rinfo["trials"], rinfo["accepted_lr"]
    else:
        tr = orc.FistaTrace()
        with pytest.warns(UserWarning, match="backtracking line search failed"):
            ref = orc.fista(xp, z0, W, nf.ALPHA, lr=lr, maxiter=2, tol=0.0, backtrack=True, trace=tr)
        trials, lrs = tr.trials, tr.accepted_lr
    assert trials == [1000, 1000]
    with pytest.warns(UserWarning, match="backtracking line search failed"):
        got, info = ista(xp.cuda(), z0.cuda(), W.cuda(), nf.ALPHA, lr=lr, maxiter=2, tol=0.0, backtrack=True,
                         return_info=True)
    print("backtrack", dtype, info["trials"], info["accepted_lr"], info["last_delta"])
    assert info["iterations"] == 2 and list(info["trials"]) == trials
    real = (lambda v: v) if dtype == F64 else (lambda v: float(torch.tensor(v, dtype=F32)))
    assert [real(v) for v in info["accepted_lr"]] == [real(v) for v in lrs]
    assert math.isnan(info["last_delta"])
    # (the search sums over the whole batch: no bitwise containment is claimed -- the class map of every row, and the
    # clean rows at the entry point's bar; bf16 codes are compared with their model by tests/test_backtrack_gpu.py)
    assert torch.equal(classes(got), classes(ref))
    badt, rest = torch.tensor(bad), _rest(n, bad)
    assert classes(ref[badt]).eq(IS_NAN).all() and classes(ref[rest]).eq(FINITE).all()
    if dtype != BF16:
        assert (got.cpu()[rest] - ref[rest]).abs().max().item() <= (F64_BAR if dtype == F64 else Z_ATOL)


# ---- coordinate descent -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["x", "z0"])
@pytest.mark.parametrize("n,d,k", nf.CD_SHAPES)
def test_coord_descent(n, d, k, what):
    """NaN in x: b = x W is NaN, the row's code is NaN after its first step and the row leaves the active set, as in
    the reference.  NaN in z0[i, j]: the documented departure (README "Non-finite inputs").  The reference reaches the
    result only through the argmax (coordinate_descent.py:34: |NaN| is torch's maximum, so coordinate j is committed and
    its NaN move poisons b, :36); cd_rows_kernel's maximum is fmaxf (cd.hip:104), which never takes a NaN candidate:
    coordinate j is never chosen, the tracked z keeps its NaN there and the row's code S(b) stays finite.  An argmax on
    the bit patterns follows the reference but measured 8 % slower on the benchmark's cd workload
    (profiles/nonfinite/README.md), so the kernel stays and this test pins what it does."""
    _, _, coord_descent, _, orc = _mods()
    X, W, z0, _ = nf.linear_problem(n, d, k)
    bad = [0, n - 1]
    xp = poison(X, [(0, 0), (n - 1, d - 1)], NAN) if what == "x" else X
    zp = poison(z0, [(0, 0), (n - 1, k - 1)], NAN) if what == "z0" else z0
    ref, rinfo = orc.coordinate_descent(xp, W, zp.clone(), nf.ALPHA, maxiter=30, return_info=True)
    clean = coord_descent(X.cuda(), W.cuda(), z0.clone().cuda(), nf.ALPHA, maxiter=30)
    zt = zp.clone().cuda()
    got, info = coord_descent(xp.cuda(), W.cuda(), zt, nf.ALPHA, maxiter=30, return_info=True)
    if what == "x":
        _held(got, clean, ref, bad, Z_ATOL, (what, n, d, k))
        assert info["n_active"] == rinfo["n_active"], (info, rinfo["n_active"])     # the poisoned rows left the active set
        assert torch.equal(classes(zt), classes(rinfo["z_track"]))                  # the tracked code, updated in place
    else:
        assert classes(ref[torch.tensor(bad)]).eq(IS_NAN).all()                     # the reference: NaN rows
        rest = _rest(n, bad)
        assert torch.equal(got.cpu()[rest], clean.cpu()[rest])                      # containment holds
        assert classes(got).eq(FINITE).all()                                        # the departure: finite codes ...
        assert torch.equal(classes(zt), classes(zp))                                # ... the NaN stays in the tracked z


@pytest.mark.parametrize("what", ["x", "x-from-zero", "z0"])
@pytest.mark.parametrize("n,d,k", nf.CD_SHAPES)
def test_coord_descent_mod(n, d, k, what):
    """S(NaN) / ||w||^2 is NaN (coordinate_descent.py:118-121): a sweep must visit a coordinate whose correlation is
    NaN -- `|q| > alpha` alone skips it and, from a zero start (z0=None), returns zeros for a NaN row."""
    _, _, _, coord_descent_mod, _ = _mods()
    X, W, z0, _ = nf.linear_problem(n, d, k)
    bad = [0, n - 1]
    xp = poison(X, [(0, 0), (n - 1, d - 1)], NAN) if what != "z0" else X
    zp = poison(z0, [(0, 0), (n - 1, k - 1)], NAN) if what == "z0" else z0
    start = (lambda z, dev: None) if what == "x-from-zero" else (lambda z, dev: z.clone().to(dev))
    ref, rgap, rinfo = cd_mod_model.coord_descent_mod(xp, W, start(zp, "cpu"), nf.ALPHA, max_iter=6, tol=1e-4)
    clean, cgap, cinfo = coord_descent_mod(X.cuda(), W.cuda(), start(z0, "cuda"), nf.ALPHA, max_iter=6, tol=1e-4,
                                           return_info=True)
    got, gap, info = coord_descent_mod(xp.cuda(), W.cuda(), start(zp, "cuda"), nf.ALPHA, max_iter=6, tol=1e-4,
                                       return_info=True)
    _held(got, clean, ref, bad, Z_ATOL, (what, n, d, k))
    rest, badt = _rest(n, bad), torch.tensor(bad)
    assert torch.equal(gap.cpu()[rest], cgap.cpu()[rest]) and torch.equal(info["sweeps"].cpu()[rest], cinfo["sweeps"].cpu()[rest])
    assert torch.equal(classes(gap)[badt], classes(rgap)[badt])                 # NaN: the last sweep is always checked
    assert torch.equal(info["sweeps"].cpu()[badt], rinfo["sweeps"][badt]) and not info["converged"].cpu()[badt].any()


# ---- ista_conv2d --------------------------------------------------------------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


CONV_RUNS = [("fused", F32, None), ("bands", F32, None), ("fused", F32, "0"), ("synth", F32, None),
             ("synth_few", F32, None), ("explicit", F32, None), ("synth", F64, None), ("explicit", F64, None)]


def _conv_form(nat, name, N, env):
    _, C, K, ks, pd, st, Hz, Wz = nf.CONV_CASES[name]
    args = (N, C, (Hz - 1) * st - 2 * pd + ks, (Wz - 1) * st - 2 * pd + ks, K, Hz, Wz, ks, ks, st, st, pd, pd)
    got = nat.lib().lasso_conv_ista_kernel_name(*args).decode()
    if name in ("fused", "bands") and env is None:
        assert "conv_fused_kernel" in got, got
    elif name == "explicit":
        assert "conv_residual_kernel" in got, got
    else:
        assert "conv_fused_kernel" not in got, got
        if name in ("synth", "synth_few"):
            assert "lasso::conv_%s_kernel" % name in got, got


@pytest.mark.parametrize("name,dtype,env", CONV_RUNS,
                         ids=["%s-%s%s" % (n_, "f64" if t_ == F64 else "fp32", "-two-kernel" if e_ else "") for n_, t_, e_ in CONV_RUNS])
def test_ista_conv2d(name, dtype, env):
    """One NaN pixel of one image: the NaN set of that image's code is the block of positions whose receptive field
    reaches the pixel -- growing with every iteration, exactly the oracle's -- and every other image is untouched."""
    from lasso_amd.conv2d import ista_conv2d
    nat, _, _, _, orc = _mods()
    N = {"fused": _cus() + 3, "bands": _cus() // 4}.get(name, nf.CONV_CASES[name][0])
    img = 1 if N <= 3 else N - 2                       # (a late image: past the first round of workgroups)
    x, w, z0, lr, st, pd = nf.conv_problem(name, N=N, dtype=dtype)
    xp = poison(x, (img,) + nf.CONV_PIXEL[name], NAN)
    near = [img - 1, img, img + 1]                     # the oracle on the poisoned image and its two neighbours
    atol = F64_BAR if dtype == F64 else Z_ATOL
    if env is not None:
        os.environ["LASSO_CONV_FUSED"] = env
    try:
        if dtype == F32:
            _conv_form(nat, name, N, env)
        xg, xpg, wg, zg = x.cuda(), xp.cuda(), w.cuda(), z0.cuda()
        for T in nf.CONV_ITERS:
            kw = dict(stride=st, padding=pd, maxiter=T, lr=lr, tol=0.0)
            clean = ista_conv2d(xg, zg, wg, nf.ALPHA, **kw)
            got = ista_conv2d(xpg, zg, wg, nf.ALPHA, **kw)
            ref = orc.conv_fista(xp[near], z0[near], w, nf.ALPHA, **kw)
            reach = nf.conv_reach(name, T, x.shape[2:], z0.shape[2:])
            assert torch.equal(classes(ref[1]).eq(IS_NAN), reach.expand(z0.shape[1], -1, -1))
            _held(got, clean, torch.cat([clean.cpu()[:img - 1], ref, clean.cpu()[img + 2:]]), [img], atol, (name, T))
            assert (clean.cpu()[near] - orc.conv_fista(x[near], z0[near], w, nf.ALPHA, **kw)).abs().max().item() <= atol
        _, rinfo = orc.conv_fista(xp[near], z0[near], w, nf.ALPHA, stride=st, padding=pd, maxiter=12, lr=lr, tol=1e-4,
                                  return_info=True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            _, info = ista_conv2d(xpg, zg, wg, nf.ALPHA, stride=st, padding=pd, maxiter=12, lr=lr, tol=1e-4,
                                  return_info=True)
        assert info["iterations"] == rinfo["iterations"] == 12 and math.isnan(info["last_delta"])
    finally:
        os.environ.pop("LASSO_CONV_FUSED", None)


# ---- bounds, steps, objectives ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "f64"])
@pytest.mark.parametrize("value", [NAN, PINF], ids=["nan", "pinf"])
def test_conv_bound_and_auto_step(dtype, value):
    """lip_const.py:131: torch.max keeps the NaN of a frequency (Inf * sin(0) is one); fmax dropped it"""
    from lasso_amd.conv2d import ista_conv2d, lip_bound_conv2d
    _, _, _, _, orc = _mods()
    x, w, z0, lr, st, pd = nf.conv_problem("synth", dtype=dtype)
    wp = poison(w, (3, 2, 1, 1), value)
    for kern in (wp, wp.transpose(0, 1).contiguous()):
        ref = orc.conv_lipschitz_bound(kern.float(), pd)              # (the reference's bound is float32 arithmetic)
        got = lip_bound_conv2d(kern.cuda(), pd)
        assert got.dtype == dtype and torch.equal(classes(got), classes(ref)) and math.isnan(ref.item())
        assert math.isnan(lip_bound_conv2d(kern.cuda(), pd, sqrt=True).item())
    # lr='auto' on that kernel: the step is 1 / NaN, which the reference's softshrink refuses (ista.py:29 -> ATen:
    # "lambda must be in range") and the HIP path refuses as a bad argument before any launch (README "Non-finite inputs")
    with pytest.raises(RuntimeError, match="lambda must be"):
        orc.conv_fista(x.float(), z0.float(), wp.float(), nf.ALPHA, padding=pd, maxiter=2, tol=0.0)
    with pytest.raises(ValueError, match="lr"):
        ista_conv2d(x.cuda(), z0.cuda(), wp.cuda(), nf.ALPHA, padding=pd, maxiter=2, tol=0.0)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "f64"])
@pytest.mark.parametrize("value", [NAN, PINF], ids=["nan", "pinf"])
def test_lipschitz_and_auto_step(dtype, value):
    """The reference has no value here: ARPACK refuses a Gram matrix with a NaN (ista.py:8-14 raises ArpackError,
    tests/test_nonfinite_cpu.py).  The HIP path's documented extension (README "Non-finite inputs"): lipschitz_constant
    returns NaN.  lr='auto' then has the step 1 / NaN: where the host computes it (fp32 beyond the fused shapes) the
    solve is refused as a bad argument before any launch; where it is computed on the stream without a host round trip
    (the fused fp32 shapes, float64) every code comes back NaN -- never a finite code from a NaN step."""
    from lasso_amd.linear.lipschitz import lipschitz_constant
    _, ista, _, _, _ = _mods()
    for n, d, k in [nf.LINEAR_FUSED[0], nf.LINEAR_GENERAL[0]]:
        X, W, z0, _ = nf.linear_problem(n, d, k, dtype=dtype)
        wp = poison(W, (d - 1, 0), value)
        assert math.isnan(lipschitz_constant(wp.cuda())), (n, d, k)
        if dtype == F32 and (n, d, k) == nf.LINEAR_GENERAL[0]:
            with pytest.raises(ValueError, match="lr"):
                ista(X.cuda(), z0.cuda(), wp.cuda(), nf.ALPHA, lr="auto", maxiter=2, tol=0.0)
            continue
        got = ista(X.cuda(), z0.cuda(), wp.cuda(), nf.ALPHA, lr="auto", maxiter=2, tol=0.0)
        assert classes(got).eq(IS_NAN).all(), (n, d, k)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "f64"])
def test_objectives(dtype):
    from lasso_amd.conv2d.ista import conv_loss
    from lasso_amd.linear.dict_learning import lasso_loss
    _, _, _, _, orc = _mods()
    x, w, z0, lr, st, pd = nf.conv_problem("synth", dtype=dtype)
    z = orc.conv_fista(x, z0, w, nf.ALPHA, padding=pd, maxiter=2, lr=lr, tol=0.0)
    for xs, zs in ((poison(x, (1, 0, 0, 0), NAN), z), (x, poison(z, (1, 0, 0, 0), NAN)),
                   (poison(x, (1, 0, 0, 0), PINF), z), (x, poison(z, (2, 3, 1, 1), nf.NINF))):
        ref = orc.conv_objective(xs, zs, w, nf.ALPHA, st, pd)
        got = conv_loss(xs.cuda(), zs.cuda(), w.cuda(), nf.ALPHA, st, pd)
        assert torch.equal(classes(got), classes(ref)) and not classes(ref).eq(FINITE).any()
    for n, d, k in [nf.LINEAR_FUSED[0], nf.LINEAR_GENERAL[0]]:
        X, W, z0, lr = nf.linear_problem(n, d, k, dtype=dtype)
        Z = orc.fista(X, z0, W, nf.ALPHA, lr=lr, maxiter=2, tol=0.0)
        for xs, zs in ((poison(X, (3, 2), NAN), Z), (X, poison(Z, (3, 2), NAN)), (poison(X, (n - 1, d - 1), nf.NINF), Z),
                       (X, poison(Z, (n - 1, k - 1), PINF))):
            ref = orc.lasso_objective(xs, zs, W, nf.ALPHA)
            got = lasso_loss(xs.cuda(), zs.cuda(), W.cuda(), nf.ALPHA)
            assert torch.equal(classes(got), classes(ref)) and not classes(ref).eq(FINITE).any(), (n, d, k)


# ---- M-steps ------------------------------------------------------------------------------------------------------
def _codes(n, k, dtype):
    g = torch.Generator().manual_seed(5)
    return torch.randn(n, k, generator=g, dtype=dtype) * (torch.rand(n, k, generator=g) < 0.4)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "f64"])
@pytest.mark.parametrize("positive", [False, True], ids=["plain", "positive"])
@pytest.mark.parametrize("n,d,k", nf.MSTEP_SHAPES)
def test_update_dict(n, d, k, positive, dtype):
    """dict_learning.py:85-100: one NaN in Z or X reaches every atom (a NaN in X: feature d - 1 of each update, and the
    atom's norm with it).  clamp_(0, None) keeps it (:87-88) and NaN < eps is False (:92): no atom is replaced."""
    from lasso_amd.linear import update_dict
    _, _, _, _, orc = _mods()
    X, W, _, _ = nf.linear_problem(n, d, k, dtype=dtype)
    Z = _codes(n, k, dtype)
    for what in ("Z", "X"):
        Zp = poison(Z, (n // 2, k // 2), NAN) if what == "Z" else Z
        Xp = poison(X, (n // 2, d - 1), NAN) if what == "X" else X
        ref = orc.update_dict(W.clone(), Xp, Zp.clone(), positive=positive)
        torch.manual_seed(0)
        Dg, Zg = W.clone().cuda(), Zp.clone().cuda()
        got = update_dict(Dg, Xp.cuda(), Zg, positive=positive)
        assert got.data_ptr() == Dg.data_ptr()
        assert torch.equal(classes(got), classes(ref)) and classes(ref).eq(IS_NAN).all(), (what, int(classes(got).eq(FINITE).sum()))
        assert torch.equal(classes(Zg), classes(Zp))                           # no column of Z was zeroed (:98)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "f64"])
@pytest.mark.parametrize("n,d,k", nf.MSTEP_SHAPES)
def test_update_dict_ridge(n, d, k, dtype):
    """dict_learning.py:117-121.  A NaN in X: column d - 1 of Z^T X, so row d - 1 of V, nothing else.  A NaN in Z: the
    Gram matrix cannot be factored and torch.linalg.cholesky raises (:120) -- the HIP path raises the same error."""
    from lasso_amd.linear import update_dict_ridge
    _, _, _, _, orc = _mods()
    X, W, _, _ = nf.linear_problem(n, d, k, dtype=dtype)
    Z = _codes(n, k, dtype)
    Xp = poison(X, (n // 2, d - 1), NAN)
    ref = orc.update_dict_ridge(Xp, Z, lambd=1e-2)
    got = update_dict_ridge(Xp.cuda(), Z.cuda(), lambd=1e-2).cpu()
    assert torch.equal(classes(got), classes(ref)) and classes(ref)[d - 1].eq(IS_NAN).all() and classes(ref)[:d - 1].eq(FINITE).all()
    clean = update_dict_ridge(X.cuda(), Z.cuda(), lambd=1e-2).cpu()
    assert torch.equal(got[:d - 1], clean[:d - 1])                             # the other features: the clean solve's
    bar = 2e-4 if dtype == F32 else 2e-4 * 2.0 ** -29                          # tests/test_dict_learning_gpu.py, test_f64_mstep_gpu.py
    assert (got[:d - 1] - ref[:d - 1]).abs().max().item() <= bar * max(1.0, ref[:d - 1].abs().max().item())
    Zp = poison(Z, (n // 2, k // 2), NAN)
    with pytest.raises(RuntimeError, match="cholesky"):
        orc.update_dict_ridge(X, Zp, lambd=1e-2)
    with pytest.raises(RuntimeError, match="cholesky"):
        update_dict_ridge(X.cuda(), Zp.cuda(), lambd=1e-2)


# ---- autograd -----------------------------------------------------------------------------------------------------
def _backward(fn, tensors, cot, dev):
    leaves = [t.detach().clone().to(dev).requires_grad_(True) for t in tensors]
    z = fn(*leaves)
    z.backward(cot.to(dev))
    return z.detach().cpu(), [t.grad.cpu() for t in leaves]


@pytest.mark.parametrize("T", [1, 6])
def test_autograd_linear(T):
    """NaN in one row of the cotangent, at a coordinate whose code is far from zero (softshrink's backward SELECTS:
    a zero code passes 0 whatever the cotangent -- ATen and bw_prox_kernel alike)"""
    _, ista, _, _, orc = _mods()
    n, d, k = nf.LINEAR_FUSED[0]
    X, W, z0, lr = nf.linear_problem(n, d, k)
    g = torch.Generator().manual_seed(9)
    gz = torch.randn(n, k, generator=g)
    row = 5
    col = int(orc.fista(X, z0, W, nf.ALPHA, lr=lr, maxiter=T, tol=0.0)[row].abs().argmax())
    gzp = poison(gz, (row, col), NAN)
    ref_fn = lambda x, z, w: orc.fista(x, z, w, nf.ALPHA, lr=lr, maxiter=T, tol=0.0)
    hip_fn = lambda x, z, w: ista(x, z, w, nf.ALPHA, lr=lr, maxiter=T, tol=0.0)
    _, (rdx, rdz0, rdw) = _backward(ref_fn, (X, z0, W), gzp, "cpu")
    _, (cdx, cdz0, cdw) = _backward(hip_fn, (X, z0, W), gz, "cuda")
    _, (dx, dz0, dw) = _backward(hip_fn, (X, z0, W), gzp, "cuda")
    assert classes(rdx[row]).eq(IS_NAN).all() and classes(rdz0[row]).eq(IS_NAN).all() and classes(rdw).eq(IS_NAN).all()
    for name, a, c, r in (("dx", dx, cdx, rdx), ("dz0", dz0, cdz0, rdz0)):
        _held(a, c, r, [row], 0.0, (name, T))
    assert torch.equal(classes(dw), classes(rdw))


@pytest.mark.parametrize("T", [1, 6])
def test_autograd_conv(T):
    from lasso_amd.conv2d import ista_conv2d
    _, _, _, _, orc = _mods()
    x, w, z0, lr, st, pd = nf.conv_problem("synth")
    g = torch.Generator().manual_seed(9)
    gz = torch.randn(z0.shape, generator=g)
    kw = dict(stride=st, padding=pd, maxiter=T, lr=lr, tol=0.0)
    zr = orc.conv_fista(x, z0, w, nf.ALPHA, **kw)
    at = int(zr[1].abs().argmax())
    idx = (1,) + tuple(int(v) for v in torch.unravel_index(torch.tensor(at), zr[1].shape))
    gzp = poison(gz, idx, NAN)
    ref_fn = lambda a, b, c: orc.conv_fista(a, b, c, nf.ALPHA, **kw)
    hip_fn = lambda a, b, c: ista_conv2d(a, b, c, nf.ALPHA, **kw)
    _, (rdx, rdz0, rdw) = _backward(ref_fn, (x, z0, w), gzp, "cpu")
    _, (cdx, cdz0, cdw) = _backward(hip_fn, (x, z0, w), gz, "cuda")
    _, (dx, dz0, dw) = _backward(hip_fn, (x, z0, w), gzp, "cuda")
    assert classes(rdx[1]).eq(IS_NAN).any() and classes(rdw).eq(IS_NAN).all()
    for name, a, c, r in (("dx", dx, cdx, rdx), ("dz0", dz0, cdz0, rdz0)):
        bar = 2e-4 * max(r[~r.isnan()].abs().max().item(), 1e-3)               # tests/test_conv_autograd_gpu.py
        _held(a, c, r, [1], bar, (name, T))
    assert torch.equal(classes(dw), classes(rdw))


# ---- patches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("center", [True, False], ids=["centred", "plain"])
def test_patches(center):
    from lasso_amd.patches import extract_patches, reconstruct_from_patches
    F = torch.nn.functional
    g = torch.Generator().manual_seed(2)
    clean_img = torch.randn(2, 1, 9, 10, generator=g)
    img = poison(clean_img, (1, 0, 4, 5), NAN)
    ref = F.unfold(img, 3).transpose(1, 2).reshape(-1, 9)
    ref_mu = ref.mean(1)
    if center:
        ref = ref - ref_mu[:, None]
    X, mu = extract_patches(img.cuda(), 3, center=center)
    Xc, muc = extract_patches(clean_img.cuda(), 3, center=center)
    assert torch.equal(classes(X), classes(ref)) and int(classes(ref).eq(IS_NAN).any(1).sum()) == 9
    keep = ~classes(ref).eq(IS_NAN).any(1)
    assert torch.equal(X.cpu()[keep], Xc.cpu()[keep])                          # the other patches: bitwise the clean image's
    if center:
        assert torch.equal(classes(mu), classes(ref_mu)) and torch.equal(mu.cpu()[keep], muc.cpu()[keep])
    rec = reconstruct_from_patches(X, img.shape, 3, means=mu).cpu()
    cols = (ref + ref_mu[:, None] if center else ref).reshape(2, -1, 9).transpose(1, 2)
    want = F.fold(cols, (9, 10), 3) / F.fold(torch.ones_like(cols), (9, 10), 3)
    assert torch.equal(classes(rec), classes(want))
    assert int(classes(want)[0].ne(FINITE).sum()) == 0 and int(classes(want)[1].eq(IS_NAN).sum()) == (25 if center else 1)
    assert (rec - want)[~want.isnan()].abs().max().item() <= 1e-5               # tests/test_patches_gpu.py
