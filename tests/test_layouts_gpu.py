"""The C-ABI entry points on pitched, odd-pitch and offset operands (include/lasso_hip.h: "matrices are row-major with an
explicit leading dimension in ELEMENTS").  Every Python caller hands the library contiguous torch allocations, so the
vector / scalar forms the kernels choose from the leading dimension and the pointer's alignment, and the strided host
copies (seed_state, the stop rule's save / restore and replay, lasso_fista_run's y copies), are reached here only: the
calls go through nat.lib() with operands placed by tests/layouts.py.

Per call: every operand `natural` once (the anchor); then one operand at a time `pitched`, `odd`, `offset`; then all
operands `odd`, all `offset`.  Asserted for every layout:
  * the result against the CPU oracle / an fp64 reference at the bar the existing suite uses for that entry point;
  * inputs unchanged bit for bit, the padding of inputs and outputs unchanged bit for bit, no NaN in a result (the
    padding of every input is NaN: a result that depends on it shows it);
  * torch.equal with the anchor's result -- the layout changes how operands are fetched, not the arithmetic -- except
    for the cases of _REORDERED, where another kernel with another summation order legitimately runs.
A layout an entry point cannot serve must be refused before anything is enqueued (status + text, operands untouched); the
header documents two such refusals: lasso_fista_solve_sharded with ldz != k, and the lasso_mstep_pipe_* alignment rules.
Measured deviations are recorded through tests/margins.py, one entry per case."""
import ctypes as C

import pytest
import torch

import layouts
from margins import record_margins

pytestmark = pytest.mark.gpu
NAN = float("nan")
Z_BAR = 5e-5                        # max|dz| against the oracle (test_random_shapes_gpu.py)
F64_BAR = 5e-5 * 2.0 ** -29         # 9.3e-14 (test_f64_gpu.py)
LOSS_RTOL, LOSS_RTOL_F64 = 3e-6, 2e-6 * 2.0 ** -29
KERNEL_UNFUSED = 0x300

# (case, layout tag) whose result is NOT bitwise the anchor's: another kernel, another summation order.  These keep the
# reference bar only.  Every other case must reproduce the anchor bit for bit.
_REORDERED = {
    # lasso_gram_accumulate: gram_ab256 / the joint gram_tn128 need 16-byte aligned Z and X with pitches that are
    # multiples of 4 (launch_gram_ab*'s guards, mstep.hip); odd / offset operands fall back to gram_tn*, whose sample
    # splits -- hence the order of the sums over n -- differ
    "gram-ab256": ("z-odd", "x-odd", "all-odd", "z-offset", "x-offset", "all-offset"),
    "gram-tn128": ("z-odd", "x-odd", "all-odd", "z-offset", "x-offset", "all-offset"),
    # (300, 200, 300): k and d are multiples of 4, so the natural and pitched layouts run gram_tn128 too; odd / offset
    # operands take gram_tn_kernel<false> on 32 x 32 blocks
    "gram-fallback": ("z-odd", "x-odd", "all-odd", "z-offset", "x-offset", "all-offset"),
}


def _nat():
    from lasso_amd import _native as nat
    return nat, nat.lib()


def _orc():
    from oracle import lasso_oracle as orc
    return orc


def _problem(n, d, k, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    W = torch.nn.functional.normalize(torch.randn(d, k, generator=g, dtype=dtype), dim=0)
    X = torch.randn(n, d, generator=g, dtype=dtype)
    return X, W


def _sparse(n, k, seed, dtype=torch.float32, density=0.2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, k, generator=g, dtype=dtype) * (torch.rand(n, k, generator=g) < density)


class Refused(Exception):
    def __init__(self, status, text):
        super().__init__("status %d: %s" % (status, text))
        self.status, self.text = status, text


def _ok(status, allow=()):
    nat, L = _nat()
    if status != nat.LASSO_OK and status not in allow:
        raise Refused(status, L.lasso_hip_last_error().decode())
    return status


class Case:
    """operands: [(name, cpu tensor, 'in' | 'out' | 'inout')] ('out': the tensor gives shape and dtype); call(P) -> dict
    of host results (P: name -> layouts.Placed); verify(out, host) -> dict of measured margins (asserts the reference
    bar); refusal(plan) -> None or (status, text) the header documents for that plan.  Which operands the layout matrix
    runs over (the others stay natural) is given where the case is registered."""

    def __init__(self, operands, call, verify, refusal=None):
        self.operands, self.call, self.verify, self.refusal = operands, call, verify, refusal


def _run(case, plan):
    P = {}
    for name, t, role in case.operands:
        lay = plan.get(name, "natural")
        if role == "out":
            P[name] = layouts.place(t, lay, layouts.SENTINEL, "cuda", name, fill=layouts.SENTINEL)
        else:
            P[name] = layouts.place(t, lay, NAN, "cuda", name)
    torch.cuda.synchronize()
    try:
        host = case.call(P)
    except Refused:
        torch.cuda.synchronize()
        for name, _, _ in case.operands:          # a refusal comes before anything is enqueued
            P[name].check(written=False)
        raise
    torch.cuda.synchronize()
    for name, _, role in case.operands:
        P[name].check(written=role != "in")
    out = {name: P[name].view.cpu().clone() for name, _, role in case.operands if role != "in"}
    for name, o in out.items():
        if o.is_floating_point():
            assert not bool(torch.isnan(o).any()), "%s holds NaN: the result depends on memory outside the operands" % name
    return out, host


# ---- the registry: case id -> factory, and the (tag, plan) list over the operands the matrix varies ---------------------------------------------------
_FACTORY, _PLANS, _BUILT, _ANCHOR, _MARGINS = {}, {}, {}, {}, {}


def _register(cid, vary, factory, plans=None):
    assert cid not in _FACTORY
    _FACTORY[cid] = factory
    _PLANS[cid] = plans if plans is not None else layouts.plans(tuple(vary))


def _case(cid):
    if cid not in _BUILT:
        _BUILT[cid] = _FACTORY[cid]()
    return _BUILT[cid]


def _anchor(cid):
    if cid not in _ANCHOR:
        _ANCHOR[cid] = _run(_case(cid), {})
    return _ANCHOR[cid]


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, float) and a != a:
        return b != b
    return a == b


def _check(cid, tag):
    case, plan = _case(cid), dict(_PLANS[cid])[tag]
    expected = case.refusal(plan) if case.refusal else None
    if expected is not None:
        with pytest.raises(Refused) as e:
            _run(case, plan)
        assert (e.value.status, e.value.text) == expected
        return
    if tag == "natural":
        out, host = _anchor(cid)
    else:
        out, host = _run(case, plan)
    margins = case.verify(out, host)
    _MARGINS.setdefault(cid, {})[tag] = margins
    record_margins("layouts_" + cid, _MARGINS[cid])
    if tag != "natural":
        a_out, a_host = _anchor(cid)
        if tag in _REORDERED.get(cid, ()):
            return
        for name in out:
            assert torch.equal(out[name], a_out[name]), "%s differs from the anchor's: max %g" % (
                name, (out[name].double() - a_out[name].double()).abs().max().item())
        for key in host:
            assert _same(host[key], a_host[key]), (key, host[key], a_host[key])


# ---- lasso_fista_solve / _f64 -----------------------------------------------------------------------------------------
def _solve(P, n, d, k, alpha, lr, fast, maxiter, tol=0.0, stop=0, hint=0, backtrack=0, z0="z0", z="z", f64=False,
           dtype=None):
    """one lasso_fista_solve(_f64) on the placed operands; z0: the name of the start (absent from P: NULL)"""
    nat, L = _nat()
    dt = nat.LASSO_F64 if f64 else (nat.LASSO_F32 if dtype is None else dtype)
    real = C.c_double if f64 else C.c_float
    nbytes = L.lasso_fista_workspace_bytes(n, d, k, dt, maxiter, tol, stop if f64 else nat.STOP_GLOBAL, backtrack)
    ws = nat.workspace(torch.device("cuda", torch.cuda.current_device()), nbytes, "layouts")
    iters, last = C.c_int32(-1), real(NAN)
    cap = max(maxiter, 1)
    trials, acc_lr, acc_f = (C.c_int32 * cap)(), (real * cap)(), (real * cap)()
    z0p = P.get(z0)
    args = (nat.ptr(P["x"].view), P["x"].ld, nat.ptr(P["w"].view), P["w"].ld,
            nat.ptr(z0p.view) if z0p is not None else None, z0p.ld if z0p is not None else 0,
            nat.ptr(P[z].view), P[z].ld, n, d, k) + (() if f64 else (dt,)) + (
        float(alpha), float(lr), int(fast), int(maxiter), float(tol), int(stop) | (0 if f64 else int(hint)), int(backtrack),
        1.5, C.byref(iters), C.byref(last), trials, acc_lr, acc_f, None, nat.ptr(ws), ws.numel(),
        nat.stream_ptr(ws.device))
    _ok((L.lasso_fista_solve_f64 if f64 else L.lasso_fista_solve)(*args))
    torch.cuda.synchronize()
    host = dict(iterations=iters.value)
    if tol > 0:
        host["last_delta"] = last.value
    if backtrack:
        host["trials"] = list(trials[:iters.value])
        host["accepted_lr"] = list(acc_lr[:iters.value])
    return host


def _lr(W):
    return 1.0 / max(_orc().lipschitz_constant(W, "exact"), 1e-3)


def _fixed(n, d, k, fast, hint=0, seed=1, name_has=None, tile_of=None):
    def factory():
        nat, L = _nat()
        X, W = _problem(n, d, k, seed)
        lr = _lr(W)
        ref = _orc().fista(X, torch.zeros(n, k), W, 0.2, fast=bool(fast), lr=lr, maxiter=11, tol=0.0)
        if name_has:
            assert name_has in L.lasso_fista_kernel_name(n, d, k, nat.LASSO_F32, 0), L.lasso_fista_kernel_name(n, d, k, nat.LASSO_F32, 0)
        if tile_of:
            # lasso_fista_kernel_name takes no hint.  LASSO_KERNEL_TILE keeps the batch on the tile kernel, whose
            # instantiation <kp, rows> depends on (d, k) alone (pad_k_solve, plan_tiles' rows rule): named here by the
            # unhinted dispatch of a batch large enough to take the tile kernel by itself
            big = L.lasso_fista_kernel_name(1 << 16, d, k, nat.LASSO_F32, 0)
            assert big.startswith(b"lasso::sp::fista_tile_sp_kernel<%d, %d," % tile_of), big

        def call(P):
            return _solve(P, n, d, k, 0.2, lr, fast, 11, hint=hint, z0=None)

        def verify(out, host):
            err = (out["z"] - ref).abs().max().item()
            assert host["iterations"] == 11 and err <= Z_BAR, err
            return dict(max_dz=err)
        return Case([("x", X, "in"), ("w", W, "in"), ("z", torch.zeros(n, k), "out")], call, verify)
    return factory


# The split-k and unfused hints have no name to assert: LASSO_KERNEL_SPLITK at n = 40 is also what the unhinted dispatch
# picks (n < 16 x #CUs), and LASSO_KERNEL_UNFUSED on a fused shape is decoded by solve_impl into solve_generic, the
# path the two shapes beyond 256 x 1024 name as "(unfused)".
for _fast in (1, 0):
    _t = "fista" if _fast else "ista"
    _register("solve-%s-tile16x256" % _t, "xwz", _fixed(40, 256, 1024, _fast, 0x100, tile_of=(1024, 16)))
    _register("solve-%s-tile32x128" % _t, "xwz", _fixed(40, 100, 512, _fast, 0x100, seed=2, tile_of=(512, 32)))
    _register("solve-%s-tile64x64" % _t, "xwz", _fixed(70, 64, 256, _fast, 0x100, seed=3, tile_of=(256, 64)))
    _register("solve-%s-splitk" % _t, "xwz", _fixed(40, 256, 1024, _fast, 0x200))
    _register("solve-%s-hybrid" % _t, "xz", _fixed(4900, 256, 1024, _fast, 0, seed=77, name_has=b"split"))
    _register("solve-%s-unfused-dma" % _t, "xwz", _fixed(70, 320, 1088, _fast, 0, seed=4, name_has=b"unfused"))
    _register("solve-%s-unfused-ragged" % _t, "xwz", _fixed(70, 300, 1100, _fast, 0, seed=5, name_has=b"unfused"))
    _register("solve-%s-unfused-hint" % _t, "xwz", _fixed(40, 256, 1024, _fast, KERNEL_UNFUSED))


def _start(n, k, seed):
    return 0.05 * torch.randn(n, k, generator=torch.Generator().manual_seed(seed))


def _with_z0(n, d, k, hint, seed, alias=False):
    """z0 a tensor of its own in each layout -- or z_out aliasing z0 ("z_out may alias z0")"""
    def factory():
        X, W = _problem(n, d, k, seed)
        lr, z0 = _lr(W), _start(n, k, seed + 100)
        ref = _orc().fista(X, z0, W, 0.2, fast=True, lr=lr, maxiter=11, tol=0.0)

        def call(P):
            return _solve(P, n, d, k, 0.2, lr, 1, 11, hint=hint, z0="z" if alias else "z0")

        def verify(out, host):
            err = (out["z"] - ref).abs().max().item()
            assert host["iterations"] == 11 and err <= Z_BAR, err
            return dict(max_dz=err)
        ops = [("x", X, "in"), ("w", W, "in")] + ([("z", z0, "inout")] if alias else
                                                  [("z0", z0, "in"), ("z", torch.zeros(n, k), "out")])
        return Case(ops, call, verify)
    return factory


def _maxiter0(n, d, k, with_z0):
    """maxiter = 0 (seed_state alone): z_out is z0 exactly, zeros without one"""
    def factory():
        X, W = _problem(n, d, k, 9)
        z0 = _start(n, k, 10)

        def call(P):
            return _solve(P, n, d, k, 0.2, 0.1, 1, 0, z0="z0")

        def verify(out, host):
            assert torch.equal(out["z"], z0 if with_z0 else torch.zeros(n, k)) and host["iterations"] == 0
            return dict(max_dz=0.0)
        ops = [("x", X, "in"), ("w", W, "in")] + ([("z0", z0, "in")] if with_z0 else []) + [("z", z0, "out")]
        return Case(ops, call, verify)
    return factory


_ALIAS_PLANS = [("natural", {}), ("z-pitched", {"z": "pitched"})]
_register("solve-z0-fused", ("x", "w", "z0", "z"), _with_z0(40, 256, 1024, 0, 11))
_register("solve-z0-tile", ("z0", "z"), _with_z0(40, 100, 512, 0x100, 12))
_register("solve-z0-unfused", ("x", "w", "z0", "z"), _with_z0(70, 300, 1100, 0, 13))
_register("solve-z0-alias-fused", "z", _with_z0(40, 256, 1024, 0, 11, alias=True), _ALIAS_PLANS)
_register("solve-z0-alias-unfused", "z", _with_z0(70, 300, 1100, 0, 13, alias=True), _ALIAS_PLANS)
_register("solve-maxiter0-z0", ("z0", "z"), _maxiter0(40, 256, 1024, True))
_register("solve-maxiter0-null", ("z",), _maxiter0(40, 256, 1024, False))


def _stop_rule(n, d, k, fast, stop, seed, maxiter, stop_at=None, tol=None, hint=0, alias=False):
    """tol > 0.  stop_at: the iteration the ORACLE must stop at -- the tolerance is put in the middle (geometric) of the gap
    between that iteration's sum |z - z_next| and the smallest one before it, and the oracle is run again with it: checked
    on the CPU that it stops where the case needs it to."""
    def factory():
        orc = _orc()
        X, W = _problem(n, d, k, seed)
        lr, z0 = _lr(W), _start(n, k, seed + 100)
        t = tol
        if stop_at is not None:
            tr = orc.FistaTrace()
            orc.fista(X, z0, W, 0.4, fast=bool(fast), lr=lr, maxiter=stop_at, tol=0.0, trace=tr)
            here, before = tr.delta[stop_at - 1], min(tr.delta[:stop_at - 1])
            assert here < before * (1 - 1e-3), (here, before)          # room for fp32 sums on either side
            t = (here * before) ** 0.5 / (n * k)
        tr = orc.FistaTrace()
        ref = orc.fista(X, z0, W, 0.4, fast=bool(fast), lr=lr, maxiter=maxiter, tol=t, trace=tr)
        assert tr.stopped and 1 < tr.iterations < maxiter and (stop_at is None or tr.iterations == stop_at), tr.iterations

        def call(P):
            return _solve(P, n, d, k, 0.4, lr, fast, maxiter, tol=t, stop=stop, hint=hint, z0="z" if alias else "z0")

        def verify(out, host):
            err = (out["z"] - ref).abs().max().item()
            assert host["iterations"] == tr.iterations, (host, tr.iterations)
            assert err <= Z_BAR, err
            return dict(max_dz=err, iterations=host["iterations"])
        ops = [("x", X, "in"), ("w", W, "in")] + ([("z", z0, "inout")] if alias else
                                                  [("z0", z0, "in"), ("z", torch.zeros(n, k), "out")])
        return Case(ops, call, verify)
    return factory


_XWZ0Z = ("x", "w", "z0", "z")
_register("stop-in-kernel", _XWZ0Z, _stop_rule(96, 256, 1024, 1, 0, 21, 200, tol=1e-4))
# solve_chunked: chunks of 64 iterations.  Stop at 30: strictly inside the first chunk -> the replay from the chunk's
# head into (z_out, ldz).  Stop at 64 of 200: the last iteration of a chunk that is not the final one -> the chunk's
# compact state is copied into (z_out, ldz) by hipMemcpy2DAsync.
_register("stop-chunked-replay", _XWZ0Z, _stop_rule(96, 256, 1024, 1, 2, 21, 200, stop_at=30))
_register("stop-chunked-chunk-end", _XWZ0Z, _stop_rule(96, 256, 1024, 0, 2, 21, 200, stop_at=64))
_register("stop-chunked-alias", "z", _stop_rule(96, 256, 1024, 1, 2, 21, 200, stop_at=30, alias=True), _ALIAS_PLANS)
_register("stop-unfused", _XWZ0Z, _stop_rule(70, 300, 1100, 1, 0, 22, 200, tol=1e-4))


def _lr_auto(n, d, k, seed):
    """lr = LASSO_LR_AUTO: lambda_max on the stream from W in each layout (span_ok, lipschitz.hip).  The existing
    test_lr_auto_* bar is 1e-4 against the reference's ARPACK step; here the oracle takes the exact 1/lambda_max: 5e-5."""
    def factory():
        nat, _ = _nat()
        X, W = _problem(n, d, k, seed)
        ref = _orc().fista(X, torch.zeros(n, k), W, 0.2, fast=True, lr=_lr(W), maxiter=11, tol=0.0)

        def call(P):
            return _solve(P, n, d, k, 0.2, nat.LR_AUTO, 1, 11, z0=None)

        def verify(out, host):
            err = (out["z"] - ref).abs().max().item()
            assert err <= Z_BAR, err
            return dict(max_dz=err)
        return Case([("x", X, "in"), ("w", W, "in"), ("z", torch.zeros(n, k), "out")], call, verify)
    return factory


_register("lr-auto-256x1024", "w", _lr_auto(40, 256, 1024, 31))
_register("lr-auto-48x160", "w", _lr_auto(40, 48, 160, 32))
_register("lr-auto-300x513", "w", _lr_auto(40, 300, 513, 33))


def _backtrack(n, d, k, fast, seed, maxiter=8):
    """the line search: x, W, z0 in each layout (z_out: test_line_search_into_a_strided_z_out); the oracle's trial trace
    exactly, codes 5e-5"""
    def factory():
        orc = _orc()
        X, W = _problem(n, d, k, seed)
        z0 = _start(n, k, seed + 100)
        tr = orc.FistaTrace()
        ref = orc.fista(X, z0, W, 0.3, fast=bool(fast), lr=1.0, maxiter=maxiter, tol=0.0, backtrack=True, trace=tr)

        def call(P):
            return _solve(P, n, d, k, 0.3, 1.0, fast, maxiter, backtrack=1, z0="z0")

        def verify(out, host):
            err = (out["z"] - ref).abs().max().item()
            assert host["iterations"] == maxiter and host["trials"] == list(tr.trials), (host["trials"], tr.trials)
            assert err <= Z_BAR, err
            return dict(max_dz=err)
        return Case([("x", X, "in"), ("w", W, "in"), ("z0", z0, "in"), ("z", torch.zeros(n, k), "out")], call, verify)
    return factory


_register("backtrack-fista-fused", ("x", "w", "z0"), _backtrack(300, 48, 160, 1, 41))
_register("backtrack-ista-fused", ("x", "w", "z0"), _backtrack(300, 48, 160, 0, 41))
_register("backtrack-fista-generic", ("x", "w", "z0"), _backtrack(70, 300, 1100, 1, 42, maxiter=5))


def _f64(n, d, k, mode, seed):
    """lasso_fista_solve_f64 ("any leading dimension and any 8-byte alignment", gemm_f64.hip)"""
    def factory():
        orc = _orc()
        X, W = _problem(n, d, k, seed, torch.float64)
        lr = _lr(W)
        z0 = _start(n, k, seed + 100).double()
        tr = orc.FistaTrace()
        kw = dict(fixed=dict(maxiter=11, tol=0.0), stop=dict(maxiter=200, tol=1e-4),
                  backtrack=dict(maxiter=6, tol=0.0, backtrack=True))[mode]
        lr0 = 1.0 if mode == "backtrack" else lr
        ref = orc.fista(X, z0, W, 0.3, fast=True, lr=lr0, trace=tr, **kw)
        if mode == "stop":
            assert tr.stopped and 1 < tr.iterations < 200

        def call(P):
            return _solve(P, n, d, k, 0.3, lr0, 1, kw["maxiter"], tol=kw["tol"], backtrack=int(mode == "backtrack"),
                          z0="z0", f64=True)

        def verify(out, host):
            err = (out["z"] - ref).abs().max().item()
            assert host["iterations"] == tr.iterations
            if mode == "backtrack":
                assert host["trials"] == list(tr.trials)
            assert err <= F64_BAR, err
            return dict(max_dz=err)
        return Case([("x", X, "in"), ("w", W, "in"), ("z0", z0, "in"), ("z", torch.zeros(n, k, dtype=torch.float64), "out")],
                    call, verify)
    return factory


for _mode in ("fixed", "stop", "backtrack"):
    _register("f64-%s-33x200x513" % _mode, _XWZ0Z, _f64(33, 200, 513, _mode, 51))
    _register("f64-%s-37x10x50" % _mode, _XWZ0Z, _f64(37, 10, 50, _mode, 52))


# ---- lasso_fista_solve on bf16 tensors ---------------------------------------------------------------------------------
def _bf16(n, d, k, backtrack, hint, seed):
    """bf16 x, W, z0, z_out (leading dimensions in bf16 elements; zvec / z0vec / pvec of the bf16 kernels): the trial trace
    and the code of the anchor call bit for bit (tests/bf16_model.py pins that trace elsewhere), and the objective of the
    code within 2e-3 of the fp32 oracle's on the same bf16-rounded inputs."""
    def factory():
        nat, L = _nat()
        orc = _orc()
        X, W = _problem(n, d, k, seed)
        X, W, z0 = X.bfloat16(), W.bfloat16(), _start(n, k, seed + 100).bfloat16()
        Xf, Wf, z0f = X.float(), W.float(), z0.float()
        lr = 1.0 if backtrack else _lr(Wf)
        maxiter = 8 if backtrack else 11
        ref = orc.fista(Xf, z0f, Wf, 0.3, fast=True, lr=lr, maxiter=maxiter, tol=0.0, backtrack=bool(backtrack))

        def objective(z):
            z = z.double()
            return ((0.5 * (z @ Wf.double().T - Xf.double()).pow(2).sum() + 0.3 * z.abs().sum()) / n).item()
        ref_obj = objective(ref)

        def call(P):
            return _solve(P, n, d, k, 0.3, lr, 1, maxiter, hint=hint, backtrack=backtrack, z0="z0", dtype=nat.LASSO_BF16)

        def verify(out, host):
            rel = abs(objective(out["z"].float()) - ref_obj) / ref_obj
            assert host["iterations"] == maxiter and rel <= 2e-3, (host, rel)
            return dict(objective_rel=rel)
        return Case([("x", X, "in"), ("w", W, "in"), ("z0", z0, "in"), ("z", torch.zeros(n, k, dtype=torch.bfloat16), "out")],
                    call, verify)
    return factory


for _bt in (0, 1):
    _t = "backtrack" if _bt else "fixed"
    _register("bf16-%s-persistent-200x256x1024" % _t, ("x", "w", "z0", "z"), _bf16(200, 256, 1024, _bt, 0, 131))
    _register("bf16-%s-persistent-100x100x512" % _t, ("x", "w", "z0", "z"), _bf16(100, 100, 512, _bt, 0, 132))
    _register("bf16-%s-multi-launch-100x100x512" % _t, ("x", "w", "z0", "z"), _bf16(100, 100, 512, _bt, 0x100, 132))


# ---- lasso_fista_prepare + lasso_fista_run ----------------------------------------------------------------------------
def _prepare_run(n, d, k, seed):
    """two _run calls (5 + 6 iterations of 11): (z_in, NULL) -> (z_mid, y_mid) -> (z_out, y_out); w in each layout too
    (prepare's pack / Wc copy)"""
    def factory():
        nat, L = _nat()
        X, W = _problem(n, d, k, seed)
        lr, z0 = _lr(W), _start(n, k, seed + 100)
        ref = _orc().fista(X, z0, W, 0.2, fast=True, lr=lr, maxiter=11, tol=0.0)

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            ws = nat.workspace(dev, L.lasso_fista_workspace_bytes(n, d, k, nat.LASSO_F32, 11, 0.0, nat.STOP_NONE, 0), "layouts-run")
            st = nat.stream_ptr(dev)
            _ok(L.lasso_fista_prepare(nat.ptr(P["w"].view), P["w"].ld, d, k, nat.LASSO_F32, 11, nat.ptr(ws), ws.numel(), st))

            def run(zi, yi, zo, yo, it0, iters):
                _ok(L.lasso_fista_run(nat.ptr(P["x"].view), P["x"].ld, nat.ptr(P[zi].view), P[zi].ld,
                                      nat.ptr(P[yi].view) if yi else None, P[yi].ld if yi else 0,
                                      nat.ptr(P[zo].view), P[zo].ld, nat.ptr(P[yo].view), P[yo].ld, n, d, k, nat.LASSO_F32,
                                      0.2, lr, 1, it0, iters, 11, 0, None, nat.ptr(ws), ws.numel(), st))
            run("z_in", None, "z_mid", "y_mid", 0, 5)
            run("z_mid", "y_mid", "z_out", "y_out", 5, 6)
            return {}

        def verify(out, host):
            err = (out["z_out"] - ref).abs().max().item()
            assert err <= Z_BAR, err
            return dict(max_dz=err)
        zero = torch.zeros(n, k)
        return Case([("x", X, "in"), ("w", W, "in"), ("z_in", z0, "in"), ("z_mid", zero, "out"), ("y_mid", zero, "out"),
                     ("z_out", zero, "out"), ("y_out", zero, "out")], call, verify)
    return factory


_RUN_OPS = ("w", "z_in", "z_mid", "y_mid", "z_out", "y_out")
_register("prepare-run-fused", _RUN_OPS, _prepare_run(40, 256, 1024, 61))
_register("prepare-run-unfused", _RUN_OPS, _prepare_run(70, 300, 1100, 62))


# ---- lasso_fista_solve_sharded ----------------------------------------------------------------------------------------
def _sharded(n, d, k, seed, maxiter):
    """one rank holding the whole batch (the callback leaves the sums as they are): the single-process line search's
    trace.  The header: "Requires ldz == k" -- any other z_out is LASSO_ERR_UNSUPPORTED, nothing written."""
    def factory():
        nat, L = _nat()
        orc = _orc()
        X, W = _problem(n, d, k, seed)
        z0 = _start(n, k, seed + 100)
        tr = orc.FistaTrace()
        ref = orc.fista(X, z0, W, 0.3, fast=True, lr=1.0, maxiter=maxiter, tol=0.0, backtrack=True, trace=tr)
        cb = nat.ALLREDUCE_FN(lambda ctx, sums, count: 0)

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            ws = nat.workspace(dev, L.lasso_fista_workspace_bytes(n, d, k, nat.LASSO_F32, maxiter, 0.0, nat.STOP_GLOBAL, 1), "layouts")
            iters, last = C.c_int32(-1), C.c_float(NAN)
            trials, acc_lr, acc_f = (C.c_int32 * maxiter)(), (C.c_float * maxiter)(), (C.c_float * maxiter)()
            _ok(L.lasso_fista_solve_sharded(
                nat.ptr(P["x"].view), P["x"].ld, nat.ptr(P["w"].view), P["w"].ld, nat.ptr(P["z0"].view), P["z0"].ld,
                nat.ptr(P["z"].view), P["z"].ld, n, n, d, k, nat.LASSO_F32, 0.3, 1.0, 1, maxiter, 0.0, 1.5, cb, None,
                C.byref(iters), C.byref(last), trials, acc_lr, acc_f, nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)))
            return dict(iterations=iters.value, trials=list(trials[:iters.value]), accepted_lr=list(acc_lr[:iters.value]))

        def verify(out, host):
            err = (out["z"] - ref).abs().max().item()
            assert host["iterations"] == maxiter and host["trials"] == list(tr.trials), (host["trials"], tr.trials)
            assert err <= Z_BAR, err
            return dict(max_dz=err)

        def refusal(plan):
            if plan.get("z", "natural") != "natural":                # every other layout has ldz != k
                return nat.LASSO_ERR_UNSUPPORTED, "row-sharded line search needs ldz == k"
            return None
        return Case([("x", X, "in"), ("w", W, "in"), ("z0", z0, "in"), ("z", torch.zeros(n, k), "out")], call, verify,
                    refusal)
    return factory


_register("sharded-fused", _XWZ0Z, _sharded(300, 48, 160, 71, 6))


# ---- lasso_objective / _throttled / _f64 ------------------------------------------------------------------------------
def _objective(n, d, k, form, seed):
    def factory():
        nat, L = _nat()
        f64 = form == "f64"
        dt = torch.float64 if f64 else torch.float32
        X, W = _problem(n, d, k, seed, dt)
        Z = _sparse(n, k, seed + 1, dt)
        X64, W64, Z64 = X.double(), W.double(), Z.double()
        rr, l1 = (Z64 @ W64.T - X64).pow(2).sum().item(), Z64.abs().sum().item()
        ref = (0.5 * rr + 0.7 * l1) / n

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            loss = torch.full((), NAN, dtype=dt, device=dev)
            sums = torch.full((2,), NAN, dtype=torch.float64, device=dev)
            nb = (L.lasso_objective_f64_workspace_bytes if f64 else L.lasso_objective_workspace_bytes)(n, d, k)
            ws = nat.workspace(dev, nb, "layouts-obj")
            head = (nat.ptr(P["x"].view), P["x"].ld, nat.ptr(P["w"].view), P["w"].ld, nat.ptr(P["z"].view), P["z"].ld, n, d, k)
            tail = (nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
            if f64:
                _ok(L.lasso_objective_f64(*head, 0.7, nat.ptr(loss), nat.ptr(sums), *tail))
            elif form == "throttled":
                _ok(L.lasso_objective_throttled(*head, nat.LASSO_F32, 0.7, nat.ptr(loss), nat.ptr(sums), 2, *tail))
            else:
                _ok(L.lasso_objective(*head, nat.LASSO_F32, 0.7, nat.ptr(loss), nat.ptr(sums), *tail))
            torch.cuda.synchronize()
            return dict(loss=loss.item(), rr=sums[0].item(), l1=sums[1].item())

        def verify(out, host):
            rtol = LOSS_RTOL_F64 if f64 else LOSS_RTOL
            err = abs(host["loss"] - ref) / abs(ref)
            assert err <= rtol, (host, ref)
            assert abs(host["rr"] - rr) <= rtol * rr and abs(host["l1"] - l1) <= rtol * l1, (host, rr, l1)
            return dict(loss_rel=err)
        return Case([("x", X, "in"), ("w", W, "in"), ("z", Z, "in")], call, verify)
    return factory


for _form in ("plain", "throttled", "f64"):
    _register("objective-%s-tile" % _form, "xwz", _objective(50, 256, 1024, _form, 81))
    _register("objective-%s-generic-small" % _form, "xwz", _objective(50, 48, 160, _form, 82))
    _register("objective-%s-generic-large" % _form, "xwz", _objective(50, 300, 1100, _form, 83))


# ---- lasso_lipschitz --------------------------------------------------------------------------------------------------
def _lipschitz(d, k, f64):
    def factory():
        nat, L = _nat()
        W = torch.randn(d, k, generator=torch.Generator().manual_seed(d + k), dtype=torch.float64 if f64 else torch.float32)
        ref = _orc().lipschitz_constant(W, "exact")

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            ws = nat.workspace(dev, L.lasso_lipschitz_workspace_bytes(d, k), "layouts-lip")
            out = C.c_double(NAN)
            _ok(L.lasso_lipschitz(nat.ptr(P["w"].view), P["w"].ld, d, k, nat.LASSO_F64 if f64 else nat.LASSO_F32,
                                  C.byref(out), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)))
            return dict(lambda_max=out.value)

        def verify(out, host):
            err = abs(host["lambda_max"] - ref) / ref
            assert err <= 2e-6, (host, ref)
            return dict(rel=err)
        return Case([("w", W, "in")], call, verify)
    return factory


for _d, _k in ((48, 160), (200, 513), (300, 513), (513, 300)):
    _register("lipschitz-f32-%dx%d" % (_d, _k), "w", _lipschitz(_d, _k, False))
    _register("lipschitz-f64-%dx%d" % (_d, _k), "w", _lipschitz(_d, _k, True))


# ---- lasso_init_transpose ---------------------------------------------------------------------------------------------
def _init_transpose(n, d, k, f64):
    def factory():
        nat, L = _nat()
        dt = torch.float64 if f64 else torch.float32
        X, W = _problem(n, d, k, n + d, dt)
        ref = X.double() @ W.double()
        bound = d * (2.0 ** -53 if f64 else 2.0 ** -24) * (X.double().abs() @ W.double().abs())

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            ws = nat.workspace(dev, L.lasso_init_transpose_workspace_bytes(d, k), "layouts-init")
            _ok(L.lasso_init_transpose(n, d, k, nat.LASSO_F64 if f64 else nat.LASSO_F32, nat.ptr(P["x"].view), P["x"].ld,
                                       nat.ptr(P["w"].view), P["w"].ld, nat.ptr(P["z"].view), P["z"].ld, nat.ptr(ws),
                                       ws.numel(), nat.stream_ptr(dev)))
            return {}

        def verify(out, host):
            err = (out["z"].double() - ref).abs()
            ratio = (err / bound.clamp_min(1e-300)).max().item()
            assert bool((err <= bound).all()), ratio
            return dict(worst_error_over_bound=ratio)
        return Case([("x", X, "in"), ("w", W, "in"), ("z", torch.zeros(n, k, dtype=dt), "out")], call, verify)
    return factory


for _n, _d, _k in ((37, 10, 50), (33, 200, 513), (20, 784, 1100)):
    _register("init-transpose-f32-%dx%dx%d" % (_n, _d, _k), "xwz", _init_transpose(_n, _d, _k, False))
    _register("init-transpose-f64-%dx%dx%d" % (_n, _d, _k), "xwz", _init_transpose(_n, _d, _k, True))


# ---- lasso_gram_accumulate (+ _signal, _f64) --------------------------------------------------------------------------
def _gram(n, d, k, form, seed):
    def factory():
        nat, L = _nat()
        f64 = form == "f64"
        dt = torch.float64 if f64 else torch.float32
        Z = _sparse(n, k, seed, dt, 0.15)
        X = torch.randn(n, d, generator=torch.Generator().manual_seed(seed + 1), dtype=dt)
        Ar, Br = Z.double().T @ Z.double(), Z.double().T @ X.double()

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            A = torch.full((k, k), NAN, dtype=dt, device=dev)
            B = torch.full((k, d), NAN, dtype=dt, device=dev)
            nb = (L.lasso_gram_f64_workspace_bytes if f64 else L.lasso_gram_workspace_bytes)(n, d, k)
            ws = nat.workspace(dev, nb, "layouts-gram")
            head = (nat.ptr(P["z"].view), P["z"].ld, nat.ptr(P["x"].view), P["x"].ld, n, d, k)
            tail = (nat.ptr(A), nat.ptr(B), nat.ptr(ws), ws.numel())
            host = {}
            if f64:
                _ok(L.lasso_gram_accumulate_f64(*head, *tail, nat.stream_ptr(dev)))
            elif form == "signal":
                word = torch.zeros(1, dtype=torch.int32, device=dev)
                _ok(L.lasso_gram_accumulate_signal(*head, nat.LASSO_F32, *tail, nat.ptr(word), 7, nat.stream_ptr(dev)))
                torch.cuda.synchronize()
                host["started"] = int(word.item())
            else:
                _ok(L.lasso_gram_accumulate(*head, nat.LASSO_F32, *tail, nat.stream_ptr(dev)))
            torch.cuda.synchronize()
            host["A"], host["B"] = A.cpu(), B.cpu()
            return host

        def verify(out, host):
            A, B = host["A"], host["B"]
            assert not bool(torch.isnan(A).any()) and not bool(torch.isnan(B).any())
            assert torch.equal(A, A.T)
            bar = 2e-6 * 2.0 ** -29 if f64 else 2e-6
            ea = ((A.double() - Ar).abs().max() / Ar.abs().max()).item()
            eb = ((B.double() - Br).abs().max() / Br.abs().max()).item()
            assert ea <= bar and eb <= bar and host.get("started", 7) == 7, (ea, eb, host.get("started"))
            return dict(A_rel=ea, B_rel=eb)
        return Case([("z", Z, "in"), ("x", X, "in")], call, verify)
    return factory


_register("gram-ab256", "zx", _gram(4096, 256, 256, "plain", 91))
_register("gram-tn128", "zx", _gram(600, 64, 256, "plain", 92))
_register("gram-fallback", "zx", _gram(300, 200, 300, "plain", 93))
_register("gram-signal-tn128", "zx", _gram(600, 64, 256, "signal", 92))
_register("gram-f64", "zx", _gram(300, 200, 300, "f64", 93))
_REORDERED["gram-signal-tn128"] = _REORDERED["gram-tn128"]


# ---- lasso_ridge_solve (+ _f64) ---------------------------------------------------------------------------------------
def _ridge(d, k, f64):
    def factory():
        nat, L = _nat()
        dt = torch.float64 if f64 else torch.float32
        n = 4 * k
        Z, X = _sparse(n, k, k, torch.float64), torch.randn(n, d, generator=torch.Generator().manual_seed(k + 1), dtype=torch.float64)
        A, B = (Z.T @ Z).to(dt), (Z.T @ X).to(dt)
        A = ((A + A.T) / 2).contiguous()
        lam = 1e-2 * n
        M = A.double().clone()
        M.diagonal().add_(lam)
        ref = torch.cholesky_solve(B.double(), torch.linalg.cholesky(M)).T

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            Ag, Bg = A.to(dev), B.to(dev)
            nb = (L.lasso_ridge_f64_workspace_bytes if f64 else L.lasso_ridge_workspace_bytes)(d, k)
            ws = nat.workspace(dev, nb, "layouts-ridge")
            info = C.c_int32(-1)
            if f64:
                _ok(L.lasso_ridge_solve_f64(nat.ptr(Ag), nat.ptr(Bg), nat.ptr(P["v"].view), P["v"].ld, d, k, lam, C.byref(info),
                                            nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)))
            else:
                _ok(L.lasso_ridge_solve(nat.ptr(Ag), nat.ptr(Bg), nat.ptr(P["v"].view), P["v"].ld, d, k, nat.LASSO_F32, lam,
                                        C.byref(info), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)))
            torch.cuda.synchronize()
            assert torch.equal(Ag.cpu(), A) and torch.equal(Bg.cpu(), B)
            return dict(info=info.value)

        def verify(out, host):
            err = (out["v"].double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
            assert host["info"] == 0 and err <= (2e-4 * 2.0 ** -29 if f64 else 2e-5), err      # (f64: test_f64_mstep_gpu.py's bar)
            return dict(rel=err)
        return Case([("v", torch.zeros(d, k, dtype=dt), "out")], call, verify)
    return factory


for _k in (100, 513):
    _register("ridge-f32-k%d" % _k, "v", _ridge(48, _k, False))
    _register("ridge-f64-k%d" % _k, "v", _ridge(48, _k, True))


# ---- lasso_dict_fill_degenerate, lasso_zero_columns (+ _f64) ----------------------------------------------------------
def _fill_degenerate(f64, positive):
    d, k, rows = 37, 50, 5
    def factory():
        nat, L = _nat()
        dt = torch.float64 if f64 else torch.float32
        g = torch.Generator().manual_seed(5)
        D, pool = torch.randn(d, k, generator=g, dtype=dt), torch.randn(rows, d, generator=g, dtype=dt)
        flags = torch.zeros(k, dtype=torch.int32)
        flagged = [3, 17, 18, 49]
        flags[flagged] = 1
        def unit(v):
            """the kernel's arithmetic (fill_degenerate_kernel, mstep.hip / mstep_f64.hip; d <= 256: one element per
            thread): squares in 256 slots, folded pairwise 128, 64, ... 1; fp32 multiplies by 1 / sqrt, double divides"""
            sh = torch.zeros(256, dtype=dt)
            sh[:d] = v * v
            half = 128
            while half:
                sh[:half] = sh[:half] + sh[half:2 * half]
                half //= 2
            return v / sh[0].sqrt() if f64 else v * (1.0 / sh[0].sqrt())
        ref = D.clone()
        for i, j in enumerate(flagged):
            ref[:, j] = unit(pool[i].clamp_min(0) if positive else pool[i])

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            fl = flags.to(dev)
            if f64:
                _ok(L.lasso_dict_fill_degenerate_f64(nat.ptr(P["d"].view), P["d"].ld, d, k, nat.ptr(fl), nat.ptr(P["pool"].view),
                                                     rows, P["pool"].ld, positive, nat.stream_ptr(dev)))
            else:
                _ok(L.lasso_dict_fill_degenerate(nat.ptr(P["d"].view), P["d"].ld, d, k, nat.LASSO_F32, nat.ptr(fl),
                                                 nat.ptr(P["pool"].view), rows, P["pool"].ld, positive, nat.stream_ptr(dev)))
            return {}

        def verify(out, host):
            err = (out["d"] - ref).abs().max().item()
            assert torch.equal(out["d"], ref), err              # exact: untouched atoms, and the replaced ones bit for bit
            return dict(max_err=err)
        return Case([("d", D, "inout"), ("pool", pool, "in")], call, verify)
    return factory


def _zero_columns(f64):
    n, k = 33, 50
    def factory():
        nat, L = _nat()
        dt = torch.float64 if f64 else torch.float32
        Z = torch.randn(n, k, generator=torch.Generator().manual_seed(6), dtype=dt)
        flags = torch.zeros(k, dtype=torch.int32)
        flags[[0, 7, 31, 49]] = 1
        ref = Z.clone()
        ref[:, flags != 0] = 0

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            fl = flags.to(dev)
            if f64:
                _ok(L.lasso_zero_columns_f64(nat.ptr(P["z"].view), P["z"].ld, n, k, nat.ptr(fl), nat.stream_ptr(dev)))
            else:
                _ok(L.lasso_zero_columns(nat.ptr(P["z"].view), P["z"].ld, n, k, nat.LASSO_F32, nat.ptr(fl), nat.stream_ptr(dev)))
            return {}

        def verify(out, host):
            assert torch.equal(out["z"], ref)
            return dict(max_err=0.0)
        return Case([("z", Z, "inout")], call, verify)
    return factory


for _f in (False, True):
    _register("fill-degenerate-%s" % ("f64" if _f else "f32"), ("d", "pool"), _fill_degenerate(_f, 0))
    _register("fill-degenerate-positive-%s" % ("f64" if _f else "f32"), ("d", "pool"), _fill_degenerate(_f, 1))
    _register("zero-columns-%s" % ("f64" if _f else "f32"), "z", _zero_columns(_f))


# ---- lasso_cd_solve, lasso_cd_prepare / _run / _finish ----------------------------------------------------------------
def _cd(n, d, k, seed, split):
    """15 steps against the oracle (test_cd_random_shapes): the code, and the tracked z the reference leaves in z0.
    split: prepare / run / finish with the tracked z written to a tensor of its own (z_track_out)"""
    def factory():
        nat, L = _nat()
        orc = _orc()
        X, W = _problem(n, d, k, seed)
        z0 = _start(n, k, seed + 100)
        track = z0.clone()
        ref = orc.coordinate_descent(X, W, track, 0.3, maxiter=15)           # (updates `track` in place)

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            ws = nat.workspace(dev, L.lasso_cd_workspace_bytes(n, d, k, nat.LASSO_F32), "layouts-cd")
            wsp, st = (nat.ptr(ws), ws.numel()), nat.stream_ptr(dev)
            xw = (nat.ptr(P["x"].view), P["x"].ld, nat.ptr(P["w"].view), P["w"].ld, nat.ptr(P["z0"].view), P["z0"].ld)
            act, steps = C.c_int32(-1), C.c_int32(-1)
            if split:
                _ok(L.lasso_cd_prepare(*xw, n, d, k, nat.LASSO_F32, *wsp, st))
                _ok(L.lasso_cd_run(n, d, k, 0.3, 1e-6 * k, 15, C.byref(act), C.byref(steps), *wsp, st))
                _ok(L.lasso_cd_finish(nat.ptr(P["z"].view), P["z"].ld, nat.ptr(P["zt"].view), P["zt"].ld, n, d, k, 0.3, *wsp, st))
            else:
                _ok(L.lasso_cd_solve(*xw, nat.ptr(P["z"].view), P["z"].ld, n, d, k, nat.LASSO_F32, 0.3, 15, 1e-6,
                                     C.byref(act), C.byref(steps), *wsp, st))
            return dict(n_active=act.value, max_steps=steps.value)

        def verify(out, host):
            err = (out["z"] - ref).abs().max().item()
            err_t = (out["zt" if split else "z0"] - track).abs().max().item()
            assert err <= Z_BAR and err_t <= Z_BAR and host["max_steps"] == 15, (err, err_t, host)
            return dict(max_dz=err, max_dz_tracked=err_t)
        zero = torch.zeros(n, k)
        ops = [("x", X, "in"), ("w", W, "in"), ("z0", z0, "in" if split else "inout"), ("z", zero, "out")]
        return Case(ops + ([("zt", zero, "out")] if split else []), call, verify)
    return factory


_register("cd-solve-30x200x513", _XWZ0Z, _cd(30, 200, 513, 101, False))
_register("cd-solve-30x48x3000", _XWZ0Z, _cd(30, 48, 3000, 102, False))
_register("cd-split-30x200x513", _XWZ0Z + ("zt",), _cd(30, 200, 513, 101, True))
_register("cd-split-30x48x3000", _XWZ0Z + ("zt",), _cd(30, 48, 3000, 102, True))


# ---- lasso_dict_sweep, _async_to, _f64 ---------------------------------------------------------------------------------
def _sweep(n, d, k, form, seed, dead=2):
    """the atom sweep on (A, B) of a sparse code with `dead` unused atoms (replaced by pool rows in atom order; float64:
    flagged and left zero): D, and the output of the out-of-place form, in each layout -- bitwise the anchor's dictionary,
    flags and count, the oracle's Gram-form sweep within 1e-4 (test_update_dict_random_shapes)."""
    def factory():
        nat, L = _nat()
        orc = _orc()
        f64 = form == "f64"
        dt = torch.float64 if f64 else torch.float32
        g = torch.Generator().manual_seed(seed)
        Z = _sparse(n, k, seed + 1, torch.float64)
        gone = sorted(torch.randperm(k, generator=g)[:dead].tolist())
        Z[:, gone] = 0
        X = torch.randn(n, d, generator=g, dtype=torch.float64)
        A, B = (Z.T @ Z).to(dt).contiguous(), (Z.T @ X).to(dt).contiguous()
        D = torch.nn.functional.normalize(torch.randn(d, k, generator=g, dtype=dt), dim=0)
        pool = torch.randn(max(dead, 1), d, generator=g, dtype=dt)
        order = {j: i for i, j in enumerate(gone)}
        ref, ref_mask = orc.update_dict_gram(D.clone(), A.clone(), B.clone(), fresh_atom=lambda j: pool[order[j]].clone())
        assert ref_mask.nonzero().flatten().tolist() == gone

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            Ag, Bg = A.to(dev), B.to(dev)
            nb = (L.lasso_dict_sweep_f64_workspace_bytes if f64 else L.lasso_dict_sweep_workspace_bytes)(d, k)
            ws = nat.workspace(dev, nb, "layouts-sweep")
            flags = torch.full((k,), -1, dtype=torch.int32, device=dev)
            ndeg = C.c_int32(-1)
            tail = (nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
            if f64:
                _ok(L.lasso_dict_sweep_f64(nat.ptr(Ag), nat.ptr(Bg), nat.ptr(P["d"].view), P["d"].ld, d, k, 1e-10, 0,
                                           nat.ptr(flags), C.byref(ndeg), *tail))
                count = ndeg.value
            elif form == "to":
                words = nat.HostWords(2)
                _ok(L.lasso_dict_sweep_async_to(nat.ptr(Ag), nat.ptr(Bg), nat.ptr(P["d"].view), P["d"].ld, nat.ptr(P["out"].view),
                                                P["out"].ld, d, k, nat.LASSO_F32, 1e-10, 0, nat.ptr(P["pool"].view), pool.shape[0],
                                                P["pool"].ld, 0, nat.ptr(flags), words.arm(), None, 0, *tail))
                torch.cuda.synchronize()
                count = int(words.wait(10.0)[0])
            else:
                _ok(L.lasso_dict_sweep(nat.ptr(Ag), nat.ptr(Bg), nat.ptr(P["d"].view), P["d"].ld, d, k, nat.LASSO_F32, 1e-10, 0,
                                       nat.ptr(P["pool"].view), pool.shape[0], P["pool"].ld, 0, nat.ptr(flags), C.byref(ndeg), *tail))
                count = ndeg.value
            torch.cuda.synchronize()
            assert torch.equal(Ag.cpu(), A) and torch.equal(Bg.cpu(), B)
            return dict(count=count, flags=flags.cpu())

        def verify(out, host):
            got = out["out" if form == "to" else "d"]
            assert host["count"] == dead and host["flags"].nonzero().flatten().tolist() == gone, host
            keep = torch.ones(k, dtype=torch.bool)
            if f64:                          # flagged atoms leave the model: zero columns until fill_degenerate
                keep[gone] = False
                assert not bool(got[:, gone].any())
            err = (got - ref)[:, keep].abs().max().item()
            assert err <= (1e-4 * 2.0 ** -29 if f64 else 1e-4), err
            return dict(max_dD=err)
        if f64:
            ops = [("d", D, "inout")]
        elif form == "to":
            ops = [("d", D, "in"), ("out", torch.zeros(d, k), "out"), ("pool", pool, "in")]
        else:
            ops = [("d", D, "inout"), ("pool", pool, "in")]
        return Case(ops, call, verify)
    return factory


for _tag, (_n, _d, _k) in (("one-workgroup", (1024, 48, 200)), ("persist", (2048, 256, 512)), ("multi-launch", (1024, 300, 320))):
    _register("sweep-%s" % _tag, ("d", "pool"), _sweep(_n, _d, _k, "plain", 111))
    _register("sweep-to-%s" % _tag, ("d", "out", "pool"), _sweep(_n, _d, _k, "to", 111))
    _register("sweep-f64-%s" % _tag, ("d",), _sweep(_n, _d, _k, "f64", 111))


# ---- lasso_patches_extract / _reconstruct -----------------------------------------------------------------------------
def _patches(center):
    N, Cc, H, W, ph, pw, sh, sw = 2, 3, 17, 21, 5, 3, 2, 3
    def factory():
        nat, L = _nat()
        F = torch.nn.functional
        img = torch.rand(N, Cc, H, W, generator=torch.Generator().manual_seed(H))
        u = F.unfold(img, (ph, pw), stride=(sh, sw))
        ref = u.transpose(1, 2).reshape(-1, u.shape[1])
        M, cols = ref.shape
        mean = ref.mean(1)
        want_p = ref - mean[:, None] if center else ref
        c3 = ref.reshape(N, -1, cols).transpose(1, 2)
        num, den = F.fold(c3, (H, W), (ph, pw), stride=(sh, sw)), F.fold(torch.ones_like(c3), (H, W), (ph, pw), stride=(sh, sw))
        want_img = torch.where(den > 0, num / den.clamp(min=1), torch.zeros_like(num))

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            ig = img.to(dev)
            means = torch.full((M,), NAN, device=dev) if center else None
            rec = torch.full((N, Cc, H, W), NAN, device=dev)
            st = nat.stream_ptr(dev)
            _ok(L.lasso_patches_extract(nat.ptr(ig), nat.ptr(P["p"].view), P["p"].ld, nat.ptr(means), N, Cc, H, W, ph, pw, sh, sw,
                                        int(center), st))
            _ok(L.lasso_patches_reconstruct(nat.ptr(P["p"].view), P["p"].ld, nat.ptr(means), nat.ptr(rec), N, Cc, H, W, ph, pw, sh,
                                            sw, st))
            torch.cuda.synchronize()
            return dict(rec=rec.cpu(), means=means.cpu() if center else None)

        def verify(out, host):
            e_p = (out["p"] - want_p).abs().max().item()
            e_r = (host["rec"] - want_img).abs().max().item()
            if center:
                assert (host["means"] - mean).abs().max().item() <= 1e-6 and e_p <= 1e-6, e_p
            else:
                assert torch.equal(out["p"], ref)
            assert e_r <= 1e-5, e_r
            return dict(patches=e_p, image=e_r)
        return Case([("p", torch.zeros(M, cols), "out")], call, verify)
    return factory


_register("patches-plain", ("p",), _patches(False))
_register("patches-centred", ("p",), _patches(True))


# ---- lasso_fista_backward(_steps) -------------------------------------------------------------------------------------
def _backward(n, d, k, seed, steps_form):
    """the reverse pass given the iterates z_0 .. z_T (here the oracle's, so that the test does not depend on a forward
    solve), x and W in each layout; torch.autograd through the oracle's loop, 2e-4 of each gradient's largest entry"""
    T = 5
    def factory():
        nat, L = _nat()
        orc = _orc()
        X, W = _problem(n, d, k, seed)
        g = torch.Generator().manual_seed(seed + 1)
        Z0, G = 0.05 * torch.randn(n, k, generator=g), torch.randn(n, k, generator=g)
        lr = _lr(W)
        trace = torch.stack([orc.fista(X, Z0, W, 0.3, fast=True, lr=lr, maxiter=t, tol=0.0) for t in range(T + 1)]).contiguous()
        x, w, z0 = (t.clone().requires_grad_(True) for t in (X, W, Z0))
        (orc.fista(x, z0, w, 0.3, fast=True, lr=lr, maxiter=T, tol=0.0) * G).sum().backward()
        ref = dict(gx=x.grad, gw=w.grad, gz0=z0.grad)

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            ws = nat.workspace(dev, L.lasso_fista_backward_workspace_bytes(n, d, k), "layouts-bw")
            tr, Gg = trace.to(dev), G.to(dev)
            out = {key: torch.full(shape, NAN, device=dev) for key, shape in (("gx", (n, d)), ("gw", (d, k)), ("gz0", (n, k)))}
            head = (nat.ptr(P["x"].view), P["x"].ld, nat.ptr(P["w"].view), P["w"].ld, nat.ptr(tr), nat.ptr(Gg), n, d, k, nat.LASSO_F32)
            tail = (nat.ptr(out["gx"]), nat.ptr(out["gw"]), nat.ptr(out["gz0"]), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
            if steps_form:
                _ok(L.lasso_fista_backward_steps(*head, 1.0, (C.c_float * T)(*([lr] * T)), 1, T, *tail))
            else:
                _ok(L.lasso_fista_backward(*head, lr, 1, T, *tail))
            torch.cuda.synchronize()
            return {key: v.cpu() for key, v in out.items()}

        def verify(out, host):
            m = {}
            for key, r in ref.items():
                assert not bool(torch.isnan(host[key]).any()), key
                m[key] = (host[key] - r).abs().max().item() / max(r.abs().max().item(), 1e-3)
                assert m[key] <= 2e-4, (key, m[key])
            return m
        return Case([("x", X, "in"), ("w", W, "in")], call, verify)
    return factory


_register("backward-40x64x256", "xw", _backward(40, 64, 256, 121, False))
_register("backward-30x300x1100", "xw", _backward(30, 300, 1100, 122, False))
_register("backward-steps-40x64x256", "xw", _backward(40, 64, 256, 121, True))
_register("backward-steps-30x300x1100", "xw", _backward(30, 300, 1100, 122, True))


# ---- lasso_gpsr_solve -------------------------------------------------------------------------------------------------
def _gpsr(name):
    """a case of tests/gpsr_cases.py (golden: tests/golden/gpsr_cases.npz) through the C ABI: the assertions of
    test_gpsr_gpu.py (gpsr_cases.check_against_golden) at its bar (gpsr_cases.z_bar)"""
    def factory():
        import os
        import numpy as np
        import gpsr_cases
        from lasso_amd.linear.solvers.gpsr import _KW_DEFAULTS
        nat, L = _nat()
        spec = gpsr_cases.CASES[name]
        n, d, k, tau = spec["n"], spec["d"], spec["k"], spec["alpha"]
        X, W, z0 = gpsr_cases.case_inputs(spec)
        gold = gpsr_cases.load_case(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpsr_cases.npz"),
                                            allow_pickle=False), name)
        kw = dict(stop_criterion=3, tol=1e-2, maxiter=1000, miniter=5, continuation=False, debias=False)
        opt = dict(_KW_DEFAULTS)
        for key, v in spec["kwargs"].items():
            (kw if key in kw else opt)[key] = v
        bar = gpsr_cases.z_bar(X, W, tau, x0=z0, **spec["kwargs"])[0]

        def call(P):
            dev = torch.device("cuda", torch.cuda.current_device())
            cap = kw["maxiter"] + 2
            dcap = max(int(opt["maxiter_debias"]), int(opt["miniter_debias"])) + 2 if kw["debias"] else 0
            f32, i32 = (lambda c: (C.c_float * max(c, 1))()), (lambda c: (C.c_int32 * max(c, 1))())
            lam, lam0, obj, crit, trials, nz = f32(cap), f32(cap), f32(cap), f32(cap), i32(cap), i32(cap)
            s_tau, s_f0, s_nz0, s_end, db_rr, db_conv = (C.c_double * 1)(), f32(1), i32(1), i32(1), f32(dcap), f32(dcap)
            trace = nat.GpsrTrace(cap, lam, lam0, trials, obj, crit, nz, 1, s_tau, s_f0, s_nz0, s_end, dcap, db_rr, db_conv)
            options = nat.GpsrOptions(kw["stop_criterion"], kw["maxiter"], kw["miniter"], 0, 0, int(kw["debias"]), 1,
                                      int(opt["maxiter_debias"]), int(opt["miniter_debias"]), 0, float(kw["tol"]), float(opt["mu"]),
                                      float(opt["lambda_backtrack"]), -1.0, float(opt["tol_debias"]))
            res = nat.GpsrResult()
            res.trace = C.pointer(trace)
            ws = nat.workspace(dev, L.lasso_gpsr_workspace_bytes(n, d, k, nat.LASSO_F32), "layouts-gpsr")
            z0p = P.get("z0")
            _ok(L.lasso_gpsr_solve(nat.ptr(P["x"].view), P["x"].ld, nat.ptr(P["w"].view), P["w"].ld,
                                   nat.ptr(z0p.view) if z0p else None, z0p.ld if z0p else 0, nat.ptr(P["z"].view), P["z"].ld,
                                   n, d, k, nat.LASSO_F32, float(tau), C.byref(options), C.byref(res), nat.ptr(ws), ws.numel(),
                                   nat.stream_ptr(dev)))
            its = min(res.n_iter - res.db_iters, cap)
            return dict(iterations=res.n_iter, objective=list(obj[:its]), accepted_lambda=list(lam[:its]),
                        trials=list(trials[:its]), criterion=list(crit[:its]), final_objective=res.objective, flags=res.flags)

        def verify(out, host):
            assert host["flags"] == 0, host["flags"]
            dz = gpsr_cases.check_against_golden(name, out["z"], host, gold, bar, [])
            return dict(max_dz=dz, bar=bar)
        ops = [("x", X, "in"), ("w", W, "in")] + ([("z0", z0, "in")] if z0 is not None else []) + [("z", torch.zeros(n, k), "out")]
        return Case(ops, call, verify)
    return factory


_register("gpsr-default", "xwz", _gpsr("default"))
_register("gpsr-debias", "xwz", _gpsr("debias"))
_register("gpsr-warm", ("x", "w", "z0", "z"), _gpsr("warm"))


# ---- the matrix -------------------------------------------------------------------------------------------------------
def _order(tag):           # natural and pitched first, offset last (a fault met on an offset case leaves the others run)
    return 0 if tag == "natural" else 1 if "pitched" in tag else 2 if "odd" in tag else 3


_PARAMS = sorted(((cid, tag) for cid in _FACTORY for tag, _ in _PLANS[cid]), key=lambda p: _order(p[1]))


@pytest.mark.parametrize("cid,tag", _PARAMS, ids=["%s-%s" % p for p in _PARAMS])
def test_layout(cid, tag):
    _check(cid, tag)


# ---- lasso_mstep_pipe_* -----------------------------------------------------------------------------------------------
def _pipelined_mstep(eng, n, d, k, Z, X, AB, D, seq):
    """one pipelined M-step as test_pipelined_mstep_against_the_plain_one runs it (the later stages on the side stream)"""
    stages = eng.mstep_pipe_stages(d, k)
    ws = eng.mstep_pipe_workspace(n, d, k)
    S = eng.side_stream()
    eng.pipe_gram(Z, X, AB, 0, ws)
    eng.pipe_rows(AB, D, n, 0, ws, seq=seq)
    with torch.cuda.stream(S):
        eng.pipe_wait(n, d, k, seq, ws)
        for s_ in range(1, len(stages)):
            eng.pipe_gram(Z, X, AB, s_, ws)
            eng.pipe_rows(AB, D, n, s_, ws)
        eng.pipe_signal(n, d, k, seq, ws)
    mask = eng.pipe_sweep(AB, D, n, 1e-10, False, ws)
    _, ndeg = eng.pipe_finish(D, n, 1e-10, False, mask, ws, wait_seq=seq)()
    torch.cuda.synchronize()
    return mask.cpu(), ndeg


def test_pipelined_mstep_on_pitched_operands():
    """[A | B], Z, X and the dictionary pitched (16-byte aligned, pitches multiples of 4: what the header asks of the
    lasso_mstep_pipe_* calls) against the plain form: [A | B], dictionary, flags and count bit for bit, padding untouched;
    [A | B] against the fp64 products at 2e-6.  `odd` and `offset` operands answer LASSO_ERR_BAD_ARG with the rule, and
    nothing is written."""
    from lasso_amd.engine import HipEngine
    nat, L = _nat()
    n, d, k = 300, 256, 512
    eng = HipEngine()
    g = torch.Generator().manual_seed(n + k)
    X = torch.randn(n, d, generator=g)
    Z = _sparse(n, k, 7)
    D0 = torch.nn.functional.normalize(torch.randn(d, k, generator=g), dim=0)
    assert len(eng.mstep_pipe_stages(d, k)) >= 2
    results = {}
    for lay in ("natural", "pitched"):
        P = dict(z=layouts.place(Z, lay, NAN, "cuda", "z"), x=layouts.place(X, lay, NAN, "cuda", "x"),
                 d=layouts.place(D0, lay, NAN, "cuda", "d"),
                 ab=layouts.place(torch.zeros(k, k + d), lay, layouts.SENTINEL, "cuda", "ab", fill=layouts.SENTINEL))
        mask, ndeg = _pipelined_mstep(eng, n, d, k, P["z"].view, P["x"].view, P["ab"].view, P["d"].view, 1)
        P["z"].check()
        P["x"].check()
        P["d"].check(written=True)
        P["ab"].check(written=True)
        results[lay] = (P["ab"].view.cpu(), P["d"].view.cpu(), mask, ndeg)
    AB, D, mask, ndeg = results["natural"]
    A64, B64 = Z.double().T @ Z.double(), Z.double().T @ X.double()
    ea = (AB[:, :k].double() - A64).abs().max().item() / A64.abs().max().item()
    eb = (AB[:, k:].double() - B64).abs().max().item() / B64.abs().max().item()
    record_margins("layouts_mstep_pipe", dict(A_rel=ea, B_rel=eb))
    assert ea <= 2e-6 and eb <= 2e-6 and ndeg == 0 and not bool(torch.isnan(D).any())
    for a, b in zip(results["natural"], results["pitched"]):
        assert _same(a, b)
    # refusals: the rule in the text, nothing enqueued
    ws = eng.mstep_pipe_workspace(n, d, k)
    flags = torch.zeros(k, dtype=torch.int32, device="cuda")
    for lay in ("odd", "offset"):
        for which in ("ab", "z", "x", "d"):
            P = {nm: layouts.place(t, lay if nm == which else "natural", NAN if nm != "ab" else layouts.SENTINEL, "cuda", nm,
                                   fill=layouts.SENTINEL if nm == "ab" else None)
                 for nm, t in (("z", Z), ("x", X), ("d", D0), ("ab", torch.zeros(k, k + d)))}
            z, x, dd, ab = (P[nm] for nm in ("z", "x", "d", "ab"))
            st, tail = nat.stream_ptr(ws.device), (nat.ptr(ws), ws.numel())
            got = []
            if which != "d":
                got.append(L.lasso_mstep_pipe_gram(nat.ptr(z.view), z.ld, nat.ptr(x.view), x.ld, n, d, k, nat.LASSO_F32,
                                                   nat.ptr(ab.view), ab.ld, 0, *tail, st))
            if which in ("ab", "d"):
                got.append(L.lasso_mstep_pipe_rows(nat.ptr(ab.view), ab.ld, nat.ptr(dd.view), dd.ld, n, d, k, nat.LASSO_F32, 0, 1,
                                                   *tail, st))
            if which == "d":
                got.append(L.lasso_mstep_pipe_sweep(nat.ptr(ab.view), ab.ld, nat.ptr(dd.view), dd.ld, n, d, k, nat.LASSO_F32,
                                                    1e-10, 0, nat.ptr(flags), *tail, st))
            assert got == [nat.LASSO_ERR_BAD_ARG] * len(got), (lay, which, got)
            assert "16-byte aligned" in L.lasso_hip_last_error().decode()
            torch.cuda.synchronize()
            for pl in P.values():
                pl.check()
