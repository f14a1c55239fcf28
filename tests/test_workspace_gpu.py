"""Every Python entry point on poisoned scratch and on a late side stream (include/lasso_hip.h, "Scratch and stream
contract").

The registry below holds the smallest case per dispatched form, each with an anchor: the call on zero-filled scratch of
exactly the size the library asked for (tests/ws_poison.py, mode ``zero``).  Per case:

  1. the anchor against the oracle / the fp64 reference / the recorded run at the bar which that entry point's own test
     uses (each bar is quoted with the file it comes from);
  2. ``ones`` (0xFF: NaN, -1), ``fives`` (0x55: a large finite float, a plausible count) and ``roomy`` (1 MiB + 4 bytes
     more than asked for) return the anchor's tensors with torch.equal and report the same iterations, sums, traces,
     statuses and info dicts: nothing the call computes may depend on what the scratch held or on how large it was;
  3. the 4096-byte guard bands in front of and behind every workspace the call asked for are intact in all four modes:
     ``*_workspace_bytes`` is sufficient and nothing outside the workspace is written;
  4. ``stream``: the call on a fresh torch.cuda.Stream() S whose operands are still NaN when the host reaches the library
     -- S first holds itself back for ~45 ms (one spinning thread, then two 8192^3 products), then runs the copies that
     fill the operands, then the call; scratch is ``ones`` and filled on S too; the default stream stays idle and is
     never synchronised.  A launch, memset or copy the library
     enqueued on the null stream or on a stream of its own is not ordered behind S's work on torch's non-blocking
     streams: it reads NaN operands or unfilled scratch, and the result differs from the anchor.  (Once an entry point
     has waited for S on the host, e.g. for a stop decision, its later launches are no longer early: the check covers
     every launch up to the call's first host wait.  S is taken from torch's pool until one is found that does not
     share the default stream's hardware queue -- behind one that does, the runtime serves the two in order and a stray
     launch on the default stream would wait for S after all: _runs_beside_the_default_stream.)

_NOT_REPRODUCIBLE lists the cases excused from (2) and from the bitwise part of (4); the project documents its paths as
bitwise reproducible, so the table is empty.  A case may be listed only if two ``zero`` runs of it already differ -- the
test checks that before it excuses the case -- and keeps (1) and (3) in every mode.

One line per case with the dispatched kernel or form goes to tests/margins.py ("workspace/<case>") and is printed."""
import contextlib
import io
import math
import time
import warnings

import numpy as np
import pytest
import torch

from margins import record_margins
from ws_poison import MODES, GuardBroken, Poison

pytestmark = pytest.mark.gpu
NAN = float("nan")
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
S29 = 2.0 ** -29                    # float64 bars: the fp32 bar scaled by the ratio of the unit roundoffs
Z_BAR = 5e-5                        # max|dz| against the oracle (tests/test_random_shapes_gpu.py, test_fista_gpu.py)
Z_BAR_F64 = 5e-5 * S29              # tests/test_f64_gpu.py
LOSS_RTOL, LOSS_RTOL_F64 = 2e-6, 2e-6 * S29      # tests/test_dict_learning_gpu.py::test_lasso_loss, test_f64_gpu.py
G_RTOL = 2e-4                       # gradients: tests/test_autograd_gpu.py, tests/test_conv_autograd_gpu.py
BF16_OBJ_RTOL = 2e-3                # SURVEY 8d, tests/test_layouts_gpu.py::_bf16

# case id -> why two runs of the same call on the same scratch differ (checked by the test before it excuses the case)
_NOT_REPRODUCIBLE = {}


def _nat():
    from lasso_amd import _native as nat
    return nat, nat.lib()


def _orc():
    from oracle import lasso_oracle as orc
    return orc


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _problem(n, d, k, seed, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    W = torch.nn.functional.normalize(torch.randn(d, k, generator=g, dtype=dtype), dim=0)
    X = torch.randn(n, d, generator=g, dtype=dtype)
    return X, W


def _start(n, k, seed, dtype=F32):
    return (0.05 * torch.randn(n, k, generator=torch.Generator().manual_seed(seed))).to(dtype)


def _lr(W):
    return 1.0 / max(_orc().lipschitz_constant(W.double(), "exact"), 1e-3)


@contextlib.contextmanager
def _quiet():
    """-> [warnings' texts, printed text]: what a call says is part of what it reports"""
    out, said = io.StringIO(), []
    with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(out):
        warnings.simplefilter("always")
        yield said
    said.append(sorted(str(c.message) for c in caught))
    said.append(out.getvalue())


class Case:
    """operands: {name: CPU tensor}; call(ops) with ops the same tensors on the device -> ({name: device tensor},
    {key: host value}) -- the entry point alone, nothing that waits or computes on the CPU in front of it;
    verify(tensors on the CPU, host values) asserts the reference bar and returns the measured margins;
    kernel: the dispatched kernel / form, as the library names it where it has a name for it."""

    def __init__(self, operands, call, verify, kernel):
        self.operands, self.call, self.verify, self.kernel = operands, call, verify, kernel


_FACTORY, _BUILT, _ANCHOR = {}, {}, {}


def _register(cid, factory):
    assert cid not in _FACTORY, cid
    _FACTORY[cid] = factory


def _case(cid):
    if cid not in _BUILT:
        _BUILT[cid] = _FACTORY[cid]()
    return _BUILT[cid]


def _host(v):
    """host values in a comparable form: tensors on the CPU, containers walked"""
    if isinstance(v, torch.Tensor):
        return v.detach().cpu()
    if isinstance(v, dict):
        return {k: _host(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_host(x) for x in v]
    if isinstance(v, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(v))
    return v


def _bits(t):
    """equal as bits: a NaN a call reports (last_delta of a fixed-count solve) equals itself"""
    if t.is_floating_point():
        return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and a != a:
        return isinstance(b, float) and b != b
    return type(a) is type(b) and a == b


def _differences(got, want):
    """names of the tensors / host values of (tensors, host) that are not bit for bit the anchor's"""
    bad = ["tensor %s (max |difference| %g)" % (k, (got[0][k].double() - want[0][k].double()).abs().max().item()
                                                if got[0][k].shape == want[0][k].shape else NAN)
           for k in want[0] if not _same(got[0].get(k), want[0][k])]
    bad += ["%s: %r != %r" % (k, got[1].get(k), want[1][k]) for k in want[1] if not _same(got[1].get(k), want[1][k])]
    if got[0].keys() != want[0].keys() or got[1].keys() != want[1].keys():
        bad.append("another set of results")
    return bad


def _run(case, mode):
    """the case on scratch of `mode`, operands in place before the call -> (tensors on the CPU, host values)"""
    ops = {name: t.cuda() for name, t in case.operands.items()}
    torch.cuda.synchronize()
    with Poison(mode).installed() as poison:
        tensors, host = case.call(ops)
        out = {k: v.detach().cpu() for k, v in tensors.items()}, _host(host)
        torch.cuda.synchronize()
    assert poison.requests, "the call asked for no workspace: the patch did not reach it"
    return out


_BUSY = {}
SPIN_MS = 25.0


def _busy_init():
    """the operands of the matmuls, and how many cycles of torch.cuda._sleep make a millisecond (measured once with
    events; clamped so that a misreading cannot turn SPIN_MS into more than 1.25 s)"""
    if not _BUSY:
        _BUSY["mm"] = [torch.randn(8192, 8192, device="cuda") for _ in range(2)] + [torch.empty(8192, 8192, device="cuda")]
        _BUSY["probe"] = torch.zeros(64, device="cuda")
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(100000)
        t0.record()
        torch.cuda._sleep(2000000)
        t1.record()
        torch.cuda.synchronize()
        _BUSY["cycles_per_ms"] = min(max(2000000 / max(t0.elapsed_time(t1), 1e-3), 5e4), 5e6)
    return _BUSY


def _busy():
    """Holds the current stream back for SPIN_MS + ~20 ms.  First ONE thread spinning (torch.cuda._sleep): the stream is
    blocked while every CU is free, so a launch on ANOTHER hardware queue meanwhile is dispatched at once, whereas
    behind two 8192^3 products alone (the busy-GPU tests' ~10 ms each, tests/test_properties_gpu.py), which fill every
    CU, when it is dispatched is up to the hardware's arbitration.  The products follow all the same."""
    busy = _busy_init()
    torch.cuda._sleep(int(SPIN_MS * busy["cycles_per_ms"]))
    a, b, c = busy["mm"]
    for _ in range(2):
        torch.mm(a, b, out=c)


def _runs_beside_the_default_stream(side):
    """Whether work handed to the default stream is served while `side` is held back.  The HIP runtime multiplexes its
    streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default) and serves the streams that share a queue in
    order: behind a side stream that shares the DEFAULT stream's queue a stray launch on the default stream waits for
    the side stream's work after all, and the harness would see nothing (without this probe the fake solver below went
    unflagged in two of four runs of this file, each time on the same stream of torch's pool; with it, never in three
    runs of six streams in a row).  Probed with 3 ms of one spinning thread on `side` and one tiny launch on the
    default stream: served within 1.5 ms or not."""
    busy = _busy_init()
    done = torch.cuda.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(3.0 * busy["cycles_per_ms"]))
    busy["probe"].add_(1)
    done.record()
    served, t0 = False, time.perf_counter()
    while not served and time.perf_counter() - t0 < 1.5e-3:
        served = done.query()
    torch.cuda.synchronize()
    return served


def _side_stream():
    """a fresh torch.cuda.Stream() that does not share the default stream's hardware queue"""
    for _ in range(16):
        side = torch.cuda.Stream()
        if _runs_beside_the_default_stream(side):
            return side
    raise AssertionError("no stream of torch's pool runs beside the default stream: the stream axis cannot see anything")


def _run_late(call, operands, mode="ones"):
    """call(ops) on a fresh side stream whose operands are filled only after ~45 ms of other work on that stream"""
    side = _side_stream()
    staging = {name: t.cuda() for name, t in operands.items()}
    ops = {name: torch.full_like(t, NAN) if t.is_floating_point() else torch.full_like(t, -1) for name, t in staging.items()}
    torch.cuda.synchronize()            # (the last synchronise of the device: the default stream is idle from here on)
    with torch.cuda.stream(side), Poison(mode).installed(sync=side.synchronize):     # (guards read on the side stream too)
        _busy()
        for name in ops:
            ops[name].copy_(staging[name], non_blocking=True)
        tensors, host = call(ops)
        out = {k: v.detach().cpu() for k, v in tensors.items()}, _host(host)       # (read back on the side stream)
        side.synchronize()
    return out


def _anchor(cid):
    if cid not in _ANCHOR:
        _ANCHOR[cid] = _run(_case(cid), "zero")
    return _ANCHOR[cid]


def _excused(cid):
    """a listed case: two runs on zeroed scratch must already differ, else the excuse does not hold"""
    if cid not in _NOT_REPRODUCIBLE:
        return False
    again = _run(_case(cid), "zero")
    assert _differences(again, _anchor(cid)), "%s is listed as not reproducible (%s) but two runs on zeroed scratch " \
        "are bitwise equal: take it off the list" % (cid, _NOT_REPRODUCIBLE[cid])
    return True


def _check(cid, mode):
    case = _case(cid)
    if mode == "zero":
        got = _anchor(cid)
        margins = case.verify(*got)
        line = dict(kernel=case.kernel, **margins)
        record_margins("workspace/" + cid, line)
        print("workspace/%s: %s" % (cid, line))
        return
    want = _anchor(cid)
    got = _run_late(case.call, case.operands) if mode == "stream" else _run(case, mode)
    if _excused(cid):
        case.verify(*got)
        return
    bad = _differences(got, want)
    assert not bad, "%s on %s differs from the anchor: %s" % (cid, "a late side stream" if mode == "stream" else
                                                              "scratch of mode '%s'" % mode, "; ".join(bad))


# ======================================================================================================================
# ista: lasso_fista_solve / _f64 through lasso_amd.linear.solvers.ista and sparse_encode
# ======================================================================================================================
def _ista(n, d, k, seed, *, fast=True, kernel="auto", start="warm", maxiter=11, tol=0.0, lr="exact", backtrack=False,
          dtype=F32, stop_mode="global", alpha=0.2, name_has=None, tile_of=None, stop_at=None):
    """start: 'warm' (a z0 tensor), 'zeros' (a zeros tensor) or 'lazy' (sparse_encode's own start: a NULL z0, the
    zero-start kernels).  lr: 'exact' (1 / lambda_max in double, as the oracle forms it), 'auto' or a number.
    stop_at: the iteration the ORACLE must stop at (tests/test_layouts_gpu.py::_stop_rule: the tolerance goes into the
    geometric middle of the gap between that iteration's sum and the smallest one before it)."""
    def factory():
        from lasso_amd.linear import sparse_encode
        from lasso_amd.linear.solvers import ista
        nat, L = _nat()
        orc = _orc()
        X, W = _problem(n, d, k, seed)
        z0 = torch.zeros(n, k) if start in ("zeros", "lazy") else _start(n, k, seed + 100)
        X, W, z0 = X.to(dtype), W.to(dtype), z0.to(dtype)
        ref_t = F64 if dtype == F64 else F32
        Xr, Wr, z0r = X.to(ref_t), W.to(ref_t), z0.to(ref_t)
        step = _lr(Wr) if lr in ("exact", "auto") else float(lr)
        t = tol
        if stop_at is not None:
            tr = orc.FistaTrace()
            orc.fista(Xr, z0r, Wr, alpha, fast=fast, lr=step, maxiter=stop_at, tol=0.0, trace=tr)
            here, before = tr.delta[stop_at - 1], min(tr.delta[:stop_at - 1])
            assert here < before * (1 - 1e-3), (here, before)
            t = (here * before) ** 0.5 / (n * k)
        # float64 with lr='auto': the oracle at the step of the library's own lambda_max, which the call reports beside the
        # codes and which is held to 2e-6 of the exact value (tests/test_f64_gpu.py::test_lipschitz_constant_of_a_float64_...)
        own_step = lr == "auto" and dtype == F64
        tr = orc.FistaTrace()
        ref = orc.fista(Xr, z0r, Wr, alpha, fast=fast, lr=step, maxiter=maxiter, tol=t, backtrack=backtrack, trace=tr)
        if t > 0:
            assert tr.stopped and 1 < tr.iterations < maxiter and (stop_at is None or tr.iterations == stop_at), tr.iterations
        code = {F32: nat.LASSO_F32, F64: nat.LASSO_F64, BF16: nat.LASSO_BF16}[dtype]
        name = L.lasso_fista_kernel_name(n, d, k, code, int(backtrack)).decode()
        if name_has:
            assert name_has in name, name
        if tile_of:       # (lasso_fista_kernel_name takes no hint: the tile instantiation depends on (d, k) alone)
            big = L.lasso_fista_kernel_name(1 << 16, d, k, code, 0).decode()
            assert big.startswith("lasso::sp::fista_tile_sp_kernel<%d, %d," % tile_of), big
            name = big
        if kernel != "auto":
            name = "kernel=%r (unhinted: %s)" % (kernel, name)

        def call(ops):
            kw = dict(fast=fast, lr="auto" if lr == "auto" else step, maxiter=maxiter, tol=t, backtrack=backtrack,
                      return_info=True, stop_mode=stop_mode, kernel=kernel)
            with _quiet() as said:
                if start == "lazy":
                    z, info = sparse_encode(ops["x"], ops["w"], alpha, **kw)
                else:
                    z, info = ista(ops["x"], ops["z0"], ops["w"], alpha, **kw)
            host = dict(info=info, said=said)
            if own_step:
                from lasso_amd.linear.lipschitz import lipschitz_constant
                host["lambda_max"] = lipschitz_constant(ops["w"])
            return dict(z=z), host

        def verify(out, host):
            info = host["info"]
            assert info["iterations"] == tr.iterations, (info["iterations"], tr.iterations)
            if backtrack:
                assert info["trials"] == list(tr.trials), (info["trials"], tr.trials)
            if dtype == BF16:
                def objective(z):
                    z = z.double()
                    return ((0.5 * (z @ Wr.double().T - Xr.double()).pow(2).sum() + alpha * z.abs().sum()) / n).item()
                rel = abs(objective(out["z"].float()) - objective(ref)) / objective(ref)
                assert rel <= BF16_OBJ_RTOL, rel
                return dict(objective_rel=rel, iterations=info["iterations"])
            want = ref
            if own_step:
                assert abs(host["lambda_max"] * step - 1.0) <= 2e-6, (host["lambda_max"], 1.0 / step)
                want = orc.fista(Xr, z0r, Wr, alpha, fast=fast, lr=1.0 / host["lambda_max"], maxiter=maxiter, tol=t)
            err = (out["z"] - want).abs().max().item()
            assert err <= (Z_BAR_F64 if dtype == F64 else Z_BAR), err
            return dict(max_dz=err, iterations=info["iterations"])
        ops = dict(x=X, w=W)
        if start != "lazy":
            ops["z0"] = z0
        return Case(ops, call, verify, name)
    return factory


_register("ista-tile16x256", _ista(40, 256, 1024, 1, kernel="tile", tile_of=(1024, 16)))
_register("ista-tile32x128", _ista(40, 100, 512, 2, kernel="tile", tile_of=(512, 32)))
_register("ista-tile64x64", _ista(70, 64, 256, 3, kernel="tile", tile_of=(256, 64)))
_register("ista-plain-tile16x256", _ista(40, 256, 1024, 1, kernel="tile", fast=False, tile_of=(1024, 16)))
# solve_geometry() pads 300 atoms to 384 and 700 to 768 (tests/test_fista_gpu.py::test_exactly_sized_workspace_fits_...)
_register("ista-384-atoms", _ista(4096, 64, 300, 4, name_has="384"))
_register("ista-768-atoms", _ista(2500, 200, 700, 5, name_has="768"))
_register("ista-splitk", _ista(40, 256, 1024, 1, kernel="splitk"))
_register("ista-splitk-auto", _ista(40, 256, 1024, 1, name_has="splitk"))
_register("ista-narrow", _ista(40, 100, 1024, 6, kernel="narrow"))
_register("ista-unfused-hint", _ista(40, 256, 1024, 1, kernel="unfused"))
_register("ista-unfused-ragged", _ista(70, 300, 1100, 7, name_has="unfused"))
_register("ista-hybrid-4900", _ista(4900, 256, 1024, 77, start="zeros", name_has="split"))
_register("ista-zero-start", _ista(40, 256, 1024, 8, start="lazy"))
_register("ista-zero-start-tile", _ista(4100, 64, 256, 9, start="lazy", name_has="fista_tile_sp"))
_register("ista-warm-fused", _ista(40, 256, 1024, 11))
_register("ista-stop-in-kernel", _ista(96, 256, 1024, 21, alpha=0.4, maxiter=200, tol=1e-4))
_register("ista-stop-in-kernel-tile", _ista(4100, 64, 256, 23, alpha=0.4, maxiter=200, tol=1e-4, name_has="fista_tile_sp"))
_register("ista-stop-chunked-replay", _ista(96, 256, 1024, 21, alpha=0.4, maxiter=200, stop_at=30, stop_mode="chunked"))
_register("ista-stop-unfused", _ista(70, 300, 1100, 22, alpha=0.4, maxiter=200, tol=1e-4))
# lr='auto': lambda_max on the stream inside the solve (d <= 256, k <= 1024: the persistent squaring kernel at d = 256, the
# one-workgroup chain at d <= 64), or lipschitz_constant() + the unfused solve beyond.  The bar: tests/test_layouts_gpu.py
# ::_lr_auto (the oracle takes the exact 1 / lambda_max: 5e-5)
_register("ista-lr-auto-256x1024", _ista(40, 256, 1024, 31, start="zeros", lr="auto"))
_register("ista-lr-auto-48x160", _ista(40, 48, 160, 32, start="zeros", lr="auto"))
_register("ista-lr-auto-300x513", _ista(40, 300, 513, 33, start="zeros", lr="auto"))
_register("ista-backtrack-windows", _ista(300, 48, 160, 41, alpha=0.3, lr=1.0, maxiter=8, backtrack=True, name_has="bt_iter_kernel"))
_register("ista-backtrack-multi-launch", _ista(300, 48, 160, 41, alpha=0.3, lr=1.0, maxiter=8, backtrack=True, kernel="splitk"))
_register("ista-backtrack-k-odd", _ista(60, 48, 162, 43, alpha=0.3, lr=1.0, maxiter=6, backtrack=True, name_has="bt_grad_kernel"))
_register("ista-backtrack-generic", _ista(70, 300, 1100, 42, alpha=0.3, lr=1.0, maxiter=5, backtrack=True))
_register("ista-bf16-persistent", _ista(200, 256, 1024, 131, alpha=0.3, dtype=BF16, name_has="bt16_persist_kernel"))
_register("ista-bf16-persistent-backtrack", _ista(200, 256, 1024, 131, alpha=0.3, lr=1.0, maxiter=8, backtrack=True, dtype=BF16,
                                                  name_has="bt16_persist_kernel"))
_register("ista-bf16-multi-launch", _ista(100, 100, 512, 132, alpha=0.3, dtype=BF16, kernel="tile"))
_register("ista-bf16-multi-launch-backtrack", _ista(100, 100, 512, 132, alpha=0.3, lr=1.0, maxiter=8, backtrack=True, dtype=BF16,
                                                    kernel="tile"))
_register("ista-f64-fixed", _ista(33, 200, 513, 51, alpha=0.3, dtype=F64))
_register("ista-f64-stop", _ista(33, 200, 513, 51, alpha=0.3, dtype=F64, maxiter=200, tol=1e-4))
_register("ista-f64-lr-auto", _ista(33, 200, 513, 51, alpha=0.3, dtype=F64, lr="auto"))
_register("ista-f64-backtrack", _ista(33, 200, 513, 51, alpha=0.3, dtype=F64, lr=1.0, maxiter=6, backtrack=True))


# ======================================================================================================================
# lasso_loss, init='transpose', lipschitz_constant
# ======================================================================================================================
def _loss(n, d, k, seed, dtype):
    def factory():
        from lasso_amd.linear import lasso_loss
        X, W = _problem(n, d, k, seed, dtype)
        g = torch.Generator().manual_seed(seed + 1)
        Z = torch.randn(n, k, generator=g, dtype=dtype) * (torch.rand(n, k, generator=g) < 0.2)
        X64, W64, Z64 = X.double(), W.double(), Z.double()
        ref = ((0.5 * (Z64 @ W64.T - X64).pow(2).sum() + 0.7 * Z64.abs().sum()) / n).item()

        def call(ops):
            return dict(loss=lasso_loss(ops["x"], ops["z"], ops["w"], 0.7)), {}

        def verify(out, host):
            err = abs(out["loss"].item() - ref) / abs(ref)
            assert err <= (LOSS_RTOL_F64 if dtype == F64 else LOSS_RTOL), err
            return dict(loss_rel=err)
        form = "tile (d <= 256, k <= 1024)" if d <= 256 and k <= 1024 and d > 64 else "generic"
        return Case(dict(x=X, w=W, z=Z), call, verify, "lasso_objective%s: %s" % ("_f64" if dtype == F64 else "_throttled", form))
    return factory


for _dt, _t in ((F32, "f32"), (F64, "f64")):
    _register("loss-%s-tile" % _t, _loss(50, 256, 1024, 81, _dt))
    _register("loss-%s-generic-small" % _t, _loss(50, 48, 160, 82, _dt))
    _register("loss-%s-generic-large" % _t, _loss(50, 300, 1100, 83, _dt))


def _init_transpose(n, d, k, dtype):
    """the bound of tests/test_layouts_gpu.py::_init_transpose and test_f64_gpu.py: |error| <= d eps (|X| |W|)"""
    def factory():
        from lasso_amd.linear import initialize_code
        X, W = _problem(n, d, k, n + d, dtype)
        ref = X.double() @ W.double()
        bound = d * (2.0 ** -53 if dtype == F64 else 2.0 ** -24) * (X.double().abs() @ W.double().abs())

        def call(ops):
            with torch.no_grad():
                return dict(z0=initialize_code(ops["x"], ops["w"], 1.0, "transpose")), {}

        def verify(out, host):
            err = (out["z0"].double() - ref).abs()
            ratio = (err / bound.clamp_min(1e-300)).max().item()
            assert bool((err <= bound).all()), ratio
            return dict(worst_error_over_bound=ratio)
        return Case(dict(x=X, w=W), call, verify, "lasso_init_transpose")
    return factory


_register("init-transpose-f32", _init_transpose(33, 200, 513, F32))
_register("init-transpose-f64", _init_transpose(33, 200, 513, F64))


def _lipschitz(d, k, dtype):
    """2e-6 of the exact value (tests/test_dict_learning_gpu.py, test_f64_gpu.py)"""
    def factory():
        from lasso_amd.linear.lipschitz import lipschitz_constant
        W = torch.randn(d, k, generator=torch.Generator().manual_seed(d + k), dtype=dtype)
        ref = _orc().lipschitz_constant(W.double(), "exact")

        def call(ops):
            return {}, dict(lambda_max=lipschitz_constant(ops["w"]))

        def verify(out, host):
            err = abs(host["lambda_max"] - ref) / ref
            assert err <= 2e-6, (host, ref)
            return dict(rel=err)
        m = min(d, k)
        form = "square_chain (m <= 64)" if m <= 64 else "square_persist (64 < m <= 256)" if m <= 256 else "syrk per squaring"
        return Case(dict(w=W), call, verify, "lasso_lipschitz: " + form)
    return factory


for _d, _k in ((48, 160), (200, 513), (300, 513)):
    _register("lipschitz-f32-%dx%d" % (_d, _k), _lipschitz(_d, _k, F32))
_register("lipschitz-f64-200x513", _lipschitz(200, 513, F64))


# ======================================================================================================================
# M-step: update_dict (Gram product + atom sweep), update_dict_ridge
# ======================================================================================================================
def _update_dict(n, d, k, dtype, forms, positive=False):
    """fp32: 1e-4 on the used atoms, 1e-6 on the re-drawn ones (tests/test_dict_learning_gpu.py::
    test_update_dict_wide_rows); float64: ATOM_BAR / DRAW_BAR of tests/test_f64_mstep_gpu.py.  Z: 8 FISTA iterations of
    the oracle with two atoms zeroed (degenerate in the sweep), as in that file."""
    def factory():
        from lasso_amd.linear import update_dict
        orc = _orc()
        X, W = _problem(n, d, k, d + k, dtype)
        Z = orc.fista(X, X.new_zeros(n, k), W, 0.3, lr=_lr(W), maxiter=8, tol=0.0).clone()
        Z[:, [0, 7 % k]] = 0.0
        Dref, Zref = W.clone(), Z.clone()
        torch.manual_seed(3)
        orc.update_dict(Dref, X, Zref, positive=positive)
        redrawn = (Zref == 0).all(0)

        def call(ops):
            D, Zg = ops["d"].clone(), ops["z"].clone()
            torch.manual_seed(3)                   # (the directions of the re-drawn atoms: torch's CPU generator)
            out = update_dict(D, ops["x"], Zg, positive=positive)
            assert out is D
            return dict(d=D, z=Zg), {}

        def verify(out, host):
            err = (out["d"] - Dref).abs().max(0).values
            used = err[~redrawn].max().item()
            drawn = err[redrawn].max().item() if redrawn.any() else 0.0
            bars = (1e-4 * S29, 5e-5 * S29) if dtype == F64 else (1e-4, 1e-6)
            assert used <= bars[0] and drawn <= bars[1], (used, drawn)
            assert torch.equal(out["z"] == 0, Zref == 0)
            return dict(used_atoms=used, redrawn_atoms=drawn)
        return Case(dict(d=W, x=X, z=Z), call, verify, forms)
    return factory


_register("update-dict-gram-ab256-sweep-persistent", _update_dict(4096, 256, 256, F32, "gram_ab256_kernel + sweep_persist_kernel"))
_register("update-dict-gram-tn128-sweep-small", _update_dict(600, 64, 256, F32, "gram_tn128_kernel (A and B in one) + sweep_small_kernel"))
_register("update-dict-gram-fallback-sweep-persistent", _update_dict(300, 200, 300, F32, "gram_tn128_kernel / gram_tn_kernel + sweep_persist_kernel"))
_register("update-dict-sweep-blocked", _update_dict(400, 300, 96, F32, "gram_tn_kernel + sweep_block_kernel / trailing_update_kernel"))
_register("update-dict-positive", _update_dict(300, 200, 300, F32, "sweep_persist_kernel, positive", positive=True))
_register("update-dict-f64", _update_dict(100, 48, 200, F64, "lasso_gram_accumulate_f64 + lasso_dict_sweep_f64"))
_register("update-dict-f64-wide", _update_dict(60, 520, 40, F64, "lasso_dict_sweep_f64, d > 512"))


def _update_dict_ridge(n, d, k, dtype):
    """fp32: 2e-4 max(1, max|V|) (tests/test_dict_learning_gpu.py::test_update_dict_against_reference_outputs); float64:
    RIDGE_BAR of tests/test_f64_mstep_gpu.py; lambd = 1e-2 as there"""
    def factory():
        from lasso_amd.linear import update_dict_ridge
        orc = _orc()
        X, W = _problem(n, d, k, d + k, dtype)
        Z = orc.fista(X, X.new_zeros(n, k), W, 0.3, lr=_lr(W), maxiter=8, tol=0.0).clone()
        ref = orc.update_dict_ridge(X.double(), Z.double(), lambd=1e-2)

        def call(ops):
            return dict(v=update_dict_ridge(ops["x"], ops["z"], lambd=1e-2)), {}

        def verify(out, host):
            err = (out["v"].double() - ref).abs().max().item()
            bar = 2e-4 * (S29 if dtype == F64 else 1.0) * max(1.0, ref.abs().max().item())
            assert err <= bar, (err, bar)
            return dict(max_dv=err, bar=bar)
        return Case(dict(x=X, z=Z), call, verify, "lasso_gram_accumulate + lasso_ridge_solve" + ("_f64" if dtype == F64 else ""))
    return factory


_register("update-dict-ridge-f32", _update_dict_ridge(257, 70, 33, F32))
_register("update-dict-ridge-f32-k513", _update_dict_ridge(600, 48, 513, F32))
_register("update-dict-ridge-f64", _update_dict_ridge(150, 20, 130, F64))


# ======================================================================================================================
# autograd: the traced forward (lasso_fista_prepare + lasso_fista_run on a held workspace) and lasso_fista_backward_steps
# ======================================================================================================================
def _ista_backward(n, d, k, fast, T=6):
    """tests/test_autograd_gpu.py: codes 5e-5, gradients 2e-4 of max(|gradient|, 1e-3)"""
    def factory():
        from lasso_amd.linear.solvers import ista
        orc = _orc()
        g = torch.Generator().manual_seed(0)
        W = torch.nn.functional.normalize(torch.randn(d, k, generator=g), dim=0)
        X = torch.randn(n, d, generator=g)
        Z0 = torch.randn(n, k, generator=g) * 0.05
        G = torch.randn(n, k, generator=g)
        lr = _lr(W)

        def grads(fn, x, w, z0, gz):
            x, w, z0 = (t.detach().clone().requires_grad_(True) for t in (x, w, z0))
            z = fn(x, z0, w)
            (z * gz).sum().backward()
            return dict(z=z.detach(), dx=x.grad, dw=w.grad, dz0=z0.grad)
        ref = grads(lambda x, z0, w: orc.fista(x, z0, w, 0.3, fast=fast, lr=lr, maxiter=T, tol=0.0), X, W, Z0, G)

        def call(ops):
            return grads(lambda x, z0, w: ista(x, z0, w, 0.3, fast=fast, lr=lr, maxiter=T, tol=0.0),
                         ops["x"], ops["w"], ops["z0"], ops["g"]), {}

        def verify(out, host):
            assert (out["z"] - ref["z"]).abs().max().item() <= Z_BAR
            worst = {}
            for name in ("dx", "dw", "dz0"):
                worst[name] = (out[name] - ref[name]).abs().max().item() / (G_RTOL * max(ref[name].abs().max().item(), 1e-3))
            assert all(v <= 1.0 for v in worst.values()), worst
            return dict(worst_fraction_of_bar=worst)
        return Case(dict(x=X, w=W, z0=Z0, g=G), call, verify, "lasso_fista_run x %d + lasso_fista_backward_steps" % T)
    return factory


_register("ista-backward-fused", _ista_backward(64, 256, 1024, True))
_register("ista-backward-small", _ista_backward(37, 10, 50, False))
_register("ista-backward-unfused", _ista_backward(40, 300, 70, True))


# ======================================================================================================================
# the other linear solvers
# ======================================================================================================================
def _coord_descent(n, d, k, seed, maxiter=15):
    """tests/test_cd_gpu.py: max|dz| <= 5e-5 against the oracle while the steps are few"""
    def factory():
        from lasso_amd.linear.solvers import coord_descent
        orc = _orc()
        X, W = _problem(n, d, k, seed)
        z0 = _start(n, k, seed + 100)
        track = z0.clone()
        ref = orc.coordinate_descent(X, W, track, 0.3, maxiter=maxiter)

        def call(ops):
            zt = ops["z0"].clone()
            z, info = coord_descent(ops["x"], ops["w"], zt, 0.3, maxiter=maxiter, return_info=True)
            return dict(z=z, tracked=zt), dict(info=info)

        def verify(out, host):
            err, err_t = (out["z"] - ref).abs().max().item(), (out["tracked"] - track).abs().max().item()
            assert err <= Z_BAR and err_t <= Z_BAR and host["info"]["max_steps"] == maxiter, (err, err_t, host)
            return dict(max_dz=err, max_dz_tracked=err_t)
        return Case(dict(x=X, w=W, z0=z0), call, verify, "lasso_cd_prepare / _run / _finish")
    return factory


_register("coord-descent-30x200x513", _coord_descent(30, 200, 513, 101))
_register("coord-descent-30x48x3000", _coord_descent(30, 48, 3000, 102))


def _golden(name):
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))


def _coord_descent_mod(name):
    """tests/test_cd_mod_gpu.py::test_case_against_fixture: sweeps on the decisive rows, max|dz| <= max(10 spread,
    1e-6 max|z|) there, the reported gap within 5 % of tol_row of the float64 gap of z"""
    def factory():
        import cd_mod_cases as cc
        from lasso_amd.linear.solvers import coord_descent_mod
        spec, g = cc.CASES[name], cc.load_case(_golden("cd_mod_cases"), name)
        x, w = cc.case_inputs(spec)

        def call(ops):
            z, gap, info = coord_descent_mod(ops["x"], ops["w"], alpha=spec["alpha"], max_iter=cc.MAX_ITER, tol=cc.TOL,
                                             return_info=True)
            return dict(z=z, gap=gap), dict(info=info)

        def verify(out, host):
            z, gap, info = out["z"], out["gap"], host["info"]
            c = torch.from_numpy(g["decisive"])
            assert torch.equal(info["sweeps"][c], torch.from_numpy(g["sweeps32"])[c])
            spread = float(g["spread"][g["decisive"]].max())
            dz = float((z - torch.from_numpy(g["z32"]))[c].abs().max())
            bar = max(10.0 * spread, 1e-6 * float(np.abs(g["z32"]).max()))
            assert dz <= bar, (dz, bar)
            tr = cc.tol_row(x).double()
            diff = (gap.double() - cc.gap_f64(z, x, w, spec["alpha"])).abs()
            err = float(torch.where(tr > 0, diff / tr.clamp_min(1e-300), diff).max())
            assert err <= 0.05, err
            return dict(dz=dz, bar=bar, gap_err_over_tol_row=err)
        return Case(dict(x=x, w=w), call, verify, "lasso_cd_mod_solve, k = %d" % spec["k"])
    return factory


for _name in ("sq48_zero_atom", "k257", "k1030"):
    _register("coord-descent-mod-" + _name, _coord_descent_mod(_name))


def _gpsr(name):
    """tests/test_gpsr_gpu.py::test_golden_case: gpsr_cases.check_against_golden at the model's bar"""
    def factory():
        import gpsr_cases as gc
        from lasso_amd.linear import sparse_encode
        spec, gold = gc.CASES[name], gc.load_case(_golden("gpsr_cases"), name)
        x, w, z0 = gc.case_inputs(spec)
        bar, gap, _, _ = gc.z_bar(x, w, spec["alpha"], x0=z0, **spec["kwargs"])

        def call(ops):
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                z, info = sparse_encode(ops["x"], ops["w"], alpha=spec["alpha"], z0=ops.get("z0"), algorithm="gpsr",
                                        return_info=True, **spec["kwargs"])
            return dict(z=z), dict(info=info, warnings=sorted(str(c.message) for c in caught))

        def verify(out, host):
            class Msg:
                def __init__(self, m):
                    self.message = m
            dz = gc.check_against_golden(name, out["z"], host["info"], gold, bar, [Msg(m) for m in host["warnings"]])
            return dict(model_f32_f64_gap=gap, bar=bar, hip_max_dz=dz)
        ops = dict(x=x, w=w)
        if z0 is not None:
            ops["z0"] = z0
        return Case(ops, call, verify, "lasso_gpsr_solve: " + name)
    return factory


for _name in ("default", "debias", "warm", "ragged"):
    _register("gpsr-" + _name, _gpsr(_name))


def _spread_case(module, npz, name, run, form):
    """the solvers with recorded runs and a measured spread (own, iter_ridge, interior_point): codes within
    max(5e-5, 4 spread_z) of the recorded float32 run where the fixture admits the comparison, else the objective within
    max(1e-6, 4 spread_f) of the recorded float64 one -- the rule of tests/test_own_gpu.py, test_iter_ridge_gpu.py and
    test_interior_point_gpu.py"""
    def factory():
        spec, g = module.CASES[name], module.load_case(_golden(npz), name)
        x, w, z0 = module.case_inputs(spec)

        def call(ops):
            with _quiet() as said:
                z, report = run(ops, spec)
            return dict(z=z), dict(report=report, said=said)

        def verify(out, host):
            z = out["z"]
            assert torch.isfinite(z).all()
            if spec["compare"] == "z":
                assert module.admitted_z(g)
                bar = max(5e-5, 4.0 * float(g["spread_z"]))
                dz = float((z - torch.from_numpy(g["z32"])).abs().max())
                assert bar <= 1e-2 and dz <= bar, (dz, bar)
                return dict(dz=dz, bar=bar)
            assert module.admitted_f(g)
            zd = z.double()
            f = float(0.5 * (zd @ w.double().T - x.double()).pow(2).sum() + spec["alpha"] * zd.abs().sum())
            f_ref = float(g["lasso64"]) if "lasso64" in g else float(g["f64"][-1])
            err, bar = abs(f - f_ref) / f_ref, max(1e-6, 4.0 * float(g["spread_f"]))
            assert err <= bar, (err, bar)
            return dict(objective_rel=err, bar=bar)
        return Case(dict(x=x, w=w, z0=z0), call, verify, form)
    return factory


def _own_run(ops, spec):
    from lasso_amd.linear.solvers import orthant_wise_newton
    return orthant_wise_newton(ops["w"], ops["x"], ops["z0"], alpha=spec["alpha"], return_info=True, **spec["kwargs"])


def _iter_ridge_run(ops, spec):
    from lasso_amd.linear.solvers import iterative_ridge
    return iterative_ridge(ops["z0"], ops["x"], ops["w"], alpha=spec["alpha"], return_info=True, **spec["kwargs"])


def _interior_point_run(ops, spec):
    from lasso_amd.linear.solvers import interior_point
    z, ok, info = interior_point(ops["x"], ops["w"], z0=ops["z0"], alpha=spec["alpha"], return_info=True, **spec["kwargs"])
    return z, dict(success=ok, info=info)


def _late(module_name, npz, name, run, form):
    def factory():
        return _spread_case(__import__(module_name), npz, name, run, form)()
    return factory


_register("own-brent", _late("own_cases", "own_cases", "brent_1a", _own_run, "lasso_own_solve: Brent"))
_register("own-brent-6", _late("own_cases", "own_cases", "brent_6a", _own_run, "lasso_own_solve: Brent, 6 iterations"))
_register("own-backtrack", _late("own_cases", "own_cases", "bt_ragged", _own_run, "lasso_own_solve: backtracking"))
_register("own-backtrack-runout", _late("own_cases", "own_cases", "bt_runout", _own_run, "lasso_own_solve: backtracking runs out"))
_register("own-fixed-step", _late("own_cases", "own_cases", "none_half", _own_run, "lasso_own_solve: fixed step"))
_register("iter-ridge-lds-tier", _late("iter_ridge_cases", "iter_ridge_cases", "odd", _iter_ridge_run,
                                       "lasso_iter_ridge_solve: rows_kernel<LDS>"))
_register("iter-ridge-scratch-tier", _late("iter_ridge_cases", "iter_ridge_cases", "k300", _iter_ridge_run,
                                           "lasso_iter_ridge_solve: rows_kernel, triangle in scratch (s = 300)"))
_register("iter-ridge-search", _late("iter_ridge_cases", "iter_ridge_cases", "brent_1b", _iter_ridge_run,
                                     "lasso_iter_ridge_solve: with the Brent search"))
_register("iter-ridge-tolstop", _late("iter_ridge_cases", "iter_ridge_cases", "tolstop2", _iter_ridge_run,
                                      "lasso_iter_ridge_solve: stops before maxiter"))
_register("interior-point-odd", _late("interior_point_cases", "interior_point_cases", "odd", _interior_point_run,
                                      "lasso_interior_point_solve"))
_register("interior-point-d256", _late("interior_point_cases", "interior_point_cases", "d256", _interior_point_run,
                                       "lasso_interior_point_solve: 36 blocks"))
_register("interior-point-stop", _late("interior_point_cases", "interior_point_cases", "stop_odd", _interior_point_run,
                                       "lasso_interior_point_solve: stops before maxiter"))


def _split_bregman(name):
    """tests/test_split_bregman_gpu.py::test_golden_case"""
    def factory():
        import split_bregman_cases as sc
        from lasso_amd.linear.solvers import split_bregman
        spec, g = sc.CASES[name], sc.load_case(_golden("split_bregman_cases"), name)
        A, y, x0 = sc.case_inputs(spec)

        def call(ops):
            x, itn, info = split_bregman(ops["a"], ops["y"], ops.get("x0"), alpha=spec["alpha"], return_info=True, **spec["kwargs"])
            return dict(x=x), dict(itn=itn, info=info)

        def verify(out, host):
            info = host["info"]
            dx = float((out["x"] - torch.from_numpy(g["x32"])).abs().max())
            assert host["itn"] == int(g["itn"]) and info["iterations"] == int(g["iterations"]) and info["stopped"] == bool(g["stopped"])
            got, want = np.asarray(info["update"], dtype=np.float64), np.asarray(g["update32"], dtype=np.float64)
            ru = float(np.max(np.abs(got - want) / np.abs(want)))
            assert dx <= sc.bar_z(g) <= 1e-2 and ru <= sc.rtol_update(g), (dx, sc.bar_z(g), ru)
            return dict(dx=dx, bar=sc.bar_z(g), update_rel=ru)
        ops = dict(a=A, y=y)
        if x0 is not None:
            ops["x0"] = x0
        tol = spec["kwargs"].get("tol", 1e-10)
        return Case(ops, call, verify, "lasso_split_bregman_solve, tol = %g" % tol)
    return factory


_register("split-bregman-tol-positive", _split_bregman("tol_1em2"))
_register("split-bregman-x0", _split_bregman("n33_d20_k70_x0"))
_register("split-bregman-k257", _split_bregman("n40_d32_k257"))


def _split_bregman_no_rule():
    """tol < 0: the stop rule is off, all `maxiter` iterations run.  No recorded run has a negative tol; the reference for
    the codes is the recorded run of the same case with the default tol = 1e-10, which also ran all 20 iterations
    (`stopped` is False there), at its bar"""
    def factory():
        import split_bregman_cases as sc
        from lasso_amd.linear.solvers import split_bregman
        spec, g = sc.CASES["n37_d19_k70"], sc.load_case(_golden("split_bregman_cases"), "n37_d19_k70")
        assert not bool(g["stopped"])
        A, y, _ = sc.case_inputs(spec)

        def call(ops):
            x, itn, info = split_bregman(ops["a"], ops["y"], None, alpha=spec["alpha"], tol=-1.0, return_info=True)
            return dict(x=x), dict(itn=itn, info=info)

        def verify(out, host):
            dx = float((out["x"] - torch.from_numpy(g["x32"])).abs().max())
            assert host["info"]["iterations"] == int(g["iterations"]) and not host["info"]["stopped"]
            assert dx <= sc.bar_z(g), (dx, sc.bar_z(g))
            return dict(dx=dx, bar=sc.bar_z(g))
        return Case(dict(a=A, y=y), call, verify, "lasso_split_bregman_solve, tol < 0")
    return factory


_register("split-bregman-tol-negative", _split_bregman_no_rule())


def _cg(name, dtype=F32):
    """tests/test_conjgrad_gpu.py::check_golden"""
    def factory():
        import conjgrad_cases as cc
        from lasso_amd.conjgrad import batch_cg, cg
        conv = name in cc.CONV
        spec, g = (cc.CONV if conv else cc.DENSE)[name], cc.load_case(_golden("conjgrad_cases"), name)
        A, b = (cc.conv_inputs if conv else cc.dense_inputs)(spec, dtype)

        def call(ops):
            if conv:
                from lasso_amd.conjgrad import batch_cg_conv2d
                x, info = batch_cg_conv2d(ops["a"], ops["b"], tik=spec["tik"], return_info=True, **spec["kwargs"],
                                          **cc.conv_kwargs(spec))
            else:
                x, info = (cg if spec.get("vector") else batch_cg)(ops["a"], ops["b"], return_info=True, **spec["kwargs"])
            return dict(x=x), dict(info=info)

        def verify(out, host):
            info = host["info"]
            if dtype == F64 and not spec.get("f64_only"):
                # a float32 case in double: the same exit, and x as far from the float32 reference as the double reference
                # was (tests/test_conjgrad_gpu.py::test_float64_runs_of_the_float32_cases_stay_within_their_distance)
                dx = float((out["x"] - torch.from_numpy(g["x32"]).double()).abs().max())
                assert info["status"] == int(g["status"]) and info["iterations"] == int(g["iterations"])
                assert dx <= float(g["gap_x"]) + 1e-9, (dx, float(g["gap_x"]))
                return dict(dx_to_x32=dx, gap_x=float(g["gap_x"]), form=info["form"])
            want, floor = ("x64", 1e-12) if dtype == F64 else ("x32", 5e-5)
            dx = float((out["x"].double() - torch.from_numpy(g[want]).double()).abs().max())
            bar, rtol = cc.bar_x(g, floor), cc.rtol_seq(g)
            rs = max(cc.rel(info["r_abs"], g["r_abs"]), cc.rel(info["curv_sum"], g["curv_sum"]), cc.rel(info["rs"], g["rs"]))
            assert info["status"] == int(g["status"]) and info["iterations"] == int(g["iterations"])
            assert dx <= bar <= 1e-2 and rs <= rtol, (dx, bar, rs, rtol)
            return dict(dx=dx, bar=bar, seq_rel=rs, form=info["form"])
        return Case(dict(a=A, b=b), call, verify, "lasso_%scg_solve%s: %s" % ("conv_" if conv else "", " (double)" if dtype == F64 else "", name))
    return factory


_register("cg-vector-f32", _cg("cg_vector"))
_register("batch-cg-f32", _cg("n130_k129_rtol1em4"))
_register("batch-cg-f32-k1030", _cg("n16_k1030_rtol1em4"))
_register("batch-cg-f64", _cg("f64_defaults", F64))
_register("cg-vector-f64", _cg("cg_vector", F64))
_register("batch-cg-conv2d-implicit", _cg("grey_tik0p5"))
_register("batch-cg-conv2d-patches", _cg("stride2_tik0"))


# ======================================================================================================================
# the convolutional path
# ======================================================================================================================
def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _conv(n_spec, C, K, kh, kw, stride, padding, Hz, Wz, *, name_has, dtype=F32, fast=True, maxiter=9, stop=False, grad=False,
          seed=0):
    """ista_conv2d with an explicit step against the oracle: 5e-5 (tests/test_conv_gpu.py; float64: 5e-5 * 2^-29,
    tests/test_conv_f64_gpu.py); gradients 2e-4 of their max magnitude (tests/test_conv_autograd_gpu.py; float64 scaled).
    n_spec: a number of images, or ('cus', a) for #CUs + a, or ('cus/', b) for max(#CUs // b, 8) (the fused kernel's forms
    depend on the number of images per CU).  stop: a tolerance the oracle's sums leave 3 % of room around
    (tests/test_conv_gpu.py::test_stop_rule_count_pinned_exactly_against_the_oracle)."""
    def factory():
        from lasso_amd.conv2d import ista_conv2d
        nat, L = _nat()
        orc = _orc()
        N = n_spec if isinstance(n_spec, int) else _cus() + n_spec[1] if n_spec[0] == "cus" else max(_cus() // n_spec[1], 8)
        (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
        H, W_ = (Hz - 1) * sh - 2 * ph + kh, (Wz - 1) * sw - 2 * pw + kw
        g = torch.Generator().manual_seed(seed + 7 * K + Hz)
        w = (torch.randn(K, C, kh, kw, generator=g) / (C * kh * kw) ** 0.5).to(dtype)
        x = torch.randn(N, C, H, W_, generator=g).to(dtype)
        z0 = (torch.randn(N, K, Hz, Wz, generator=g) * 0.05).to(dtype)
        G = torch.randn(N, K, Hz, Wz, generator=g).to(dtype)
        lr = 0.3 / max(w.pow(2).sum().item(), 1e-3)
        name = L.lasso_conv_ista_kernel_name(N, C, H, W_, K, Hz, Wz, kh, kw, sh, sw, ph, pw).decode()
        if dtype == F32:
            assert name_has in name, name
        else:
            name = "csrc/conv_f64.hip (fp64 MFMA)"
        if grad:
            name = "lasso_conv_ista_run_traced + lasso_conv_ista_backward; the solve alone: " + name
        geo = dict(stride=stride, padding=padding)
        n_ref = min(N, 24)                                   # (the oracle on the first images: they are independent)
        tol, T = 0.0, maxiter
        if stop:
            sums = [orc.conv_fista(x[:N], z0[:N], w, 0.1, maxiter=m, lr=lr, tol=0.0, return_info=True, fast=fast, **geo)[1]["last_delta"]
                    for m in range(1, 25)]
            pick = None
            for m in range(4, 24):
                lo, hi = sums[m - 1], min(sums[:m - 1])
                if lo < hi and hi / lo >= 1.03:
                    pick, budget = m, math.sqrt(lo * hi)
                    break
            assert pick is not None, sums
            tol, T, maxiter_call = budget / z0.numel(), pick, 200
        else:
            maxiter_call = maxiter

        def solve(a, b, c, ist, **kw):
            return ist(a, b, c, 0.1, fast=fast, lr=lr, **geo, **kw)

        def grads(ist, xx, ww, zz, gg, n=None, **kw):
            xx, ww, zz = (t.detach().clone().requires_grad_(True) for t in (xx, ww, zz))
            z = solve(xx, zz, ww, ist, **kw)
            (z * gg).sum().backward()
            return dict(z=z.detach(), dx=xx.grad, dw=ww.grad, dz0=zz.grad)
        if grad:
            ref = grads(orc.conv_fista, x, w, z0, G, maxiter=T, tol=0.0)
        else:
            ref = dict(z=orc.conv_fista(x[:n_ref], z0[:n_ref], w, 0.1, fast=fast, lr=lr, maxiter=T, tol=0.0, **geo))

        def call(ops):
            if grad:
                return grads(ista_conv2d, ops["x"], ops["w"], ops["z0"], ops["g"], maxiter=maxiter_call, tol=tol), {}
            z, info = solve(ops["x"], ops["z0"], ops["w"], ista_conv2d, maxiter=maxiter_call, tol=tol, return_info=True)
            return dict(z=z), dict(info=info)

        def verify(out, host):
            s = S29 if dtype == F64 else 1.0
            err = (out["z"][:ref["z"].shape[0]] - ref["z"]).abs().max().item()
            assert err <= Z_BAR * s, err
            m = dict(max_dz=err)
            if not grad:
                assert host["info"]["iterations"] == T, (host["info"], T)
            else:
                worst = {k_: (out[k_] - ref[k_]).abs().max().item() / (G_RTOL * s * max(ref[k_].abs().max().item(), 1e-3))
                         for k_ in ("dx", "dw", "dz0")}
                assert all(v <= 1.0 for v in worst.values()), worst
                m["worst_fraction_of_gradient_bar"] = worst
            return m
        ops = dict(x=x, w=w, z0=z0)
        if grad:
            ops["g"] = G
        return Case(ops, call, verify, name)
    return factory


_register("conv-fused", _conv(("cus", 1), 1, 4, 3, 3, 1, 1, 3, 4, name_has="conv_fused_kernel"))
_register("conv-fused-two-atom-tiles", _conv(("cus", 3), 1, 100, 3, 3, 1, 1, 9, 9, name_has="conv_fused_kernel"))
_register("conv-fused-bands", _conv(("cus/", 4), 1, 8, 3, 3, 1, 1, 32, 32, name_has="conv_fused_kernel"))
_register("conv-synth-few", _conv(3, 2, 24, 7, 7, 1, 3, 12, 11, name_has="conv_synth_few_kernel"))
_register("conv-synth", _conv(3, 8, 32, 3, 3, 1, 1, 12, 12, name_has="conv_synth_kernel"))
_register("conv-explicit-overlap-add", _conv(2, 17, 8, 3, 3, 1, 1, 6, 6, name_has="conv_residual_kernel"))
_register("conv-stride2", _conv(3, 2, 12, 3, 3, 2, 1, 6, 7, name_has="conv_residual_kernel"))
_register("conv-ista-explicit", _conv(2, 3, 20, 3, 5, (1, 2), (1, 2), 5, 6, name_has="conv_residual_kernel", fast=False))
_register("conv-stop-fused", _conv(("cus", 0), 1, 8, 3, 3, 1, 1, 12, 12, name_has="conv_fused_kernel", stop=True, seed=3))
_register("conv-stop-two-kernel", _conv(3, 8, 32, 3, 3, 1, 1, 12, 12, name_has="conv_synth_kernel", stop=True))
_register("conv-f64", _conv(3, 1, 100, 3, 3, 1, 1, 9, 9, name_has="", dtype=F64, maxiter=6))
_register("conv-f64-stride2", _conv(3, 2, 12, 3, 3, 2, 1, 6, 7, name_has="", dtype=F64, maxiter=6))
_register("conv-grad-f32", _conv(3, 8, 32, 3, 3, 1, 1, 12, 12, name_has="conv_synth_kernel", maxiter=6, grad=True))
_register("conv-grad-f32-fused-forward", _conv(("cus", 3), 1, 100, 3, 3, 1, 1, 9, 9, name_has="conv_fused_kernel", maxiter=6, grad=True))
_register("conv-grad-f32-stride2", _conv(3, 2, 12, 3, 3, 2, 1, 6, 7, name_has="conv_residual_kernel", maxiter=6, grad=True))
_register("conv-grad-f64", _conv(3, 2, 12, 3, 3, 2, 1, 6, 7, name_has="", dtype=F64, maxiter=6, grad=True))


def _bound_in_double(kernel, padding, sample=50):
    """tests/test_conv_f64_gpu.py::_bound_in_double: the Toeplitz bound on the grid 2 pi i / (sample - 1), in double"""
    ks = kernel.size(-1)
    if kernel.size(0) > kernel.size(1):
        kernel = kernel.transpose(0, 1)
    freq = 2 * math.pi * torch.arange(sample, dtype=F64) / (sample - 1)
    f0, f1 = torch.meshgrid(freq, freq, indexing="ij")
    pos = 1.0 + torch.arange(padding - ks, padding, dtype=F64)
    h0, h1 = torch.meshgrid(pos, pos, indexing="ij")
    phase = (f0.reshape(-1, 1) * h0.reshape(1, -1) + f1.reshape(-1, 1) * h1.reshape(1, -1)).T
    taps = kernel.flatten(2)
    re, im = torch.matmul(taps, torch.cos(phase)), torch.matmul(taps, torch.sin(phase))
    return (re.square().sum(1) + im.square().sum(1)).max(-1)[0].sum()


def _conv_auto_step(mode, dtype=F32):
    """lr='auto' / lr='exact': the step comes from lip_bound_conv2d / lip_constant on the stream of the call.  Checked in two
    parts, each at its own test's bar: the constant the call used (1e-5 of the oracle's bound, tests/test_conv_gpu.py::
    test_lipschitz_bound; lip_constant: conv_lip_cases.parity_bar), and the codes at 5e-5 of the oracle's at THAT step."""
    def factory():
        import conv_lip_cases as lc
        from lasso_amd.conv2d import ista_conv2d, lip_bound_conv2d, lip_constant
        nat, L = _nat()
        orc = _orc()
        spec, g = lc.CASES[lc.EXACT_LR_CASE], lc.load_case(_golden("conv_lip_cases"), lc.EXACT_LR_CASE)
        w, x = lc.kernel_of(spec, dtype), lc.exact_lr_image(spec, dtype)
        geo = lc.conv_kwargs(spec)
        Hz, Wz = lc.code_size(spec)
        z0 = torch.zeros(x.shape[0], spec["K"], Hz, Wz, dtype=dtype)
        T = 8

        def call(ops):
            if mode == "auto":
                const = lip_bound_conv2d(ops["w"], geo["padding"]).item()
            else:
                _, linfo = lip_constant(ops["w"], ops["x"].shape[-2:], return_info=True, **geo)
                const = linfo["theta"] + linfo["residual"]
            z, info = ista_conv2d(ops["x"], ops["z0"], ops["w"], lc.EXACT_LR_ALPHA, lr=mode, maxiter=T, tol=0.0,
                                  return_info=True, **geo)
            return dict(z=z), dict(info=info, constant=const)

        def verify(out, host):
            const = host["constant"]
            if mode == "auto":
                # (float64: lip_const.py:96-135 restated in double, 1e-12 -- tests/test_conv_f64_gpu.py::test_bound)
                ref_c = (orc.conv_lipschitz_bound(w, geo["padding"]) if dtype == F32 else _bound_in_double(w, geo["padding"])).item()
                dev, bar = abs(const - ref_c) / ref_c, 1e-5 if dtype == F32 else 1e-12
                lr = float(np.float32(1.0) / np.float32(const)) if dtype == F32 else 1.0 / const
            else:
                ref_c = float(g["ref64"][0])
                dev, bar = abs(const - ref_c) / ref_c, lc.parity_bar(g, dtype, lc.tol_of(spec, dtype)) + lc.tol_of(spec, dtype)
                lr = 1.0 / const
            assert dev <= bar, (const, ref_c, dev, bar)
            ref = orc.conv_fista(x, z0, w, lc.EXACT_LR_ALPHA, lr=lr, maxiter=T, tol=0.0, **geo)
            err = (out["z"] - ref).abs().max().item()
            assert err <= Z_BAR * (S29 if dtype == F64 else 1.0), err
            return dict(constant_rel=dev, constant_bar=bar, max_dz=err)
        name = L.lasso_conv_ista_kernel_name(x.shape[0], spec["C"], x.shape[2], x.shape[3], spec["K"], Hz, Wz, *spec["ks"],
                                             *_pair(spec["stride"]), *_pair(spec["padding"])).decode()
        return Case(dict(x=x, w=w, z0=z0), call, verify,
                    ("lasso_conv_lip_bound" if mode == "auto" else "lasso_conv_lip_constant") + " + " + name)
    return factory


_register("conv-lr-auto", _conv_auto_step("auto"))
_register("conv-lr-exact", _conv_auto_step("exact"))
_register("conv-lr-auto-f64", _conv_auto_step("auto", F64))


def _gpsr_conv(name, form):
    """tests/test_gpsr_conv_gpu.py::test_golden_case"""
    def factory():
        import gpsr_conv_cases as gc
        from lasso_amd.conv2d import gpsr_conv2d
        spec, gold = gc.CASES[name], gc.load_case(_golden("gpsr_conv_cases"), name)
        x, w, z0 = gc.case_inputs(spec)
        geo = dict(stride=spec["stride"], padding=spec["padding"])
        bars, gaps, _, _ = gc.z_bar(x, w, spec["tau"], z0=z0, **geo, **spec["kwargs"])

        def call(ops):
            with _quiet() as said:
                z, info = gpsr_conv2d(ops["x"], ops["w"], spec["tau"], z0=ops.get("z0"), return_info=True, **geo, **spec["kwargs"])
            return dict(z=z), dict(info=info, said=said)

        def verify(out, host):
            info, z = host["info"], out["z"]
            assert info["form"] == form, info["form"]
            assert info["iterations"] == int(gold["n_iter"]) + int(gold["db_iters"]) and list(info["trials"]) == list(gold["trials"])
            rows = gold["z_rows"]
            dev = dict(z=float(np.abs(gc.rows_of(z).numpy()[rows] - gold["z"]).max()),
                       lam=gc.max_rel(info["accepted_lambda"], gold["lam"]), obj=gc.max_rel(info["objective"], gold["objective"]))
            for key in ("z", "lam", "obj"):
                assert dev[key] <= bars[key], (key, dev[key], bars[key])
            return dict(hip=dev, bar=bars)
        ops = dict(x=x, w=w)
        if z0 is not None:
            ops["z0"] = z0
        return Case(ops, call, verify, "lasso_conv_gpsr_solve: " + form)
    return factory


_register("gpsr-conv-implicit", _gpsr_conv("gray7", "implicit"))
_register("gpsr-conv-implicit-debias", _gpsr_conv("debias", "implicit"))
_register("gpsr-conv-patches", _gpsr_conv("stride2", "patches"))
_register("gpsr-conv-implicit-warm", _gpsr_conv("warm", "implicit"))


def _lip_bound(tag):
    """1e-5 of the recorded value (tests/test_conv_gpu.py::test_lipschitz_bound)"""
    def factory():
        from lasso_amd.conv2d import lip_bound_conv2d
        g = _golden("conv_cases")
        w = torch.from_numpy(g[tag + "_w"])
        cfg = [int(v) for v in g[tag + "_cfg"]]
        pd = cfg[5]                                          # (N, C, K, ks, stride, padding, Hz, Wz)
        ref = float(g[tag + "_lip"])

        def call(ops):
            return dict(bound=lip_bound_conv2d(ops["w"], pd), root=lip_bound_conv2d(ops["w"], pd, sqrt=True)), {}

        def verify(out, host):
            err = abs(out["bound"].item() - ref) / ref
            assert err <= 1e-5 and abs(out["root"].item() - float(g[tag + "_lip_sqrt"])) <= 1e-5 * ref, err
            return dict(rel=err)
        return Case(dict(w=w), call, verify, "lasso_conv_lip_bound")
    return factory


def _lip_constant(name, dtype):
    """tests/test_conv_lip_gpu.py::test_value_matches_the_reference"""
    def factory():
        import conv_lip_cases as lc
        from lasso_amd.conv2d import lip_constant
        spec, g = lc.CASES[name], lc.load_case(_golden("conv_lip_cases"), name)
        w = lc.kernel_of(spec, dtype)
        kw = dict(tol=spec["tol"]) if "tol" in spec else {}

        def call(ops):
            v, info = lip_constant(ops["w"], lc.imsize_of(spec, False), return_info=True, **kw, **lc.conv_kwargs(spec))
            return {}, dict(value=v, info=info)

        def verify(out, host):
            ref64, bar = float(g["ref64"][0]), lc.parity_bar(g, dtype, lc.tol_of(spec, dtype))
            dev = abs(host["value"] - ref64) / ref64
            assert host["info"]["status"] in ("converged", "breakdown") and dev <= bar, (dev, bar, host["info"]["status"])
            return dict(dev=dev, bar=bar, steps=host["info"]["steps"], status=host["info"]["status"])
        return Case(dict(w=w), call, verify, "lasso_conv_lip_constant (%s), dim %d" % ("double" if dtype == F64 else "float", min(lc.dims(spec))))
    return factory


_register("lip-bound-a", _lip_bound("a"))
_register("lip-bound-c", _lip_bound("c"))
for _name in ("rgb", "c16", "rect_s2", "exhaust"):
    _register("lip-constant-f32-" + _name, _lip_constant(_name, F32))
_register("lip-constant-f64-rgb", _lip_constant("rgb", F64))
_register("lip-constant-f64-few-atoms", _lip_constant("few_atoms", F64))


# ======================================================================================================================
# the tests
# ======================================================================================================================
CASE_IDS = sorted(_FACTORY)


@pytest.mark.parametrize("mode", MODES + ("stream",))
@pytest.mark.parametrize("cid", CASE_IDS)
def test_case(cid, mode):
    _check(cid, mode)


def test_not_reproducible_table_names_registered_cases():
    assert set(_NOT_REPRODUCIBLE) <= set(_FACTORY)


def test_shared_tag_through_the_real_cache_big_small_big():
    """The default 'fista' tag is shared by `ista` and HipEngine.fista_run: through the REAL cache, unpoisoned, in the order
    big, small, big each call finds what the other left (the small call a buffer larger than it asked for, the big ones
    the other entry point's state) and returns its own anchor bit for bit."""
    from lasso_amd import _native as nat
    from lasso_amd.engine import HipEngine
    from lasso_amd.linear.solvers import ista
    nat.release_workspaces()
    eng = HipEngine()
    Xb, Wb = (t.cuda() for t in _problem(4900, 256, 1024, 77))
    Xs, Ws = (t.cuda() for t in _problem(40, 100, 512, 2))
    z0b, z0s = torch.zeros(4900, 1024, device="cuda"), _start(40, 512, 102).cuda()
    lrb, lrs = _lr(Wb.cpu()), _lr(Ws.cpu())

    def big():
        return ista(Xb, z0b, Wb, 0.2, lr=lrb, maxiter=11, tol=0.0)

    def small():
        z, y, delta = eng.fista_run(Xs, Ws, z0s, None, 0.2, lrs, True, 0, 7, True)
        return torch.cat([z.flatten(), y.flatten(), delta])

    with Poison("zero").installed():
        want_big, want_small = big().cpu(), small().cpu()
    nat.release_workspaces()
    key_count = len(nat._WS)
    got = [big().cpu(), small().cpu(), big().cpu(), small().cpu()]
    assert len(nat._WS) == key_count + 1                      # one tag, one buffer: they really shared it
    assert torch.equal(got[0], want_big) and torch.equal(got[2], want_big)
    assert torch.equal(got[1], want_small) and torch.equal(got[3], want_small)
    assert (want_big - _orc().fista(Xb.cpu(), z0b.cpu(), Wb.cpu(), 0.2, lr=lrb, maxiter=11, tol=0.0)).abs().max().item() <= Z_BAR


# ---- the harness catches what it is for (the GPU twins of tests/test_workspace_cpu.py) --------------------------------------
def test_the_stream_harness_flags_an_op_on_the_default_stream():
    """a fake solver (plain torch) that enqueues ONE op on the default stream: there the operand is still NaN"""
    x = torch.randn(1000, generator=torch.Generator().manual_seed(0))

    def honest(ops):
        return dict(y=ops["x"] * 2.0 + 1.0), {}

    def stray(ops):
        with torch.cuda.stream(torch.cuda.default_stream()):
            doubled = ops["x"] * 2.0                          # not ordered behind the side stream's copies
        return dict(y=doubled + 1.0), {}
    want = dict(y=x * 2.0 + 1.0), {}
    assert not _differences(_run_late(honest, dict(x=x)), want)
    for attempt in range(6):                  # (six streams of torch's pool in a row: every hardware queue has its turn)
        assert _differences(_run_late(stray, dict(x=x)), want), attempt
    torch.cuda.synchronize()


def test_the_poison_harness_flags_an_overrun_and_an_uninitialised_sum_on_the_device():
    from lasso_amd import _native as nat

    def sums_scratch(x):
        ws = nat.workspace(x.device, 64, "fake")
        return x.sum() + ws[:16].view(torch.float32).sum()

    def overruns(x):
        ws = nat.workspace(x.device, 64, "fake")
        torch.as_strided(ws, (ws.numel() + 1,), (1,))[-1] = 7
        return x.sum()
    x = torch.ones(8, device="cuda")
    results = {}
    for mode in MODES:
        with Poison(mode).installed():
            results[mode] = sums_scratch(x).item()
    assert results["zero"] == 8.0 and not all(_same(results[m], results["zero"]) for m in MODES)
    for mode in MODES:
        with pytest.raises(GuardBroken):
            with Poison(mode).installed():
                overruns(x)
