"""The stop rule's speculate-and-replay drivers on the device, at the places the other suites do not reach: the
checkpoint of a strided z_out (the non-compact save / restore of the unfused fp32 solve, the 2-D copies of the float64
one), and the schedule of the row-shard driver in Python against the chunked form of lasso_fista_solve."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, D, K, LDZ, SENTINEL = 60, 300, 40, 48, -7.25
ALPHA, MAXITER = 0.3, 60
# chosen with the oracle's sums (they stay >= 14 % away from each budget) and the chunk sizes the driver derives from them
# (next_stop_chunk): the rule fires at iteration 8 (chunks of 1, 5, 3 iterations), 19 (1, 10, 5, 4) and 36 (1, 16, 6, 6, 8)
# -- each time strictly inside the last chunk, so the checkpoint is restored and the stopping iteration replayed
TOLS = (4.5e-3, 1.8e-4, 4e-6)


@pytest.fixture(scope="module")
def unfused_problem():
    from oracle import lasso_oracle as orc
    g = torch.Generator().manual_seed(7)
    W = torch.nn.functional.normalize(torch.randn(D, K, generator=g), dim=0)
    X = torch.randn(N, D, generator=g)
    return X, W, 1.0 / orc.lipschitz_constant(W, "exact")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_stop_inside_a_chunk_with_a_strided_z_out(unfused_problem, dtype):
    """z_out as the first 40 columns of a [60, 48] tensor (ldz != k; every Python caller passes a contiguous z_out): the
    checkpoint at the head of a chunk and its restore copy a strided state.  Three tolerances whose stops fall inside a
    chunk: the oracle's iteration count, bit for bit the codes of the contiguous solve, padding columns untouched."""
    from lasso_amd import _native as nat
    from oracle import lasso_oracle as orc
    X, W, lr = unfused_problem
    X, W = X.to(dtype), W.to(dtype)
    Xg, Wg, L = X.cuda(), W.cuda(), nat.lib()
    f64 = dtype == torch.float64

    def solve(z, tol):
        nbytes = L.lasso_fista_workspace_bytes(N, D, K, nat.LASSO_F64 if f64 else nat.LASSO_F32, MAXITER, tol,
                                               nat.STOP_GLOBAL, 0)
        ws = nat.workspace(Xg.device, nbytes)
        iters = C.c_int32(0)
        head = (nat.ptr(Xg), Xg.stride(0), nat.ptr(Wg), Wg.stride(0), None, 0, nat.ptr(z), z.stride(0), N, D, K)
        args = (ALPHA, lr, 1, MAXITER, tol, nat.STOP_GLOBAL, 0, 1.5, C.byref(iters))
        tail = (None, None, None, None, nat.ptr(ws), ws.numel(), nat.stream_ptr(Xg.device))
        if f64:
            last = C.c_double(float("nan"))
            nat.check(L.lasso_fista_solve_f64(*head, *args, C.byref(last), *tail))
        else:
            last = C.c_float(float("nan"))
            nat.check(L.lasso_fista_solve(*head, nat.LASSO_F32, *args, C.byref(last), *tail))
        torch.cuda.synchronize()
        return iters.value, last.value

    stops = []
    for tol in TOLS:
        tr = orc.FistaTrace()
        orc.fista(X, torch.zeros(N, K, dtype=dtype), W, ALPHA, lr=lr, maxiter=MAXITER, tol=tol, trace=tr)
        assert tr.stopped and 3 <= tr.iterations <= MAXITER - 1
        flat = torch.empty(N, K, dtype=dtype, device="cuda")
        wide = torch.full((N, LDZ), SENTINEL, dtype=dtype, device="cuda")
        it_f, last_f = solve(flat, tol)
        it_w, last_w = solve(wide[:, :K], tol)
        print("dtype %s tol %g: oracle %d iterations, contiguous %d, strided %d, last delta %r / %r"
              % (dtype, tol, tr.iterations, it_f, it_w, last_f, last_w))
        assert it_w == tr.iterations and it_f == tr.iterations, (tol, it_w, it_f, tr.iterations)
        assert last_w == last_f
        assert torch.equal(wide[:, K:], torch.full((N, LDZ - K), SENTINEL, dtype=dtype, device="cuda")), tol
        assert torch.equal(wide[:, :K], flat), (tol, (wide[:, :K] - flat).abs().max().item())
        stops.append(tr.iterations)
    assert len(set(stops)) == len(TOLS)


def test_row_shard_driver_keeps_the_schedule_of_the_chunked_form(monkeypatch, tmp_path):
    """parallel.sharded_encode on ONE rank with LASSO_FORCE_COLLECTIVES=1 (chunks of lasso_fista_run, their sums
    all-reduced) against ista(stop_mode='chunked') (lasso_fista_solve's chunked form) on 300 x 48 x 160 with a tolerance
    that needs more than 64 iterations, so several chunks and a replay: same iteration count, same last sum bit for bit,
    same codes bit for bit.  The stop decision is exact and the replay bitwise under ANY chunk sizes, so this holds the two
    drivers to the same result, not their sizers to the same schedule: that is tests/test_stoprule_host_cpu.py's twin test."""
    import torch.distributed as dist
    from lasso_amd.engine import HipEngine
    from lasso_amd.linear.solvers.ista import ista
    from lasso_amd.parallel import sharded_encode
    n, d, k, alpha, lr, maxiter, tol = 300, 48, 160, 0.3, 0.1, 300, 1e-4
    g = torch.Generator().manual_seed(5)
    W = torch.nn.functional.normalize(torch.randn(d, k, generator=g), dim=0).cuda()
    X = torch.randn(n, d, generator=g).cuda()
    z_c, info_c = ista(X, torch.zeros(n, k, device="cuda"), W, alpha, lr=lr, maxiter=maxiter, tol=tol,
                       stop_mode='chunked', return_info=True)
    monkeypatch.setenv("LASSO_FORCE_COLLECTIVES", "1")
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "rendezvous"), rank=0, world_size=1)
    try:
        z_s, info_s = sharded_encode(HipEngine(), X, W, alpha, None, lr=lr, maxiter=maxiter, tol=tol, return_info=True)
    finally:
        dist.destroy_process_group()
    print("chunked form: %r; row-shard driver: %r" % (info_c, info_s))
    assert 64 < info_c["iterations"] < maxiter
    assert info_s["iterations"] == info_c["iterations"]
    assert np.float32(info_s["last_delta"]).tobytes() == np.float32(info_c["last_delta"]).tobytes()
    assert torch.equal(z_s, z_c), (z_s - z_c).abs().max().item()
