"""tests/ws_poison.py on CPU tensors: what the harness hands out (fill patterns, exact size, alignment, the roomy size,
the guard bands), how it patches and restores, and that it CATCHES what it is for -- two fake torch-only "solvers", one
that sums four uninitialised floats of its scratch into its result and one that writes one byte past its scratch, are
both flagged.  (The GPU twins, and a fake solver that enqueues an op on the default stream, are in
tests/test_workspace_gpu.py.)"""
import types

import pytest
import torch

import ws_poison
from ws_poison import FILL, GUARD, MODES, ROOM, SENTINEL, GuardBroken, Poison

CPU = torch.device("cpu")


def _fake_library():
    """stand-ins for lasso_amd._native and HipEngine: the harness patches attributes, nothing else"""
    def workspace(device, nbytes, tag="fista"):
        return torch.zeros(max(int(nbytes), 1), dtype=torch.uint8, device=device)

    class Engine:
        device = CPU

        def fista_workspace(self, n, d, k, cap):
            return {"buf": torch.zeros(n * k + cap, dtype=torch.uint8), "packed": False, "shape": (n, d, k), "cap": cap}
    return types.SimpleNamespace(workspace=workspace), Engine


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbytes", [1, 4, 255, 256, 4097, 100000])
def test_fill_size_and_guards(mode, nbytes):
    p = Poison(mode)
    ws = p.workspace(CPU, nbytes, "t")
    want = nbytes + (ROOM if mode == "roomy" else 0)
    assert ws.dtype == torch.uint8 and ws.numel() == want and ws.is_contiguous()
    assert bool((ws == FILL[mode]).all())
    (tag, asked, alloc, view), = p.requests
    assert (tag, asked) == ("t", nbytes) and view is ws
    # the view's base sits GUARD bytes into an allocation of its own: the allocator's alignment is kept (256 | 4096)
    assert ws.data_ptr() - alloc.data_ptr() == GUARD and GUARD % 256 == 0
    assert alloc.numel() == GUARD + want + GUARD
    assert bool((alloc[:GUARD] == SENTINEL).all()) and bool((alloc[GUARD + want:] == SENTINEL).all())
    assert SENTINEL not in FILL.values()
    assert p.check() == 1


def test_patterns_read_as_the_table_says():
    ones, fives = Poison("ones").workspace(CPU, 16), Poison("fives").workspace(CPU, 16)
    assert torch.isnan(ones.view(torch.float32)).all() and torch.isnan(ones.view(torch.float64)).all()
    assert torch.isnan(ones.view(torch.bfloat16)).all() and bool((ones.view(torch.int32) == -1).all())
    f = fives.view(torch.float32)
    assert torch.isfinite(f).all() and bool((f > 1e13).all()) and torch.isfinite(fives.view(torch.float64)).all()
    assert bool((fives.view(torch.int32) == 0x55555555).all())
    assert (ROOM, ROOM % 8) == ((1 << 20) + 4, 4)            # roomy: no multiple of a double


def test_an_empty_request_gets_one_byte_like_the_cache():
    assert Poison("ones").workspace(CPU, 0).numel() == 1


def test_every_request_is_fresh_and_kept_alive():
    p = Poison("zero")
    a, b = p.workspace(CPU, 64, "same"), p.workspace(CPU, 64, "same")
    assert a.data_ptr() != b.data_ptr() and len(p.requests) == 2


def test_install_patches_by_attribute_and_restores(monkeypatch):
    nat, Engine = _fake_library()
    keep = nat.workspace, Engine.fista_workspace
    with Poison("fives").installed(nat, Engine) as p:
        ws = nat.workspace(CPU, 32, "x")
        held = Engine().fista_workspace(3, 2, 5, 7)
        assert bool((ws == 0x55).all()) and ws.numel() == 32
        # the engine's own dict, its buffer swapped for a poisoned one of exactly its size, filled once
        assert held["shape"] == (3, 2, 5) and held["cap"] == 7 and held["packed"] is False
        assert held["buf"].numel() == 3 * 5 + 7 and bool((held["buf"] == 0x55).all())
        assert [r[0] for r in p.requests] == ["x", "fista_workspace"]
    assert (nat.workspace, Engine.fista_workspace) == keep
    with monkeypatch.context() as mp:
        p = Poison("ones").install(mp, nat, Engine)
        assert bool((nat.workspace(CPU, 8) == 0xFF).all())
        assert Engine().fista_workspace(1, 1, 4, 4)["buf"].numel() == 8
        assert p.check() == 2
    assert (nat.workspace, Engine.fista_workspace) == keep


def test_the_patch_is_restored_when_the_call_raises():
    nat, Engine = _fake_library()
    keep = nat.workspace
    with pytest.raises(ZeroDivisionError):
        with Poison("ones").installed(nat, Engine):
            1 / 0
    assert nat.workspace is keep


def test_unknown_mode():
    with pytest.raises(ValueError):
        Poison("twos")


# ---- the harness catches what it is for -----------------------------------------------------------------------------
def _solver_ok(nat, x):
    ws = nat.workspace(x.device, 64, "fake").view(torch.float32)
    ws[:4] = x[:4] * 2.0                     # written before it is read
    return x.sum() + ws[:4].sum()


def _solver_sums_uninitialised_scratch(nat, x):
    ws = nat.workspace(x.device, 64, "fake").view(torch.float32)
    return x.sum() + ws[:4].sum()            # "a partial sum the launcher forgot to clear"


def _solver_writes_past_its_scratch(nat, x):
    ws = nat.workspace(x.device, 64, "fake")
    torch.as_strided(ws, (ws.numel() + 1,), (1,))[-1] = 7         # one byte past what it was handed
    return x.sum()


def _solver_writes_in_front_of_its_scratch(nat, x):
    ws = nat.workspace(x.device, 64, "fake")
    torch.as_strided(ws, (1,), (1,), ws.storage_offset() - 1)[0] = 7
    return x.sum()


def _solver_sized_by_the_buffer(nat, x):
    ws = nat.workspace(x.device, 64, "fake")
    return x.sum() + float(ws.numel())       # "a carve-up derived from the passed size instead of the shape"


def _run_modes(solver):
    """-> {mode: result}; the guards are checked on the way out of every mode"""
    nat, Engine = _fake_library()
    out = {}
    for mode in MODES:
        with Poison(mode).installed(nat, Engine):
            out[mode] = solver(nat, torch.arange(8, dtype=torch.float32)).item()
    return out


def _matches_anchor(out):
    return all(out[m] == out["zero"] for m in MODES)


def test_a_well_behaved_solver_passes():
    out = _run_modes(_solver_ok)
    assert out["zero"] == 28.0 + 12.0 and _matches_anchor(out)


def test_a_solver_that_sums_uninitialised_scratch_is_flagged():
    out = _run_modes(_solver_sums_uninitialised_scratch)
    assert out["zero"] == 28.0                                     # right on zeroed scratch: today's suite sees this
    assert out["ones"] != out["ones"] and out["roomy"] != out["roomy"]       # NaN
    assert out["fives"] > 1e13                                     # finite, and nowhere near
    assert not _matches_anchor(out)


def test_a_solver_sized_by_the_buffer_is_flagged_by_roomy_alone():
    out = _run_modes(_solver_sized_by_the_buffer)
    assert out["zero"] == out["ones"] == out["fives"] and out["roomy"] == out["zero"] + ROOM
    assert not _matches_anchor(out)


@pytest.mark.parametrize("solver,band", [(_solver_writes_past_its_scratch, "back"), (_solver_writes_in_front_of_its_scratch, "front")])
@pytest.mark.parametrize("mode", MODES)
def test_a_solver_that_writes_outside_its_scratch_is_flagged(solver, band, mode):
    nat, Engine = _fake_library()
    with pytest.raises(GuardBroken) as e:
        with Poison(mode).installed(nat, Engine):
            assert solver(nat, torch.arange(8, dtype=torch.float32)).item() == 28.0     # the result itself is right
    assert "%s guard" % band in str(e.value) and "'fake'" in str(e.value)
    assert ("offset %d " % (-1 if band == "front" else 64 + (ROOM if mode == "roomy" else 0))) in str(e.value) + " "


def test_module_constants():
    assert ws_poison.GUARD == 4096 and set(MODES) == {"zero", "ones", "fives", "roomy"}
