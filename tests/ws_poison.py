"""Caller-owned scratch with unspecified contents (include/lasso_hip.h, "Scratch and stream contract").
TEST INFRASTRUCTURE, plain torch: no kernel of the library is reimplemented here.

``Poison(mode)`` replaces ``lasso_amd._native.workspace`` and ``HipEngine.fista_workspace`` -- every Python caller
reaches the scratch cache through ``nat.workspace(...)`` by module attribute, so one patch reaches all of them.  Every
request gets a FRESH allocation that lives until the case ends:

    [ 4096 bytes of GUARD | the view handed out | 4096 bytes of GUARD ]

The view's ``numel()`` is exactly the requested size (``roomy``: 1 MiB + 4 bytes more), its base sits 4096 bytes into the
allocation (the allocator's alignment -- 512 bytes on a HIP device -- is kept, so 256-byte alignment holds), and it is
filled on the CURRENT stream before it is returned:

    zero   0x00  exact   the anchor
    ones   0xFF  exact   NaN as f32 / f64 / bf16, -1 as int32
    fives  0x55  exact   a large finite float (1.47e13 as f32, 1.2e103 as f64) and a plausible positive int: shows
                         where an fmaxf, a `<=` or a min / max fold swallows a NaN
    roomy  0xFF  request + 1 MiB + 4   a carve-up derived from the size passed in instead of from the shape

A multi-call protocol (lasso_fista_prepare / _run through fista_workspace) is filled once, when its workspace is made.
``check()`` synchronises and asserts that both guard bands of every request are bit for bit intact: an overrun of
``*_workspace_bytes`` no longer lands in the caching allocator's rounding slack."""
import contextlib

import torch

GUARD = 4096
SENTINEL = 0xA5
ROOM = (1 << 20) + 4
FILL = {"zero": 0x00, "ones": 0xFF, "fives": 0x55, "roomy": 0xFF}
MODES = tuple(FILL)


class GuardBroken(AssertionError):
    pass


class Poison:
    def __init__(self, mode):
        if mode not in FILL:
            raise ValueError("mode %r: one of %s" % (mode, ", ".join(MODES)))
        self.mode = mode
        self.requests = []            # (tag, nbytes asked for, allocation, view)

    # -- the replacement of nat.workspace ----------------------------------------------------------------------------
    def workspace(self, device, nbytes, tag="fista"):
        asked = max(int(nbytes), 1)                                   # (nat.workspace never hands out an empty buffer)
        size = asked + (ROOM if self.mode == "roomy" else 0)
        alloc = torch.empty(GUARD + size + GUARD, dtype=torch.uint8, device=device)
        alloc[:GUARD].fill_(SENTINEL)
        alloc[GUARD + size:].fill_(SENTINEL)
        view = alloc[GUARD:GUARD + size]
        view.fill_(FILL[self.mode])                                   # on the current stream, like the call behind it
        self.requests.append((tag, asked, alloc, view))
        return view

    def fista_workspace(self, original):
        """the replacement of HipEngine.fista_workspace: the engine's own dict, its buffer swapped for a poisoned one"""
        poison = self

        def fista_workspace(engine, n, d, k, cap):
            ws = original(engine, n, d, k, cap)
            ws["buf"] = poison.workspace(engine.device, ws["buf"].numel(), "fista_workspace")
            return ws
        return fista_workspace

    # -- installing --------------------------------------------------------------------------------------------------
    def install(self, monkeypatch, nat=None, engine_cls=None):
        """through pytest's monkeypatch (undone by the fixture); nat / engine_cls: stand-ins for the CPU tests"""
        if nat is None:
            from lasso_amd import _native as nat
        if engine_cls is None:
            from lasso_amd.engine import HipEngine as engine_cls
        monkeypatch.setattr(nat, "workspace", self.workspace)
        monkeypatch.setattr(engine_cls, "fista_workspace", self.fista_workspace(engine_cls.fista_workspace))
        return self

    @contextlib.contextmanager
    def installed(self, nat=None, engine_cls=None, sync=None):
        """with Poison(mode).installed() as p: ...; the guards are checked on the way out (sync: see check())"""
        if nat is None:
            from lasso_amd import _native as nat
        if engine_cls is None:
            from lasso_amd.engine import HipEngine as engine_cls
        keep = nat.workspace, engine_cls.fista_workspace
        nat.workspace = self.workspace
        engine_cls.fista_workspace = self.fista_workspace(keep[1])
        try:
            yield self
        finally:
            nat.workspace, engine_cls.fista_workspace = keep
        self.check(sync)

    # -- the verdict -------------------------------------------------------------------------------------------------
    def check(self, sync=None):
        """after a synchronise: both guard bands of every request still hold the sentinel.  sync: what to wait with
        instead of the whole device (a side stream's .synchronize, where the default stream must be left alone)"""
        if sync is not None:
            sync()
        elif any(alloc.is_cuda for _, _, alloc, _ in self.requests):
            torch.cuda.synchronize()
        for tag, asked, alloc, view in self.requests:
            size = view.numel()
            for name, band in (("front", alloc[:GUARD]), ("back", alloc[GUARD + size:])):
                bad = (band != SENTINEL).nonzero()
                if bad.numel():
                    at = int(bad[0])
                    where = at - GUARD if name == "front" else size + at
                    raise GuardBroken("workspace %r (%d bytes asked, %d handed out, mode %s): %d byte(s) of the %s guard "
                                      "overwritten, the first at offset %d of the workspace"
                                      % (tag, asked, size, self.mode, bad.numel(), name, where))
        return len(self.requests)

    def release(self):
        self.requests = []
