"""The EM loop's host side does what it did before the engine's precision table (engine._ENTRY): dict_learning(steps=3)
takes the same forms of the loop (em_stats) and creates the same workspace cache entries -- a method that went through
another entry point, asked for a second workspace or lost its tag would show here.  The expected values were recorded
from the commit before the table, on the same machine, in one job with this test."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

# recorded from the parent commit
EXPECTED = {
    "f32": dict(engines=1, stats={"deferred_verdicts": 3, "overlapped_steps": 3, "speculative_sweeps": 3},
                ws_tags=["fista", "gram", "obj", "sweep"]),
    "f64": dict(engines=1, stats={}, ws_tags=["fista", "gram_f64", "obj", "sweep_f64"]),
}


def _inputs(kind):
    if kind == "f32":                        # config 5's shape, 64 rows
        from recipes import recipe_c4_init, recipe_c5
        return recipe_c5(64), recipe_c4_init(64, 256)
    g = torch.Generator().manual_seed(5)     # float64: n, d, k = 37, 10, 50
    X = torch.randn(37, 10, generator=g, dtype=torch.float64)
    return X, torch.nn.functional.normalize(torch.randn(10, 50, generator=g, dtype=torch.float64), dim=0)


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_em_loop_counters_and_workspace_keys(kind, monkeypatch):
    from lasso_amd import _native as nat
    from lasso_amd.engine import HipEngine
    dl = importlib.import_module("lasso_amd.linear.dict_learning")
    made = []

    class Counting(HipEngine):
        def __init__(self, device=None):
            super().__init__(device)
            self.em_stats = {}
            made.append(self)
    monkeypatch.setattr(dl, "HipEngine", Counting)
    X, W = (t.cuda() for t in _inputs(kind))
    nat.release_workspaces()
    weight, losses = dl.dict_learning(X, W.shape[1], alpha=0.1, steps=3, progbar=False, init_weight=W)
    torch.cuda.synchronize()
    stats = {}
    for e in made:
        for name, v in e.em_stats.items():
            stats[name] = stats.get(name, 0) + v
    got = dict(engines=len(made), stats=stats, ws_tags=sorted(key[-1] for key in nat._WS))
    print(kind, got)
    assert losses.dtype == X.dtype and torch.isfinite(losses).all() and len(losses) == 3
    assert got == EXPECTED[kind]
