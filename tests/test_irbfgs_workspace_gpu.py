"""lasso_irbfgs_solve under the scratch and stream contract of include/lasso_hip.h, with the treatment of
tests/ws_poison.py and the harness of tests/test_workspace_gpu.py (its Case, its late side stream, its bitwise
comparison -- used, not copied):

  zero    the anchor, on scratch of zeros between guard bands: verified against the recorded run at the bar of
          tests/test_irbfgs_gpu.py
  ones / fives / roomy   scratch of 0xFF (NaN) / 0x55 (large finite floats, plausible ints) / 0xFF with room to spare:
          the codes and everything the call reports must equal the anchor's BIT FOR BIT, and both guard bands hold
  stream  the call on a fresh side stream whose operands arrive late: the same bits again, so nothing was enqueued on
          another stream

What the scratch holds that a stale value could reach: B and the emitted systems (the strict upper triangles of the
systems are never written on the Cholesky route and never read by it), z_prev / g_prev (written by the first launch of
the row kernel before any update reads them), the per-row verdicts, the partial sums, the control record and the batch
solver's own scratch."""
import pytest
import torch

import irbfgs_cases
import test_workspace_gpu as wsg
from margins import record_margins

pytestmark = pytest.mark.gpu


def _irbfgs_run(ops, spec):
    from lasso_amd.nonlinear import iterative_ridge_bfgs, rss
    return iterative_ridge_bfgs(rss(ops["x"], ops["w"]), ops["z0"], alpha=spec["alpha"], return_info=True, **spec["kwargs"])


# fixed steps and Brent on the ragged LDS-tier shape and on the general tier (k > 256: the solver's scratch triangles)
NAMES = ("fixed12_lds70", "brent4_lds70", "fixed4_general", "brent4_general")
_CASES, _ANCHORS = {}, {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = wsg._spread_case(irbfgs_cases, "irbfgs_cases", name, _irbfgs_run, "lasso_irbfgs_solve")()
    return _CASES[name]


def _anchor(name):
    if name not in _ANCHORS:
        _ANCHORS[name] = wsg._run(_case(name), "zero")
    return _ANCHORS[name]


@pytest.mark.parametrize("name", NAMES)
def test_anchor_meets_the_recorded_run(name):
    margins = _case(name).verify(*_anchor(name))
    print("irbfgs workspace/%s: %s" % (name, margins))
    record_margins("irbfgs/workspace_" + name, margins)


@pytest.mark.parametrize("mode", ["ones", "fives", "roomy", "stream"])
@pytest.mark.parametrize("name", NAMES)
def test_same_bits_whatever_the_scratch_held(name, mode):
    case, want = _case(name), _anchor(name)
    got = wsg._run_late(case.call, case.operands) if mode == "stream" else wsg._run(case, mode)
    bad = wsg._differences(got, want)
    assert not bad, "%s on %s differs from the anchor: %s" % (
        name, "a late side stream" if mode == "stream" else "scratch of mode '%s'" % mode, "; ".join(bad))
    assert torch.isfinite(got[0]["z"]).all()
