"""lasso_ista_nl_solve under the scratch and stream contract of include/lasso_hip.h, with the treatment of
tests/ws_poison.py and the harness of tests/test_workspace_gpu.py (its Case, its late side stream, its bitwise
comparison -- used, not copied):

  zero    the anchor, on scratch of zeros between guard bands: verified against the recorded run at the bar of
          tests/test_ista_nl_gpu.py
  ones / fives / roomy   scratch of 0xFF (NaN) / 0x55 (large finite floats, plausible ints) / 0xFF with room to spare:
          the codes and everything the call reports must equal the anchor's BIT FOR BIT, and both guard bands hold
  stream  the call on a fresh side stream whose operands arrive late: the same bits again, so nothing was enqueued on
          another stream

What the scratch holds that a stale value could reach: z, y and their checkpoints, r, c and q, both vectors of the power
iteration, the rows' scales, L and t, the rows' column-block sums, the block partials, the chunk's record."""
import pytest
import torch

import test_workspace_gpu as wsg
from ista_nl_cases import CASES, case_inputs, load_case
from margins import record_margins
from test_ista_nl_gpu import bar_of

pytestmark = pytest.mark.gpu

# a fixed step and 'auto' across block boundaries; k beyond 4096; a stop inside a speculated chunk (a replay), under both rules
NAMES = ("relu_blocks_fixed", "sigmoid_blocks_auto", "identity_wide_auto", "sigmoid_mid_stop", "tanh_small_stop_auto")
_CASES, _ANCHORS = {}, {}


def _case(golden, name):
    if name not in _CASES:
        spec, g = CASES[name], load_case(golden("ista_nl_cases"), name)
        x, w, b, z0, u0 = case_inputs(spec)
        operands = dict(x=x, w=w, z0=z0, u0=u0)
        if b is not None:
            operands["b"] = b

        def call(ops):
            from lasso_amd.nonlinear import affine, ista_nl
            with wsg._quiet() as said:
                z, report = ista_nl(ops["x"], ops["z0"], affine(ops["w"], ops.get("b"), spec["activation"]), alpha=spec["alpha"],
                                    power_init=ops["u0"], return_info=True, verbose=2, **spec["kwargs"])
            tensors = dict(z=z)
            if report["L"] is not None:
                tensors["L"] = report.pop("L")
            return tensors, dict(report=report, said=said)

        def verify(out, host):
            dz = float((out["z"] - torch.from_numpy(g["z32"])).abs().max())
            assert torch.isfinite(out["z"]).all() and host["report"]["iterations"] == len(g["deltas32"]) and dz <= bar_of(g)
            return dict(dz=dz, bar=bar_of(g))
        _CASES[name] = wsg.Case(operands, call, verify, "lasso_ista_nl_solve")
    return _CASES[name]


def _anchor(golden, name):
    if name not in _ANCHORS:
        _ANCHORS[name] = wsg._run(_case(golden, name), "zero")
    return _ANCHORS[name]


@pytest.mark.parametrize("name", NAMES)
def test_anchor_meets_the_recorded_run(golden, name):
    margins = _case(golden, name).verify(*_anchor(golden, name))
    print("ista_nl workspace/%s: %s" % (name, margins))
    record_margins("ista_nl/workspace_" + name, margins)


@pytest.mark.parametrize("mode", ["ones", "fives", "roomy", "stream"])
@pytest.mark.parametrize("name", NAMES)
def test_same_bits_whatever_the_scratch_held(golden, name, mode):
    case, want = _case(golden, name), _anchor(golden, name)
    got = wsg._run_late(case.call, case.operands) if mode == "stream" else wsg._run(case, mode)
    bad = wsg._differences(got, want)
    assert not bad, "%s on %s differs from the anchor: %s" % (
        name, "a late side stream" if mode == "stream" else "scratch of mode '%s'" % mode, "; ".join(bad))
    assert torch.isfinite(got[0]["z"]).all()
