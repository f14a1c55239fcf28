"""The golden cases of OWL-QN on the logistic objective (tests/golden/owlqn_glm_cases.npz): shapes, seeds and
arguments, shared by the generator (tests/golden/generate_golden_owlqn_glm.py) and the tests.  Inputs: unit-norm atoms,
logits u* = 3 code W^T of a 10 %-sparse code, targets x ~ Bernoulli(sigmoid(u*)) (one case: the soft targets
sigmoid(u*) themselves), alpha 0.1 and a zero start unless the case says otherwise.

The generator certified every case by the rules of tests/owlqn_cases.py, whose caps and ``rtol_of`` are used as they
are: no backtracking decision within 1e-4 |f| of its bound, no y.s within a factor 10 of 1e-10, no |dx| within 1 % of
xtol; spread_z / spread_f are how far "another correct float32 implementation" moves the codes / the objective --
tests/owlqn_glm_model.py with permuted summation orders and the vector-free direction, either objective fold, and the
link evaluated in float64 and rounded once against torch's float32 operations.  ``compare``: "z" the codes (spread_z
<= 2.5e-3), "f" the objective only (spread_f <= 1e-4), "props" neither (a backtracking descends, a Brent iteration ends at the
best step its search evaluated, the reported objective is the objective of the returned codes)."""
import torch
import torch.nn.functional as F

from owlqn_cases import MID, ORDER_SEEDS, RAGGED, SMALL, SPREAD_F_CAP, SPREAD_Z_CAP, TALL, WIDE  # noqa: F401
from owlqn_cases import admitted_f, admitted_z, load_case, rtol_of  # noqa: F401

SATURATION = 120.0                    # max |z0 W^T| of a saturated start: exp(120) is not a float32


def _case(shape, seed, compare, alpha=0.1, start="zero", targets="hard", **kwargs):
    n, d, k = shape
    return dict(n=n, d=d, k=k, seed=seed, alpha=alpha, start=start, targets=targets, kwargs=kwargs, compare=compare)


_NONE = dict(line_search="none", lr=0.05, history_size=2, max_iter=6)
_BT = dict(line_search="backtrack", history_size=3, max_iter=6)
_B1 = dict(line_search="brent", max_iter=1)
_B8 = dict(line_search="brent", history_size=3, max_iter=8)

CASES = {
    # every shape under the three line searches: the codes where the spread admits it, else the objective
    "none_small": _case(SMALL, 0, "z", **_NONE),
    "bt_small": _case(SMALL, 0, "z", **_BT),
    "brent_small": _case(SMALL, 0, "z", **_B1),
    "none_mid": _case(MID, 0, "z", **_NONE),
    "bt_mid": _case(MID, 0, "z", **_BT),
    "brent_mid": _case(MID, 0, "z", **_B1),
    "none_wide": _case(WIDE, 0, "z", **_NONE),
    "bt_wide": _case(WIDE, 0, "z", **_BT),
    "brent_wide": _case(WIDE, 0, "z", **_B1),
    # (TALL: the fixed step is the case compared by its codes; one Brent iteration spreads them by 2.6e-3 to 4.4e-3 on
    # seeds 0-4 -- the reference's float32 fold of 1400 losses is the noise Brent fits its parabola to)
    "none_tall": _case(TALL, 0, "z", **_NONE),
    "bt_tall": _case(TALL, 0, "f", **_BT),
    "brent_tall": _case(TALL, 0, "f", **_B1),
    "none_ragged": _case(RAGGED, 0, "f", **_NONE),
    "bt_ragged": _case(RAGGED, 0, "f", **_BT),
    "brent_ragged": _case(RAGGED, 0, "z", **_B1),
    # several Brent iterations: by objective, and where even that spreads, by properties.  SMALL: spread_f is 1.4e-4 to
    # 3.8e-3 on seeds 0-4 and 2.8e-4 to 2.5e-3 with 10 to 20 iterations; MID: 1.1e-4 to 5.2e-4 with 8 to 12 iterations on
    # seeds 0-4, 7.2e-5 with 16
    "brent8_small": _case(SMALL, 0, "props", **_B8),
    "brent16_mid": _case(MID, 0, "f", line_search="brent", history_size=3, max_iter=16),
    "brent8_tall": _case(TALL, 0, "f", **_B8),
    "brent8_ragged": _case(RAGGED, 0, "props", **_B8),
    "brent8_wide": _case(WIDE, 0, "props", **_B8),
    # no iteration; an xtol that stops before max_iter (at the first, shortest step: no update follows); a warm start; a
    # backtracking that runs out (the warning); every pair dropped (y.s ~ 1e-12); soft targets
    "iter0": _case(SMALL, 0, "z", line_search="backtrack", max_iter=0),
    "bt_xtol": _case(SMALL, 0, "z", line_search="backtrack", history_size=2, max_iter=8, xtol=0.15),
    "bt_warm": _case(MID, 1, "z", start="warm", line_search="backtrack", history_size=2, max_iter=4),
    "bt_runout": _case(MID, 0, "z", line_search="backtrack", ls_options=dict(tol=.9, decay=.9, maxiter=2), history_size=2,
                       max_iter=3),
    "all_dropped": _case(SMALL, 0, "z", line_search="none", lr=1e-7, xtol=0.0, history_size=2, max_iter=6),
    "bt_soft": _case(MID, 0, "z", targets="soft", line_search="backtrack", history_size=3, max_iter=6),
    # a start with logits of +-120: log(1 + exp(u)) written naively is inf there.  One iteration each: the codes spread by
    # 1e-9, while four backtracking iterations from there spread the objective by 1.2e-4 to 1e-3 on seeds 0-7
    "sat_none": _case(MID, 1, "z", start="saturated", line_search="none", lr=0.05, max_iter=1),
    "sat_bt": _case(MID, 1, "z", start="saturated", line_search="backtrack", max_iter=1),
}


def recipe(n, d, k, seed, targets="hard"):
    """x [n,d] in {0, 1} (soft: in (0, 1)), W [d,k] (unit-norm atoms)"""
    g = torch.Generator().manual_seed(seed)
    w = F.normalize(torch.randn(d, k, generator=g), dim=0)
    code = torch.randn(n, k, generator=g) * (torch.rand(n, k, generator=g) < 0.1)
    p = torch.sigmoid(3.0 * code @ w.T)
    x = p if targets == "soft" else torch.bernoulli(p, generator=g)
    return x, w


def warm_start(n, k, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return 0.3 * torch.randn(n, k, generator=g) * (torch.rand(n, k, generator=g) < 0.25)


def case_inputs(spec):
    """x [n,d], W [d,k], z0 [n,k]"""
    x, w = recipe(spec["n"], spec["d"], spec["k"], spec["seed"], spec["targets"])
    z0 = torch.zeros(spec["n"], spec["k"])
    if spec["start"] != "zero":
        z0 = warm_start(spec["n"], spec["k"], spec["seed"])
    if spec["start"] == "saturated":
        z0 = z0 * (SATURATION / float((z0 @ w.T).abs().max()))
    return x, w, z0
