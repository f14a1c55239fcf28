"""The OWL-QN golden cases (tests/golden/owlqn_cases.npz): shapes, seeds and arguments, shared by the generator
(tests/golden/generate_golden_owlqn.py) and the tests.  Inputs: unit-norm atoms, x = z* W^T + 0.01 noise with a
10 %-sparse z*, a zero start unless the case says otherwise.  The generator certified every case: no backtracking
decision within 1e-4 |f| of its bound, no y.s within a factor 10 of 1e-10, no |dx| within 1 % of xtol; it measured how
far "another correct float32 implementation" (tests/owlqn_model.py with order_seed: permuted summation orders and the
vector-free direction, either objective fold) moves the codes (spread_z) and the objective (spread_f), and admitted a
case for code comparison only with spread_z <= 2.5e-3 and for objective comparison only with spread_f <= 1e-4.

Every 'none' and 'backtrack' case of at most 6 iterations and every one-iteration 'brent' case is compared by its
CODES.  Several Brent iterations, and a dozen backtracking ones, are compared by objective only: the reference's own
float32 and float64 runs end 0.05-0.16 apart in the codes there while their objectives agree.  ``props`` cases are
not admitted for either comparison: the objective falls from iteration to iteration, the reported objective is the
objective of the returned codes, and their signs are the orthant's."""
import torch
import torch.nn.functional as F

SPREAD_Z_CAP = 2.5e-3
SPREAD_F_CAP = 1e-4
ORDER_SEEDS = tuple(range(1, 9))

SMALL, MID, TALL, RAGGED, WIDE = (5, 7, 19), (24, 16, 40), (70, 20, 33), (33, 48, 130), (3, 8, 4100)


def _case(shape, seed, compare, alpha=0.1, start="zero", **kwargs):
    n, d, k = shape
    return dict(n=n, d=d, k=k, seed=seed, alpha=alpha, start=start, kwargs=kwargs, compare=compare)


CASES = {
    # n k below one segment of the direction's passes, nothing a multiple of 4
    "none_small": _case(SMALL, 0, "z", line_search="none", lr=0.05, history_size=2, max_iter=6),
    "bt_small": _case(SMALL, 0, "z", line_search="backtrack", history_size=2, max_iter=6),
    "brent_small": _case(SMALL, 0, "z", line_search="brent", max_iter=1),
    # several segments and a ragged last one; the history overflows
    "none_ragged": _case(RAGGED, 0, "z", line_search="none", lr=0.05, history_size=2, max_iter=6),
    "bt_ragged": _case(RAGGED, 9, "z", line_search="backtrack", history_size=3, max_iter=6),
    # ... and backtrackings of 4 and 6 trials
    "bt_ladder": _case(RAGGED, 0, "z", alpha=0.3, line_search="backtrack", history_size=3, max_iter=6),
    "brent_ragged": _case(RAGGED, 0, "z", line_search="brent", max_iter=1),
    "none_tall8": _case(TALL, 0, "f", line_search="none", lr=0.05, history_size=3, max_iter=8),
    "bt_hist1": _case(MID, 0, "z", line_search="backtrack", history_size=1, max_iter=6),
    # the default memory (100) over 5 iterations: four pairs are reserved and held
    "bt_default": _case(TALL, 0, "z", line_search="backtrack", max_iter=5),
    # k > 4096: beyond orthant_wise_newton's cap
    "none_wide": _case(WIDE, 0, "z", line_search="none", lr=0.05, history_size=2, max_iter=4),
    "bt_wide": _case(WIDE, 0, "z", line_search="backtrack", history_size=2, max_iter=4),
    # no iteration, and one
    "iter0": _case(SMALL, 0, "z", line_search="backtrack", max_iter=0),
    "bt_iter1": _case(MID, 0, "z", line_search="backtrack", max_iter=1),
    # a start at the optimum (alpha above |x W|_inf: pg = 0): lr / 0 takes the clamp, the solve stops at iteration 1
    "at_optimum": _case(MID, 0, "z", alpha=50.0, line_search="none", lr=0.05, max_iter=5),
    # every pair dropped (y.s ~ 1e-12), a first pair dropped and later ones kept
    "all_dropped": _case(SMALL, 0, "z", line_search="none", lr=1e-7, xtol=0.0, history_size=2, max_iter=6),
    "first_dropped": _case(RAGGED, 0, "z", line_search="none", lr=5e-5, xtol=0.0, history_size=2, max_iter=6),
    # backtracking options, a backtracking that runs out (the warning), an xtol that stops before max_iter, a warm start
    "bt_opts": _case(MID, 0, "z", line_search="backtrack", ls_options=dict(tol=.3, decay=.5, maxiter=3), history_size=2,
                     max_iter=4),
    "bt_runout": _case(MID, 0, "z", line_search="backtrack", ls_options=dict(tol=.9, decay=.9, maxiter=2), history_size=2,
                       max_iter=3),
    "bt_xtol": _case(SMALL, 0, "z", line_search="backtrack", history_size=2, max_iter=8, xtol=0.15),
    "bt_warm": _case(MID, 1, "z", start="warm", line_search="backtrack", history_size=2, max_iter=4),
    # objective only
    "brent_8": _case(SMALL, 0, "f", line_search="brent", history_size=3, max_iter=8),
    "brent_12": _case(SMALL, 0, "f", line_search="brent", history_size=3, max_iter=12),
    # properties, and the objective where the generator admitted it ("another correct implementation" ends 5e-4 away)
    "brent_ragged_8": _case(RAGGED, 0, "props", line_search="brent", history_size=3, max_iter=8),
    "bt_12": _case(RAGGED, 0, "f", line_search="backtrack", history_size=2, max_iter=12),
}


def recipe(n, d, k, seed):
    """x [n,d], W [d,k] (unit-norm atoms), from a 10 %-sparse code plus 0.01 noise"""
    g = torch.Generator().manual_seed(seed)
    w = F.normalize(torch.randn(d, k, generator=g), dim=0)
    code = torch.randn(n, k, generator=g) * (torch.rand(n, k, generator=g) < 0.1)
    x = code @ w.T + 0.01 * torch.randn(n, d, generator=g)
    return x, w


def case_inputs(spec):
    """x [n,d], W [d,k], z0 [n,k]"""
    x, w = recipe(spec["n"], spec["d"], spec["k"], spec["seed"])
    z0 = torch.zeros(spec["n"], spec["k"])
    if spec["start"] == "warm":
        g = torch.Generator().manual_seed(1000 + spec["seed"])
        z0 = 0.3 * torch.randn(spec["n"], spec["k"], generator=g) * (torch.rand(spec["n"], spec["k"], generator=g) < 0.25)
    return x, w, z0


def load_case(npz, name):
    pre = name + "/"
    return {key[len(pre):]: npz[key] for key in npz.files if key.startswith(pre)}


def admitted_z(g):
    return float(g["spread_z"]) <= SPREAD_Z_CAP


def admitted_f(g):
    return float(g["spread_f"]) <= SPREAD_F_CAP


def rtol_of(g, key, floor=1e-5):
    """the bar on a per-iteration record: 4 x its stored spread, never below the floor"""
    return max(floor, 4.0 * float(g["spread_" + key]))
