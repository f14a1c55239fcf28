"""The orthant-wise Newton golden cases (tests/golden/own_cases.npz): shapes, seeds and arguments, shared by the
generator (tests/golden/generate_golden_own.py) and the tests.  Inputs come from tests/recipes.py, zero start unless
``warm``.  The generator certified every case: no backtracking decision within 1e-4 |f| of its bound, no |dz| within
1 % of xtol; it measured how far "another correct float32 implementation" (tests/own_model.py with order_seed) moves
the codes (spread_z) and the objective (spread_f), and admitted a case for code comparison only with
spread_z <= 2.5e-3 and for objective comparison only with spread_f <= 1e-4.

Several iterations of the Brent search are compared by objective only: the reference's own float32 and float64 runs
end 0.06-0.4 apart in the codes there (its float32-rounded objective sends Brent to another t), while their objectives
agree to 1e-5.  Every case but the ``wide_*`` pair has d > k; for k > d the Hessian is the 1e-4 shift on a
(k - d)-dimensional subspace and only properties and (where admitted) the objective are compared."""
import torch

from recipes import recipe_xw

SPREAD_Z_CAP = 2.5e-3
SPREAD_F_CAP = 1e-4
ORDER_SEEDS = tuple(range(1, 9))

CASES = {
    "bt_small": dict(n=33, d=40, k=24, seed=1, alpha=0.3, kwargs=dict(line_search="backtrack", maxiter=4), compare="z"),
    "bt_ragged": dict(n=37, d=260, k=200, seed=5, alpha=0.3, kwargs=dict(line_search="backtrack", maxiter=4), compare="z"),
    "bt_131": dict(n=131, d=140, k=100, seed=6, alpha=0.4, kwargs=dict(line_search="backtrack", maxiter=3), compare="z"),
    "none_half": dict(n=130, d=128, k=96, seed=0, alpha=0.4, kwargs=dict(line_search="none", lr=0.5, maxiter=4),
                      compare="z"),
    "bt_opts": dict(n=33, d=40, k=24, seed=0, alpha=0.3,
                    kwargs=dict(line_search="backtrack", ls_options=dict(tol=.3, decay=.5, maxiter=3), maxiter=3),
                    compare="z"),
    "brent_1a": dict(n=70, d=96, k=64, seed=0, alpha=0.3, kwargs=dict(line_search="brent", maxiter=1), compare="z"),
    "brent_1b": dict(n=64, d=256, k=192, seed=0, alpha=0.5, kwargs=dict(line_search="brent", maxiter=1), compare="z"),
    "brent_6a": dict(n=70, d=96, k=64, seed=0, alpha=0.3, kwargs=dict(line_search="brent", maxiter=6), compare="f"),
    "brent_6b": dict(n=37, d=260, k=200, seed=6, alpha=0.3, kwargs=dict(line_search="brent", maxiter=6), compare="f"),
    # d and k no multiples of 4: the scalar-load operand form
    "bt_odd": dict(n=35, d=45, k=27, seed=0, alpha=0.3, kwargs=dict(line_search="backtrack", maxiter=3), compare="z"),
    # a warm start: z0 = a sparse random code
    "bt_warm": dict(n=33, d=40, k=24, seed=1, alpha=0.3, warm=True, kwargs=dict(line_search="backtrack", maxiter=3),
                    compare="z"),
    # an xtol large enough to stop before maxiter
    "bt_xtol": dict(n=33, d=40, k=24, seed=1, alpha=0.3, kwargs=dict(line_search="backtrack", maxiter=8, xtol=16.0),
                    compare="z"),
    # a backtracking that runs out: the warning, and the next rung taken unexamined
    "bt_runout": dict(n=33, d=40, k=24, seed=0, alpha=0.3,
                      kwargs=dict(line_search="backtrack", ls_options=dict(tol=.9, decay=.9, maxiter=2), maxiter=3),
                      compare="z"),
    # k > d: properties, and the objective where the generator admitted it
    "wide_brent": dict(n=48, d=64, k=128, seed=0, alpha=0.3, kwargs=dict(line_search="brent", maxiter=3), compare="wide"),
    "wide_bt": dict(n=48, d=64, k=128, seed=0, alpha=0.3, kwargs=dict(line_search="backtrack", maxiter=3), compare="wide"),
}


def case_inputs(spec):
    """x [n,d], W [d,k], z0 [n,k]"""
    x, w = recipe_xw(spec["n"], spec["d"], spec["k"], seed=spec["seed"])
    z0 = torch.zeros(spec["n"], spec["k"])
    if spec.get("warm"):
        g = torch.Generator().manual_seed(1000 + spec["seed"])
        z0 = torch.randn(spec["n"], spec["k"], generator=g) * (torch.rand(spec["n"], spec["k"], generator=g) < 0.25)
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
