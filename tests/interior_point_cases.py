"""The interior-point golden cases (tests/golden/interior_point_cases.npz): shapes, seeds and arguments, shared by the
generator (tests/golden/generate_golden_interior_point.py) and the tests.  Inputs come from tests/recipes.py; the start
is the ridge code z0 = x W (W^T W + alpha I)^-1, in float64 and rounded once.  The generator certified every case: at
every iteration of the float32 and the float64 run of the reference either some ratio mean is above 1.01 tol or all
three are below 0.99 tol; it measured how far "another correct float32 implementation"
(tests/interior_point_model.py with order_seed) moves the codes (spread_z) and the objective (spread_f), and admitted a
case for code comparison only with spread_z <= 2.5e-3 and for objective comparison only with spread_f <= 1e-4.

Short runs are compared by their codes.  From iteration 6-12 on single codes of the reference's own float32 and float64
runs part by 1e-2 (the |s| < eps mask and the clamps), while the lasso objective of the codes agrees to 5e-6: the
maxiter=20 cases are compared by that objective only."""
import torch

from recipes import recipe_xw

SPREAD_Z_CAP = 2.5e-3
SPREAD_F_CAP = 1e-4
ORDER_SEEDS = tuple(range(1, 9))
SHORT = dict(maxiter=4, tol=0.0)

CASES = {
    "small": dict(n=33, d=40, k=24, seed=0, alpha=0.3, kwargs=SHORT, compare="z"),
    # d and k no multiples of 4: the scalar-load operand form
    "odd": dict(n=35, d=45, k=27, seed=0, alpha=0.3, kwargs=SHORT, compare="z"),
    "wide": dict(n=48, d=64, k=128, seed=0, alpha=0.5, kwargs=SHORT, compare="z"),
    # the largest system of the LDS tier: 36 blocks
    "d256": dict(n=24, d=256, k=300, seed=0, alpha=1.0, kwargs=SHORT, compare="z"),
    "k256": dict(n=16, d=64, k=256, seed=0, alpha=0.5, kwargs=SHORT, compare="z"),
    # d = 33: one row and column beyond a block
    "d33": dict(n=40, d=33, k=70, seed=0, alpha=0.2, kwargs=SHORT, compare="z"),
    # stop before maxiter with the default tol
    "stop_odd": dict(n=35, d=45, k=27, seed=0, alpha=0.3, kwargs=dict(), compare="z", stops=True),
    "stop_d256": dict(n=24, d=256, k=300, seed=0, alpha=1.0, kwargs=dict(), compare="z", stops=True),
    # the whole default length: objective only
    "long_k256": dict(n=16, d=64, k=256, seed=0, alpha=0.5, kwargs=dict(maxiter=20, tol=1e-3), compare="f"),
    "long_d33": dict(n=40, d=33, k=70, seed=0, alpha=0.2, kwargs=dict(maxiter=20, tol=1e-3), compare="f"),
}
RECORDS = ("obj", "prim", "dual", "gap")


def ridge_start(x, w, alpha):
    """the reference's ridge(x.T, W, alpha).T = x W (W^T W + alpha I)^-1, in float64 here and rounded once (the start is
    an input of the case, not something under test)"""
    wd, xd = w.double(), x.double()
    m = wd.T @ wd
    m.diagonal().add_(alpha)
    return torch.linalg.solve(m, (xd @ wd).T).T.contiguous().to(w.dtype)


def case_inputs(spec):
    """x [n,d], W [d,k], z0 [n,k]"""
    x, w = recipe_xw(spec["n"], spec["d"], spec["k"], seed=spec["seed"])
    return x, w, ridge_start(x, w, spec["alpha"])


def load_case(npz, name):
    pre = name + "/"
    return {key[len(pre):]: npz[key] for key in npz.files if key.startswith(pre)}


def lasso_objective(z, x, w, alpha):
    """0.5 |z W^T - x|^2 + alpha |z|_1 in double"""
    zd = z.double()
    return float(0.5 * (zd @ w.double().T - x.double()).pow(2).sum() + alpha * zd.abs().sum())


def admitted_z(g):
    return float(g["spread_z"]) <= SPREAD_Z_CAP


def admitted_f(g):
    return float(g["spread_f"]) <= SPREAD_F_CAP


def rtol_of(g, key, floor=1e-5):
    """the bar on a per-iteration record: 4 x its stored spread, never below the floor"""
    return max(floor, 4.0 * float(g["spread_" + key]))
