"""The iterated-ridge golden cases (tests/golden/iter_ridge_cases.npz): shapes, seeds and arguments, shared by the
generator (tests/golden/generate_golden_iter_ridge.py) and the tests.  Inputs come from tests/recipes.py; the start is
the ridge code z0 = x W (W^T W + alpha I)^-1 unless ``warm`` (a sparse random code: exact zeros, ragged supports from
the first iteration).  The generator certified every case: no sum |update| within 1 % of the scaled tol in the float32
or the float64 run of the reference; it measured how far "another correct float32 implementation"
(tests/iter_ridge_model.py with order_seed) moves the codes (spread_z) and the objective (spread_f), and admitted a case
for code comparison only with spread_z <= 2.5e-3 and for objective comparison only with spread_f <= 1e-4.

Several iterations of the Brent search are compared by objective only: the reference's own float32 and float64 runs part
ways there (its float32-rounded objective sends Brent to another t), while their objectives agree."""
import torch

from recipes import recipe_xw

SPREAD_Z_CAP = 2.5e-3
SPREAD_F_CAP = 1e-4
ORDER_SEEDS = tuple(range(1, 9))
NO_LS = dict(line_search=False, maxiter=8)

CASES = {
    "small": dict(n=33, d=40, k=24, seed=0, alpha=2.0, kwargs=NO_LS, compare="z"),
    # d and k no multiples of 4: the scalar-load operand form
    "odd": dict(n=35, d=45, k=27, seed=0, alpha=2.0, kwargs=NO_LS, compare="z"),
    # k > d: G is singular, the systems live on alpha / |z| + tikhonov
    "wide": dict(n=48, d=64, k=128, seed=0, alpha=3.0, kwargs=NO_LS, compare="z"),
    # the general tier at s = 300, then the LDS tier as the support shrinks
    "k300": dict(n=24, d=330, k=300, seed=0, alpha=4.0, kwargs=NO_LS, compare="z"),
    "warm": dict(n=37, d=64, k=96, seed=0, alpha=2.0, warm=True, kwargs=NO_LS, compare="z"),
    # stops before maxiter, default tol
    "tolstop": dict(n=40, d=200, k=160, seed=0, alpha=4.0, kwargs=dict(line_search=False, maxiter=60), compare="z",
                    stops=True),
    "tolstop2": dict(n=33, d=40, k=24, seed=0, alpha=2.0, kwargs=dict(line_search=False, maxiter=30, tol=2e-3),
                     compare="z", stops=True),
    "brent_1a": dict(n=40, d=200, k=160, seed=0, alpha=4.0, kwargs=dict(maxiter=1), compare="z"),
    "brent_1b": dict(n=37, d=64, k=96, seed=0, alpha=2.0, kwargs=dict(maxiter=1), compare="z"),
    "brent_6a": dict(n=37, d=64, k=96, seed=0, alpha=2.0, warm=True, kwargs=dict(maxiter=6), compare="f"),
    "brent_6b": dict(n=48, d=64, k=128, seed=0, alpha=3.0, kwargs=dict(maxiter=6), compare="f"),
}


def ridge_start(x, w, alpha):
    """sparse_encode.initialize_code(x, W, alpha, 'ridge') of the reference: x W (W^T W + alpha I)^-1, in float64 here
    and rounded once (the start is an input of the case, not something under test)"""
    wd, xd = w.double(), x.double()
    m = wd.T @ wd
    m.diagonal().add_(alpha)
    return torch.linalg.solve(m, (xd @ wd).T).T.contiguous().to(w.dtype)


def case_inputs(spec):
    """x [n,d], W [d,k], z0 [n,k]"""
    x, w = recipe_xw(spec["n"], spec["d"], spec["k"], seed=spec["seed"])
    if spec.get("warm"):
        g = torch.Generator().manual_seed(1000 + spec["seed"])
        z0 = torch.randn(spec["n"], spec["k"], generator=g) * (torch.rand(spec["n"], spec["k"], generator=g) < 0.25)
    else:
        z0 = ridge_start(x, w, spec["alpha"])
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
