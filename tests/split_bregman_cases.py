"""The Split Bregman golden cases (tests/golden/split_bregman_cases.npz): shapes, seeds and arguments, shared by the
generator (tests/golden/generate_golden_split_bregman.py) and the tests.  Inputs come from tests/recipes.py; x0 is None
unless ``x0_seed``.  The generator certified every case: every recorded update of the reference's float32 and float64
runs is at least 1 % away from tol; it measured how far "another correct float32 implementation"
(tests/split_bregman_model.py: row-major state, a double Hinv rounded once, permuted summation orders) moves x
(spread_z) and the relative update sequence (spread_update), and admitted a case only with spread_z <= 2.5e-3."""
import torch

from recipes import recipe_xw

SPREAD_Z_CAP = 2.5e-3          # the cap tests/own_cases.py admits a case for comparison by its codes under
SPREAD_F_CAP = 1e-4            # ... and by its objective
ORDER_SEEDS = tuple(range(1, 5))

_BASE = dict(n=37, d=19, k=70, seed=0, alpha=0.3)

CASES = {
    "n8_d6_k10": dict(n=8, d=6, k=10, seed=0, alpha=0.3, kwargs=dict()),
    "n37_d19_k70": dict(_BASE, kwargs=dict()),                                   # no tile multiple
    "n33_d20_k70_x0": dict(n=33, d=20, k=70, seed=1, alpha=0.3, x0_seed=7, kwargs=dict()),
    "n64_d64_k64": dict(n=64, d=64, k=64, seed=2, alpha=0.3, kwargs=dict()),
    "n40_d32_k257": dict(n=40, d=32, k=257, seed=3, alpha=0.3, kwargs=dict()),   # across 256
    "n16_d48_k1030": dict(n=16, d=48, k=1030, seed=4, alpha=0.3, kwargs=dict()),  # across 1024
    "n24_d300_k130": dict(n=24, d=300, k=130, seed=5, alpha=0.3, kwargs=dict()),  # d > k
    "n3_d4_k1": dict(n=3, d=4, k=1, seed=6, alpha=0.3, kwargs=dict()),
    "n1_d19_k70": dict(n=1, d=19, k=70, seed=7, alpha=0.3, kwargs=dict()),
    "lambd_0p1": dict(_BASE, kwargs=dict(lambd=0.1)),
    "lambd_10": dict(_BASE, kwargs=dict(lambd=10.0)),
    "tau_0p9_inner1": dict(_BASE, kwargs=dict(tau=0.9, niter_inner=1)),
    "tol_1em2": dict(_BASE, kwargs=dict(tol=1e-2, maxiter=200)),                 # stops before maxiter
    "maxiter_1": dict(_BASE, kwargs=dict(maxiter=1)),
}


def case_inputs(spec):
    """A [d,k], y [n,d], x0 [n,k] or None"""
    y, A = recipe_xw(spec["n"], spec["d"], spec["k"], seed=spec["seed"])
    x0 = None
    if "x0_seed" in spec:
        x0 = torch.randn(spec["n"], spec["k"], generator=torch.Generator().manual_seed(spec["x0_seed"]))
    return A, y, x0


def load_case(npz, name):
    pre = name + "/"
    return {key[len(pre):]: npz[key] for key in npz.files if key.startswith(pre)}


def bar_z(g):
    """the project's rule (tests/test_gpsr_gpu.py, tests/test_own_gpu.py)"""
    return max(5e-5, 4.0 * float(g["spread_z"]))


def rtol_update(g):
    return max(1e-5, 4.0 * float(g["spread_update"]))
