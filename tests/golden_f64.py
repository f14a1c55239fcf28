"""The cases of tests/golden/f64_cases.npz (float64 codes of the real reference, written by
tests/golden/generate_golden_f64.py): inputs are re-drawn from the seeded recipe, only results -- and the step size each
case ran with -- are stored."""
import torch

from recipes import recipe_xw

ITERATIONS = 25
CASES = {}
for _n, _d, _k in [(37, 10, 50), (33, 200, 513), (32, 256, 1024)]:
    for _fast in (True, False):
        CASES["%dx%dx%d_%s" % (_n, _d, _k, "fista" if _fast else "ista")] = dict(
            shape=(_n, _d, _k), alpha=0.3, fast=_fast, backtrack=False)
CASES["33x200x513_backtrack"] = dict(shape=(33, 200, 513), alpha=0.5, fast=True, backtrack=True)


def case_step(case):
    """the step a case runs with: 1 / lambda_max(W^T W) for the fixed-step cases (eigvalsh in float64), the line
    search's start otherwise"""
    if case["backtrack"]:
        return 1.0
    n, d, k = case["shape"]
    W = recipe_xw(n, d, k)[1].double()
    gram = W @ W.t() if d <= k else W.t() @ W
    return 1.0 / torch.linalg.eigvalsh(gram)[-1].item()


def case_inputs(case, lr=None):
    """-> X, W, z0 (float64, CPU) and the solver's keyword arguments"""
    n, d, k = case["shape"]
    X, W = recipe_xw(n, d, k)
    X, W = X.double(), W.double()
    kw = dict(fast=case["fast"], lr=case_step(case) if lr is None else lr, maxiter=ITERATIONS, tol=0.0,
              backtrack=case["backtrack"])
    return X, W, X.new_zeros(n, k), kw
