"""The GPSR-Basic golden cases (tests/golden/gpsr_cases.npz): shapes, seeds and arguments, shared by the
generator (tests/golden/generate_golden_gpsr.py) and the tests.  Inputs come from tests/recipes.py; every case
has an explicit maxiter (the reference is slow on a CPU) and was certified by the generator: no line-search
decision and no stop decision is close enough to its threshold for rounding to flip it, and the trace of accepted
steps is not more sensitive to rounding than a quarter of the bar it is compared at (GPSR's step is a ratio of two
batch-wide sums over a support that changes; over many iterations one element entering the support a step earlier
moves it by 1e-4)."""
import re
import warnings

import numpy as np
import torch

from recipes import recipe_xw

CASES = {
    # the default arguments (criterion 3, tol 1e-2, miniter 5, zero start), explicit maxiter
    "default": dict(n=64, d=32, k=128, seed=1, alpha=0.3, kwargs=dict(maxiter=12), keep_stdout=True),
    "crit0": dict(n=48, d=24, k=96, seed=2, alpha=0.4, kwargs=dict(stop_criterion=0, tol=200, maxiter=25)),
    "crit1": dict(n=48, d=24, k=96, seed=3, alpha=0.4, kwargs=dict(stop_criterion=1, tol=6e-3, maxiter=25)),
    "crit2": dict(n=48, d=24, k=96, seed=4, alpha=0.4, kwargs=dict(stop_criterion=2, tol=5e-2, maxiter=25)),
    "crit4": dict(n=48, d=24, k=96, seed=5, alpha=0.4, kwargs=dict(stop_criterion=4, tol=330.0, maxiter=25)),
    # warm start from init='transpose' (z0 = x W)
    "warm": dict(n=40, d=32, k=100, seed=6, alpha=0.5, init="transpose", kwargs=dict(maxiter=12)),
    "cont": dict(n=40, d=32, k=100, seed=7, alpha=0.3, kwargs=dict(continuation=True, cont_steps=3, first_tau_factor=3.0, maxiter=7)),
    "debias": dict(n=40, d=32, k=100, seed=8, alpha=0.5, kwargs=dict(debias=True, maxiter=10, maxiter_debias=8)),
    # mu and lambda_backtrack that make the line search reject: several trials per iteration
    "search": dict(n=40, d=32, k=100, seed=12, alpha=0.4, kwargs=dict(mu=0.95, lambda_backtrack=0.6, maxiter=8)),
    "tall": dict(n=40, d=96, k=48, seed=9, alpha=0.5, kwargs=dict(maxiter=5)),                 # d > k
    "ragged": dict(n=261, d=260, k=1030, seed=10, alpha=0.6, kwargs=dict(maxiter=6)),           # beyond 256 x 1024
    "zero": dict(n=16, d=16, k=40, seed=11, alpha=50.0, kwargs=dict(maxiter=5)),                # tau >= max|Ay|
}


def case_inputs(spec):
    """x [n,d], W [d,k] and the z0 that sparse_encode is given (None, or x W for init='transpose')."""
    x, w = recipe_xw(spec["n"], spec["d"], spec["k"], seed=spec["seed"])
    z0 = torch.matmul(x, w) if spec.get("init") == "transpose" else None
    return x, w, z0


def load_case(npz, name):
    pre = name + "/"
    return {key[len(pre):]: npz[key] for key in npz.files if key.startswith(pre)}


def check_against_golden(name, z, info, gold, z_bar, caught):
    """the assertions shared with the GPU tests: z on the CPU, info as return_info gives it"""
    n_main = int(gold["n_iter"])                              # the debias steps count on top, like the reference's counter
    assert info["iterations"] == n_main + int(gold["db_iters"]), name
    assert list(info["trials"]) == list(gold["trials"]), name
    np.testing.assert_allclose(info["accepted_lambda"], gold["lam"], rtol=1e-5, err_msg=name)
    np.testing.assert_allclose(info["objective"], gold["objective"], rtol=1e-6, err_msg=name)
    assert len(info["criterion"]) == n_main
    rows = gold["z_rows"]
    dz = float(np.abs(z.numpy()[rows] - gold["z"]).max()) if rows.size else 0.0
    assert dz <= z_bar, (name, dz, z_bar)
    assert abs(float(z.double().abs().sum()) - float(gold["z_abssum"])) <= z_bar * max(1, int(gold["z_nnz"])), name
    assert sorted(str(c.message) for c in caught) == sorted(m for m in str(gold["warnings"]).split("\n") if m), name
    return dz


def same_line(a, b):
    """equal up to the last printed digit of each number (a float32 sum may round the other way)"""
    num = r"[-+]?\d+\.\d+e[-+]\d+|[-+]?\d+\.\d+|[-+]?\d+"
    if re.sub(num, "#", a) != re.sub(num, "#", b):
        return False
    for u, v in zip(re.findall(num, a), re.findall(num, b)):
        if u != v and abs(float(u) - float(v)) > 2e-5 * abs(float(v)):
            return False
    return True


def z_bar(x, w, tau, x0=None, **kwargs):
    """The bar on max|dz| for a HIP result: the model in float32 against the model in float64 measures how far
    rounding alone moves this solve (GPSR's step is a ratio of two batch-wide sums); the kernels sum in another order
    in two products and four reductions per iteration, so they get 4 x that gap -- and never less than 5e-5, the
    project's fp32 bar.  Returns (bar, gap, z32, info32); info32['lambda_sensitivity'] is the largest relative
    difference between the two runs' accepted steps (inf when they take different numbers of iterations)."""
    import gpsr_model
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z32, info = gpsr_model.gpsr_basic(x, w, tau, x0=x0, return_info=True, **kwargs)
        z64, info64 = gpsr_model.gpsr_basic(x.double(), w.double(), tau, x0=None if x0 is None else x0.double(),
                                            return_info=True, **kwargs)
    gap = float((z32.double() - z64).abs().max()) if z32.numel() else 0.0
    a, b = info["accepted_lambda"], info64["accepted_lambda"]
    info["lambda_sensitivity"] = (max([abs(p - q) / abs(q) for p, q in zip(a, b)] or [0.0])
                                  if info["trials"] == info64["trials"] else float("inf"))
    return max(5e-5, 4.0 * gap), gap, z32, info
