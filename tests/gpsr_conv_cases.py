"""The convolutional GPSR-Basic golden cases (tests/golden/gpsr_conv_cases.npz): shapes, seeds and arguments, shared
by the generator (tests/golden/generate_golden_gpsr_conv.py) and the tests.  Inputs: x ~ N(0,1), W ~ N(0,1) with every
filter normalised to unit norm, from one seeded torch.Generator (x first).  Every case has an explicit maxiter and
was certified by the generator: no sufficient-decrease test within 1e-4 |f| of flipping, no stop test within 1 % of
tol, and identical trial lists in float32 and float64."""
import warnings

import numpy as np
import torch
import torch.nn.functional as F

CASES = {
    # name: N, C, H, W, K, ks, stride, padding, seed, tau, kwargs
    "gray7": dict(shape=(6, 1, 20, 20), K=16, ks=7, stride=1, padding=0, seed=1, tau=0.3, kwargs=dict(maxiter=12),
                  keep_stdout=True),
    "rgb5": dict(shape=(4, 3, 18, 22), K=24, ks=5, stride=1, padding=2, seed=2, tau=0.4, kwargs=dict(maxiter=10)),
    "c16k3": dict(shape=(3, 16, 16, 16), K=40, ks=3, stride=1, padding=1, seed=3, tau=0.5, kwargs=dict(maxiter=10)),
    "stride2": dict(shape=(4, 2, 19, 23), K=12, ks=5, stride=2, padding=1, seed=4, tau=0.3, kwargs=dict(maxiter=10)),
    # mu and lambda_backtrack that make the line search reject: several trials per iteration
    "search": dict(shape=(4, 3, 16, 16), K=16, ks=5, stride=1, padding=0, seed=5, tau=0.4,
                   kwargs=dict(maxiter=8, mu=0.95, lambda_backtrack=0.6)),
    "cont": dict(shape=(4, 1, 16, 16), K=16, ks=5, stride=1, padding=0, seed=6, tau=0.3,
                 kwargs=dict(continuation=True, cont_steps=3, first_tau_factor=3.0, maxiter=7)),
    "debias": dict(shape=(4, 1, 16, 16), K=16, ks=5, stride=1, padding=0, seed=7, tau=0.8,
                   kwargs=dict(debias=True, maxiter=10, maxiter_debias=8)),
    "crit0": dict(shape=(4, 3, 16, 16), K=16, ks=3, stride=1, padding=1, seed=8, tau=0.4,
                  kwargs=dict(stop_criterion=0, tol=200, maxiter=25)),
    "crit1": dict(shape=(4, 3, 16, 16), K=16, ks=3, stride=1, padding=1, seed=9, tau=0.4,
                  kwargs=dict(stop_criterion=1, tol=6e-3, maxiter=25)),
    "crit2": dict(shape=(4, 3, 16, 16), K=16, ks=3, stride=1, padding=1, seed=10, tau=0.4,
                  kwargs=dict(stop_criterion=2, tol=5e-2, maxiter=25)),
    "crit4": dict(shape=(4, 3, 16, 16), K=16, ks=3, stride=1, padding=1, seed=11, tau=0.4,
                  kwargs=dict(stop_criterion=4, tol=745.0, miniter=2, maxiter=25)),
    # warm start z0 = conv2d(x, W)
    "warm": dict(shape=(4, 3, 16, 16), K=16, ks=3, stride=1, padding=1, seed=12, tau=0.5, warm=True,
                 kwargs=dict(maxiter=10)),
    "zero": dict(shape=(2, 1, 12, 12), K=8, ks=3, stride=1, padding=0, seed=13, tau=500.0, kwargs=dict(maxiter=5)),
}


def conv_inputs(shape, K, ks, seed, unit_norm=True):
    """(unit_norm=False: one-tap filters would all be +-1, a problem GPSR solves exactly in two steps)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    w = torch.randn(K, shape[1], ks, ks, generator=g)
    if unit_norm:
        w = w / w.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
    return x, w


def case_inputs(spec):
    """x [N,C,H,W], W [K,C,ks,ks] and the z0 of the case (None, or conv2d(x, W) for a warm start)"""
    x, w = conv_inputs(spec["shape"], spec["K"], spec["ks"], spec["seed"])
    z0 = F.conv2d(x, w, stride=spec["stride"], padding=spec["padding"]) if spec.get("warm") else None
    return x, w, z0


def load_case(npz, name):
    pre = name + "/"
    return {key[len(pre):]: npz[key] for key in npz.files if key.startswith(pre)}


def rows_of(z):
    """the code as rows [N*K][Hz*Wz]: what the fixture samples"""
    return z.reshape(z.shape[0] * z.shape[1], -1)


def z_bar(x, w, tau, z0=None, stride=1, padding=0, **kwargs):
    """The project's GPSR rule for a HIP result: the model in float32 against the model in float64 measures how far
    rounding alone moves this solve; the kernels sum in another order, so they get 4 x that gap -- never tighter than
    the project's floors: 5e-5 on z, 1e-5 relative on lambda, 1e-6 relative on the objective.
    Returns (bars, gaps, z32, info32): bars / gaps are dicts with keys z, lam, obj."""
    import gpsr_conv_model
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z32, i32 = gpsr_conv_model.gpsr_conv2d(x, w, tau, z0=z0, stride=stride, padding=padding, return_info=True, **kwargs)
        z64, i64 = gpsr_conv_model.gpsr_conv2d(x.double(), w.double(), tau, z0=None if z0 is None else z0.double(),
                                               stride=stride, padding=padding, return_info=True, **kwargs)
    same = i32["trials"] == i64["trials"]

    def rel(key):
        return max([abs(p - q) / abs(q) for p, q in zip(i32[key], i64[key])] or [0.0]) if same else float("inf")

    gaps = dict(z=float((z32.double() - z64).abs().max()) if z32.numel() else 0.0, lam=rel("accepted_lambda"),
                obj=rel("objective"))
    bars = dict(z=max(5e-5, 4.0 * gaps["z"]), lam=max(1e-5, 4.0 * gaps["lam"]), obj=max(1e-6, 4.0 * gaps["obj"]))
    return bars, gaps, z32, i32


def max_rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0
