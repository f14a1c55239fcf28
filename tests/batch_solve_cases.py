"""The batched-solve golden cases (tests/golden/batch_solve_cases.npz): shapes, seeds and recipes, shared by the
generator (tests/golden/generate_golden_batch_solve.py) and the tests.  TEST INFRASTRUCTURE, plain torch.

The fixture holds, per case and dtype, what the reference's ``batch_cholesky_solve`` (lasso/linear/utils.py:43-58)
returned on this recipe's float32 / float64 tensors (``x32`` / ``x64``), whether it warned (``warned``), the
``info`` of torch's ``cholesky_ex`` (``info32`` / ``info64``) and the measured ``spread32`` / ``spread64``: the largest
relative move of x, over the systems, under "another correct implementation" -- three seeded symmetric permutations
``P A P^T, P b`` solved with torch on the route the case takes and un-permuted; for float32 also the distance to the
float64 result.  A case is admitted only with spread <= SPREAD_CAP.  The inputs are NOT stored: they are these recipes.

Recipes (all built in double, then rounded to the dtype):
  spd        A_i = Q diag(lambda) Q^T, Q from the QR of a Gaussian matrix, lambda log-spaced from 1 down to 1 / cond
  iter-ridge the system iterative_ridge builds: G = W^T W with the rows and columns off a random support zeroed, plus
             diag(alpha / |z|) with |z| log-spaced over six decades on the support and `tikhonov` off it
  indef      spd (lambda from 10 down to 1), system 2 replaced by A_2 - 3 I: indefinite, not singular
  zerodiag   spd, system 1 replaced by [[0, C], [C^T, 0]] with C spd: symmetric, a zero diagonal -- LU has to exchange rows
  nonsym     indef, system 0 given a strict UPPER triangle that is not the mirror of its lower one: its Cholesky
             factorisation succeeds (the lower triangle alone is read), the LU route reads the whole matrix
"""
import math

import numpy as np
import torch

SPREAD_CAP = 2.5e-3            # the cap tests/conjgrad_cases.py admits a case under
FLOOR = {torch.float32: 5e-5, torch.float64: 1e-12}
PERM_SEEDS = (1, 2, 3)
DTYPES = {"32": torch.float32, "64": torch.float64}

# shapes the module's constants fix (lasso_amd.linear.utils.LDS_CAP / CAP); tests/test_batch_solve_cpu.py holds them equal
LDS_CAP = {"32": 256, "64": 160}
CAP = {"32": 1024, "64": 512}


def _spd(name, B, D, cond=10.0, seed=0, only=None):
    return name, dict(kind="spd", B=B, D=D, cond=cond, seed=seed, only=only)


CASES = dict([
    _spd("d1_b5", 5, 1, seed=1),
    _spd("d2_b5", 5, 2, seed=2),
    _spd("d31_b7", 7, 31, seed=3),                         # wave tier, B no multiple of four systems per workgroup
    _spd("d32_b5", 5, 32, cond=1e3, seed=4),               # the wave tier's last D
    _spd("d33_b5", 5, 33, seed=5),                         # the LDS tier's first
    _spd("d64_b1", 1, 64, cond=1e5, seed=6),
    _spd("d65_b5", 5, 65, cond=1e3, seed=7),
    _spd("d97_b5", 5, 97, seed=8),
    _spd("d255_b2", 2, 255, seed=9, only="32"),            # float32: LDS cap - 1, cap, cap + 1
    _spd("d256_b2", 2, 256, cond=1e3, seed=10, only="32"),
    _spd("d257_b5", 5, 257, seed=11, only="32"),           # (five systems: the batch that wraps is made of them)
    _spd("d159_b2", 2, 159, seed=12, only="64"),           # float64: the same around its cap
    _spd("d160_b2", 2, 160, cond=1e3, seed=13, only="64"),
    _spd("d161_b5", 5, 161, seed=14, only="64"),
    _spd("d300_b2", 2, 300, seed=15),
    _spd("d1024_b2", 2, 1024, seed=16, only="32"),         # the general caps
    _spd("d512_b2", 2, 512, seed=17, only="64"),
])
CASES["iter_ridge_d97_b5"] = dict(kind="iter-ridge", B=5, D=97, seed=20, only=None)
for _D in (33, 97, 257):
    CASES["indef_d%d_b5" % _D] = dict(kind="indef", B=5, D=_D, seed=30 + _D, only=None)
CASES["zerodiag_d34_b3"] = dict(kind="zerodiag", B=3, D=34, seed=40, only=None)
CASES["nonsym_d65_b3"] = dict(kind="nonsym", B=3, D=65, seed=41, only=None)

# non-finite inputs on the systems of a base case: (base, which operand, system, index, value)
NONFINITE = {
    "b_nan": ("d33_b5", "b", 1, (3,), float("nan")),
    "b_pinf": ("d33_b5", "b", 1, (3,), float("inf")),
    "b_ninf": ("d33_b5", "b", 1, (32,), float("-inf")),
    "b_nan_wave": ("d31_b7", "b", 4, (30,), float("nan")),
    "a_nan": ("d33_b5", "A", 1, (5, 2), float("nan")),            # in the lower triangle: the LU route
}


def dtypes_of(spec):
    return [k for k in DTYPES if spec["only"] in (None, k)]


def _orth(D, g):
    q, r = torch.linalg.qr(torch.randn(D, D, generator=g, dtype=torch.float64))
    return q * torch.sign(torch.diagonal(r))


def _spd_matrix(D, hi, lo, g):
    lam = torch.logspace(math.log10(hi), math.log10(lo), D, dtype=torch.float64) if D > 1 else torch.tensor([hi], dtype=torch.float64)
    q = _orth(D, g)
    a = (q * lam) @ q.T
    return 0.5 * (a + a.T)


def inputs(spec, dtype=torch.float64):
    """b [B,D], A [B,D,D] of a case, in `dtype` (built in double, rounded once)"""
    B, D, kind = spec["B"], spec["D"], spec["kind"]
    g = torch.Generator().manual_seed(1000 + spec["seed"])
    b = torch.randn(B, D, generator=g, dtype=torch.float64)
    if kind == "spd":
        A = torch.stack([_spd_matrix(D, 1.0, 1.0 / spec["cond"], g) for _ in range(B)])
    elif kind == "iter-ridge":
        mats, ons = [], []
        for _ in range(B):
            W = torch.nn.functional.normalize(torch.randn(48, D, generator=g, dtype=torch.float64), dim=0)
            on = torch.rand(D, generator=g) < 0.6
            G = W.T @ W
            G = G * on[:, None] * on[None, :]
            z = torch.logspace(-3, 3, D, dtype=torch.float64)[torch.randperm(D, generator=g)]
            diag = torch.where(on, 0.5 / z, torch.full_like(z, 1e-4))
            mats.append(G + torch.diag(diag))
            ons.append(on.double())
        A = torch.stack(mats)
        b = b * torch.stack(ons)                            # (the masked entries of the right-hand side are zero)
    else:
        A = torch.stack([_spd_matrix(D, 10.0, 1.0, g) for _ in range(B)])
        if kind in ("indef", "nonsym"):
            A[2] = A[2] - 3.0 * torch.eye(D, dtype=torch.float64)
        if kind == "zerodiag":
            h = D // 2
            C = _spd_matrix(h, 10.0, 1.0, g)
            Z = torch.zeros(D, D, dtype=torch.float64)
            Z[:h, h:] = C
            Z[h:, :h] = C.T
            A[1] = Z
        if kind == "nonsym":
            U = torch.triu(torch.randn(D, D, generator=g, dtype=torch.float64), diagonal=1)
            A[0] = torch.tril(A[0]) + 0.3 * U / math.sqrt(D)
    return b.to(dtype).contiguous(), A.to(dtype).contiguous()


def nonfinite_inputs(name, dtype):
    base, which, system, index, value = NONFINITE[name]
    b, A = inputs(CASES[base], dtype)
    (b if which == "b" else A)[(system,) + index] = value
    return b, A


def load_case(npz, name):
    pre = name + "/"
    return {key[len(pre):]: npz[key] for key in npz.files if key.startswith(pre)}


def bar(g, key):
    """the project's rule (bar_x of tests/conjgrad_cases.py): max(floor, 4 x spread), per system of max|x - x_ref| / max|x_ref|"""
    return max(FLOOR[DTYPES[key]], 4.0 * float(g["spread" + key]))


def rel_rows(x, ref):
    """per system: max|x - x_ref| / max|x_ref|"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape
    return np.abs(x - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-300)


def classes(x):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf"""
    x = np.asarray(x)
    return np.where(np.isnan(x), 1, np.where(np.isposinf(x), 2, np.where(np.isneginf(x), 3, 0)))
