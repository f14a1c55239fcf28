"""The conjugate-gradient golden cases (tests/golden/conjgrad_cases.npz): shapes, seeds and arguments, shared by the
generator (tests/golden/generate_golden_conjgrad.py) and the tests.  The generator certified every case: every recorded
sum|r| of the reference's runs is at least 1 % away from termcond and every sqrt(sum rs) at least 1 % away from tol;
the float32 and float64 runs end with the same status at the same iteration; it measured how far "another correct
implementation" (tests/conjgrad_model.py: permuted summation orders of the dots, the batch sums and the products'
contractions; sums folded in double and rounded once) moves x
(spread_x) and the three recorded sequences (spread_seq, relative), and admitted a case only with spread_x <= 2.5e-3.

Systems are well conditioned so that the reference alone stays inside those conditions.  Dense: A = W^T W + c I with W
from tests/recipes.py and d chosen per shape so that the condition number stays below about 100.  Convolutional:
kernels scaled by 1 / sqrt(C kh kw), b = conv2d(x, kernel): the right-hand side of the ridge code."""
import torch
import torch.nn.functional as F

from recipes import recipe_xw

SPREAD_X_CAP = 2.5e-3          # the cap tests/own_cases.py admits a case for comparison by its codes under
ORDER_SEEDS = tuple(range(1, 4))

# n, k, d (of W), seed
_SHAPES = {
    "n8_k10": (8, 10, 16, 0),
    "n37_k70": (37, 70, 19, 1),               # no tile multiple
    "n64_k64": (64, 64, 32, 2),
    "n130_k129": (130, 129, 40, 3),           # more than one row block and column block
    "n40_k257": (40, 257, 64, 4),
    "n16_k1030": (16, 1030, 128, 5),          # across 1024
    "n3_k1": (3, 1, 4, 6),
    "n1_k70": (1, 70, 19, 7),                 # also through cg with a 1-D b
}

DENSE = {}
for _name, (_n, _k, _d, _seed) in _SHAPES.items():
    # k = 1 solves exactly in one step: the residual behind it is rounding alone, below tol = 1e-10 in double and above
    # it in float32 -- tol = 0 takes the dtype out of which exit ends the run
    _kw = dict(tol=0.0) if _k == 1 else dict()
    DENSE[_name + "_rtol1"] = dict(n=_n, k=_k, d=_d, seed=_seed, kwargs=dict(_kw))
    DENSE[_name + "_rtol1em4"] = dict(n=_n, k=_k, d=_d, seed=_seed, kwargs=dict(_kw, rtol=1e-4))
_B = dict(n=37, k=70, d=19, seed=1)
DENSE["maxiter_2"] = dict(_B, kwargs=dict(maxiter=2, rtol=1e-4))                 # status 4
DENSE["abs_tol"] = dict(_B, kwargs=dict(rtol=0.0, tol=1e-2))                     # status 0
DENSE["nonsymmetric"] = dict(_B, skew=0.05, kwargs=dict(rtol=1e-2))               # positive definite, not symmetric
DENSE["cg_vector"] = dict(n=1, k=70, d=19, seed=7, vector=True, kwargs=dict(rtol=1e-4))
# float64 only: the double-precision tolerance can fire there alone
DENSE["f64_defaults"] = dict(_B, f64_only=True, kwargs=dict())
# (curv_sum ~ |A| rs^2 falls below 3 eps before rs falls below 1e-10 unless the last step is a jump: W of rank 6 gives A
# seven distinct eigenvalues, and conjugate gradients end in seven steps)
DENSE["f64_abs_tol"] = dict(_B, d=6, f64_only=True, kwargs=dict(rtol=0.0, tol=1e-10))  # status 0

_GEOMS = {
    "grey": dict(N=3, C=1, K=8, ks=(5, 5), H=12, W=12, stride=1, padding=0, seed=10),
    "rgb": dict(N=2, C=3, K=6, ks=(3, 3), H=9, W=9, stride=1, padding=1, seed=11),      # K no multiple of 4
    "stride2": dict(N=2, C=2, K=5, ks=(4, 4), H=12, W=12, stride=2, padding=1, seed=12),
    "pad_pair": dict(N=2, C=3, K=2, ks=(3, 3), H=7, W=8, stride=1, padding=(1, 0), seed=13),
}
CONV = {}
for _name, _g in _GEOMS.items():
    CONV[_name + "_tik0"] = dict(_g, tik=0, kwargs=dict(rtol=1e-2))
    CONV[_name + "_tik0p5"] = dict(_g, tik=0.5, kwargs=dict(rtol=1e-2))

VERBOSE_CASE = "n37_k70_rtol1em4"    # the case whose verbose=2 text the fixture holds


def dense_inputs(spec, dtype=torch.float32):
    """A [k,k], b [n,k] (or [k] for a vector case)"""
    _, W = recipe_xw(1, spec["d"], spec["k"], seed=spec["seed"])
    W = W.double()
    A = W.T @ W + 0.5 * torch.eye(spec["k"], dtype=torch.float64)
    g = torch.Generator().manual_seed(1000 + spec["seed"])
    if "skew" in spec:
        S = torch.randn(spec["k"], spec["k"], generator=g, dtype=torch.float64)
        A = A + spec["skew"] * (S - S.T) / spec["k"] ** 0.5
    b = torch.randn(spec["n"], spec["k"], generator=g, dtype=torch.float64)
    if spec.get("vector"):
        b = b[0]
    return A.to(dtype).contiguous(), b.to(dtype).contiguous()


def conv_kwargs(spec):
    return dict(stride=spec["stride"], padding=spec["padding"])


def conv_inputs(spec, dtype=torch.float32):
    """kernel [K,C,kh,kw], b [N,K,Hz,Wz] = conv2d(x, kernel)"""
    g = torch.Generator().manual_seed(spec["seed"])
    kh, kw = spec["ks"]
    kernel = torch.randn(spec["K"], spec["C"], kh, kw, generator=g, dtype=torch.float64) / (spec["C"] * kh * kw) ** 0.5
    x = torch.randn(spec["N"], spec["C"], spec["H"], spec["W"], generator=g, dtype=torch.float64)
    b = F.conv2d(x, kernel, **conv_kwargs(spec))
    return kernel.to(dtype).contiguous(), b.to(dtype).contiguous()


def load_case(npz, name):
    pre = name + "/"
    return {key[len(pre):]: npz[key] for key in npz.files if key.startswith(pre)}


def bar_x(g, floor=5e-5):
    """the project's rule (bar_z of tests/split_bregman_cases.py); float64 cases: the double spread, floor 1e-12"""
    return max(floor, 4.0 * float(g["spread_x"]))


def rtol_seq(g):
    return max(1e-5, 4.0 * float(g["spread_seq"]))


def rel(a, b):
    import numpy as np
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return float("inf")
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0
