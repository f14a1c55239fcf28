"""The lip_constant golden cases (tests/golden/conv_lip_cases.npz): seeded kernels and geometries, shared by the
generator (tests/golden/generate_golden_conv_lip.py) and the tests.  Each is the smallest shape at which a path of
csrc/conv_lanczos.hip can go wrong; ``imsize`` is the IMAGE's size (what ``transpose=False`` takes), ``code_size`` below
gives what ``transpose=True`` takes for the same operator.

The generator ran the real reference (ARPACK) in float32 and float64 with ``transpose`` False and True on every finite
case and certified: the two float64 runs agree to 1e-10, and the model (tests/conv_lip_model.py) in float64 with
tol = 1e-10 is within 1e-9 of the reference's float64 value.  Per case it stored ref64, ref32 (both transposes),
gap32 = the reference's own float32-against-float64 gap, the model's spread in float32 and float64 (permuted summation
orders of the dots; float32 with the dots folded in double; another start vector) and lip_bound_conv2d where it exists."""
import math

import torch

ORDER_SEEDS = (1, 2, 3)

CASES = {
    # dim = 1: the value is w^2
    "one": dict(K=1, C=1, ks=(1, 1), imsize=(1, 1), stride=1, padding=0, seed=20),
    # dim = 64 and tol = 0: the basis reaches dim (exhaustion and breakdown)
    "exhaust": dict(K=6, C=1, ks=(5, 5), imsize=(8, 8), stride=1, padding=0, seed=21, tol=0.0),
    # non-square image, and strided
    "rect": dict(K=8, C=2, ks=(3, 3), imsize=(9, 7), stride=1, padding=1, seed=22),
    "rect_s2": dict(K=8, C=2, ks=(3, 3), imsize=(9, 7), stride=2, padding=1, seed=22),
    # fewer atoms than channels: the code space is the smaller one
    "few_atoms": dict(K=2, C=5, ks=(3, 3), imsize=(6, 6), stride=1, padding=1, seed=23),
    # a non-square kernel with a pair of paddings
    "k3x5": dict(K=4, C=2, ks=(3, 5), imsize=(8, 10), stride=1, padding=(1, 2), seed=24),
    # dim = 1440: more than one segment, the few-channel synthesis kernel's geometry; the lr='exact' case
    "rgb": dict(K=16, C=3, ks=(5, 5), imsize=(24, 20), stride=1, padding=2, seed=25),
    # dim = 4096, the C = 16 template
    "c16": dict(K=32, C=16, ks=(3, 3), imsize=(16, 16), stride=1, padding=1, seed=26),
    # A = I: beta_1 = 0 at the first step
    "delta": dict(K=1, C=1, ks=(3, 3), imsize=(6, 5), stride=1, padding=1, special="delta"),
    "zero": dict(K=3, C=2, ks=(3, 3), imsize=(6, 5), stride=1, padding=1, special="zero"),
    "nan": dict(K=3, C=2, ks=(3, 3), imsize=(6, 5), stride=1, padding=1, seed=27, special="nan"),
}
FINITE = [name for name, spec in CASES.items() if spec.get("special") in (None, "delta")]
PARITY = [name for name in FINITE if name != "delta"]       # cases compared with the reference's value
EXACT_LR_CASE = "rgb"


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def kernel_of(spec, dtype=torch.float32):
    """[K, C, kh, kw] with entries N(0, 1 / (C kh kw)), made in double and rounded once"""
    kh, kw = spec["ks"]
    shape = (spec["K"], spec["C"], kh, kw)
    special = spec.get("special")
    if special == "zero":
        return torch.zeros(shape, dtype=dtype)
    if special == "delta":
        w = torch.zeros(shape, dtype=dtype)
        w[0, 0, kh // 2, kw // 2] = 1.0
        return w
    g = torch.Generator().manual_seed(spec["seed"])
    w = torch.randn(shape, generator=g, dtype=torch.float64) / math.sqrt(spec["C"] * kh * kw)
    if special == "nan":
        w[1, 0, 1, 1] = float("nan")
    return w.to(dtype).contiguous()


def conv_kwargs(spec):
    return dict(stride=spec["stride"], padding=spec["padding"])


def code_size(spec):
    (kh, kw), (H, W) = spec["ks"], spec["imsize"]
    (sh, sw), (ph, pw) = _pair(spec["stride"]), _pair(spec["padding"])
    return ((H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1)


def imsize_of(spec, transpose):
    return code_size(spec) if transpose else tuple(spec["imsize"])


def dims(spec):
    """(dim of the image space, dim of the code space)"""
    (H, W), (Hz, Wz) = spec["imsize"], code_size(spec)
    return spec["C"] * H * W, spec["K"] * Hz * Wz


EXACT_LR_ALPHA, EXACT_LR_ITERS = 0.05, 20


def exact_lr_image(spec, dtype=torch.float32):
    """x [2, C, H, W] for the FISTA comparison of lr='exact' with lr='auto'"""
    g = torch.Generator().manual_seed(500 + spec["seed"])
    return torch.randn(2, spec["C"], *spec["imsize"], generator=g, dtype=torch.float64).to(dtype).contiguous()


def default_tol(dtype):
    return 1e-5 if dtype == torch.float32 else 1e-10


def tol_of(spec, dtype):
    return spec.get("tol", default_tol(dtype))


def load_case(npz, name):
    pre = name + "/"
    return {key[len(pre):]: npz[key] for key in npz.files if key.startswith(pre)}


def parity_bar(g, dtype, tol):
    """|L - ref64| / ref64 <= tol + 4 max(the reference's float32 gap, the model's spread); float64: the double spread"""
    if dtype == torch.float64:
        return tol + 4.0 * float(g["spread64"])
    return tol + 4.0 * max(float(g["gap32"]), float(g["spread32"]))
