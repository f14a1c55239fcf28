"""NaN and Inf as operand VALUES inside valid buffers: the case table and the helpers that tests/test_nonfinite_cpu.py
(the oracle's behaviour, pinned) and tests/test_nonfinite_gpu.py (the HIP kernels against it) share.  No case passes a
bad pointer, shape or pitch."""
import torch

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
FINITE, IS_NAN, IS_PINF, IS_NINF = 0, 1, 2, 3

ALPHA = 0.3
ITERS = (1, 2, 6)                     # 2 is where Inf turns into NaN (Inf - Inf in the second gradient)

# (n, d, k) of the linear solvers, the smallest at which each kernel family is reached (tests/test_fista_gpu.py,
# test_splitk_gpu.py, test_random_shapes_gpu.py): 64-row tile, 32-row tiles with a ragged last one, the flagship
# 16-row tile (forced to 'tile' and 'splitk'), and d > 256 / k > 1024 for the general-GEMM path
LINEAR_FUSED = [(37, 10, 50), (130, 128, 512), (64, 256, 1024)]
LINEAR_GENERAL = [(40, 300, 70), (24, 96, 1300)]
LINEAR_BF16 = [(37, 10, 50), (130, 128, 512)]
LINEAR_F64 = [(37, 10, 50), (40, 300, 70)]
CD_SHAPES = [(5, 7, 64), (33, 200, 513)]
MSTEP_SHAPES = [(30, 7, 12), (300, 64, 96)]

# value poisons of x; "z0" and "w" carry NaN only
X_POISONS = [("nan", NAN), ("pinf", PINF), ("ninf", NINF)]

# convolutional cases: (N, C, K, ks, padding, stride, Hz, Wz); N = None: set from the device's CU count by the GPU test
# (the CPU test and the oracle use 3 images: images are independent)
CONV_CASES = {
    "fused": (None, 1, 100, 3, 1, 1, 9, 9),            # (a) a workgroup per image, N = CUs + 3
    "bands": (None, 2, 48, 3, 1, 1, 40, 24),           # (b) N = CUs // 4, images cut into bands of code rows
    "synth": (3, 8, 32, 3, 1, 1, 12, 12),              # (d) conv_synth.hip
    "synth_few": (3, 2, 24, 7, 3, 1, 12, 11),          # (e) conv_synth_few.hip
    "explicit": (3, 2, 12, 3, 1, 2, 6, 7),             # (f) stride 2
}
# the poisoned pixel (channel, row, column) of image 1; 'bands': pixel row 10, whose receptive field is code rows 9-11
CONV_PIXEL = {"fused": (0, 4, 4), "bands": (1, 10, 23), "synth": (7, 0, 11), "synth_few": (1, 11, 0),
              "explicit": (0, 5, 6)}
CONV_ITERS = (1, 2, 3)


def poison(t, where, value):
    """a copy of ``t`` with ``value`` at the index (or each of the list of indices) ``where``"""
    out = t.clone()
    for idx in (where if isinstance(where, list) else [where]):
        out[idx] = value
    return out


def classes(t):
    """elementwise {FINITE, IS_NAN, IS_PINF, IS_NINF} as an int8 tensor on the CPU"""
    t = t.detach().to("cpu")
    t = t.float() if t.dtype in (torch.bfloat16, torch.float16) else t
    c = torch.zeros(t.shape, dtype=torch.int8)
    c[torch.isnan(t)] = IS_NAN
    c[t == PINF] = IS_PINF
    c[t == NINF] = IS_NINF
    return c


def nonzero_column(row):
    """the last coordinate of a code row that is not zero (where softshrink's backward passes the cotangent on)"""
    return int(torch.nonzero(row.detach().cpu() != 0).flatten()[-1])


def row_positions(n, d):
    """(row, column) of the poisoned elements of an [n, d] operand: the first row of the first tile, a row in the
    second tile of the 16- and 32-row tilings (inside the only tile of the 64-row one), the last valid row of the
    ragged last tile with the last column (d - 1: past the last multiple of 16 where d % 16 != 0)"""
    rows = [(0, 0), (min(33, n // 2), d // 2), (n - 1, d - 1)]
    assert len({r for r, _ in rows}) == 3
    return rows


def linear_problem(n, d, k, seed=0, dtype=torch.float32):
    """unit-norm W, N(0,1) X, a small z0 and a step safely below 1/L -- the finite batch every case starts from"""
    g = torch.Generator().manual_seed(1000 * seed + n + d + k)
    W = torch.nn.functional.normalize(torch.randn(d, k, generator=g, dtype=torch.float64), dim=0)
    X = torch.randn(n, d, generator=g, dtype=torch.float64)
    z0 = 0.05 * torch.randn(n, k, generator=g, dtype=torch.float64)
    lr = 0.9 / torch.linalg.eigvalsh(W @ W.T if d <= k else W.T @ W)[-1].item()
    return X.to(dtype), W.to(dtype), z0.to(dtype), lr


def conv_problem(name, N=None, dtype=torch.float32):
    """(x, w, z0, lr, stride, padding) of CONV_CASES[name] with N images (3 where the table leaves it open)"""
    n_tab, C, K, ks, pd, st, Hz, Wz = CONV_CASES[name]
    N = N if N is not None else (n_tab if n_tab is not None else 3)
    g = torch.Generator().manual_seed(sum(ord(c) for c in name))
    w = torch.randn(K, C, ks, ks, generator=g, dtype=torch.float64) / ks
    x = torch.randn(N, C, (Hz - 1) * st - 2 * pd + ks, (Wz - 1) * st - 2 * pd + ks, generator=g, dtype=torch.float64)
    z0 = torch.zeros(N, K, Hz, Wz, dtype=torch.float64)
    lr = 0.3 / w.pow(2).sum().item()
    return x.to(dtype), w.to(dtype), z0.to(dtype), lr, st, pd


def conv_reach(name, iters, image_shape, code_shape):
    """The code positions [Hz, Wz] that the poisoned pixel reaches after ``iters`` iterations, from the geometry alone:
    a pixel reaches the codes whose receptive field holds it (every atom: the adjoint sums over channels), a code
    reaches the pixels it synthesises (every channel).  Counted with all-ones kernels on 0/1 masks."""
    _, C, K, ks, pd, st, Hz, Wz = CONV_CASES[name]
    F = torch.nn.functional
    ones = torch.ones(1, 1, ks, ks, dtype=torch.float64)
    px = torch.zeros(1, 1, *image_shape, dtype=torch.float64)
    _, r, c = CONV_PIXEL[name]
    px[0, 0, r, c] = 1.0
    code = torch.zeros(1, 1, *code_shape, dtype=torch.float64)
    for _ in range(iters):
        pix = ((F.conv_transpose2d(code, ones, stride=st, padding=pd) + px) > 0).double()
        code = ((F.conv2d(pix, ones, stride=st, padding=pd) + code) > 0).double()
    return code[0, 0] > 0
