"""The BFGS iterated-ridge golden cases (tests/golden/irbfgs_cases.npz): shapes, seeds and arguments, shared by the
generator (tests/golden/generate_golden_irbfgs.py) and the tests.  Inputs: unit-norm atoms, x = z* W^T + 0.01 noise with
a 10 %-sparse z*; the start is 0.3 randn with about 30 % exact zeros and an all-zero LAST row, so the mask is live from
iteration 1 and every update has an invalid row (s = y = 0 there).  The generator certified every case: no |y.s|
within a factor 10 of 1e-10 and no |dx| within 1 % of xtol, in the float32 and the float64 run; it measured how far
"another correct float32 implementation" (tests/irbfgs_model.py with order_seed) moves the codes (spread_z) and the
objective (spread_f), and admitted a case for code comparison only with spread_z <= 2.5e-3 and for objective
comparison only with spread_f <= 1e-4.

Fixed-step cases and one-iteration Brent cases are compared by their CODES; several Brent iterations by objective only
(the reference's own float32 and float64 runs end 5e-4 .. 4e-3 apart in the codes there while their objectives agree).
NONFINITE cases carry one NaN or Inf operand; only the class pattern of the reference's result is compared."""
import torch
import torch.nn.functional as F

SPREAD_Z_CAP = 2.5e-3
SPREAD_F_CAP = 1e-4
ORDER_SEEDS = tuple(range(1, 9))

# k at or below 32 (one wave per system), one past a 32-block, ragged k, above 256 (the general tier)
WAVE, LDS33, LDS70, GENERAL = (5, 8, 16), (4, 16, 33), (3, 20, 70), (2, 24, 288)
SHAPES = dict(wave=WAVE, lds33=LDS33, lds70=LDS70, general=GENERAL)


def _case(shape, seed, compare, alpha=0.1, start="sparse", **kwargs):
    n, d, k = shape
    return dict(n=n, d=d, k=k, seed=seed, alpha=alpha, start=start, kwargs=kwargs, compare=compare)


CASES = {}
for _name, _shape in SHAPES.items():
    CASES["fixed4_" + _name] = _case(_shape, 0, "z", line_search=False, lr=0.3, maxiter=4)
    CASES["fixed12_" + _name] = _case(_shape, 0, "z", line_search=False, lr=0.3, maxiter=12)
    CASES["brent1_" + _name] = _case(_shape, 0, "z", line_search=True, maxiter=1)
    CASES["brent4_" + _name] = _case(_shape, 0, "f", line_search=True, maxiter=4)
CASES.update({
    "brent8_wave": _case(WAVE, 0, "f", line_search=True, maxiter=8),
    "brent8_lds70": _case(LDS70, 0, "f", line_search=True, maxiter=8),
    # an all-zero start: every coordinate is frozen, the solve stops at iteration 1 with |dx| = 0
    "all_zero": _case(LDS33, 0, "z", start="zero", line_search=True, maxiter=5),
    # an xtol that stops before maxiter
    "xtol_early": _case(LDS70, 0, "f", line_search=True, xtol=0.4, maxiter=12),
    # a dense start: no frozen coordinate, no invalid row
    "dense_start": _case(LDS33, 1, "z", start="dense", line_search=False, lr=0.3, maxiter=4),
    "iter0": _case(WAVE, 0, "z", line_search=True, maxiter=0),
})

# (operand, row, column, value): one non-finite entry; line_search as the reference's default
NONFINITE = {
    "nan_z0": dict(case=_case(LDS33, 0, "class", line_search=True, maxiter=5), poison=("z0", 1, 2, float("nan"))),
    "nan_x": dict(case=_case(LDS33, 0, "class", line_search=True, maxiter=5), poison=("x", 1, 3, float("nan"))),
    "inf_z0": dict(case=_case(LDS33, 0, "class", line_search=True, maxiter=5), poison=("z0", 2, 1, float("inf"))),
    "inf_x": dict(case=_case(LDS33, 0, "class", line_search=True, maxiter=5), poison=("x", 2, 0, float("inf"))),
}


def recipe(n, d, k, seed):
    """x [n,d], W [d,k] (unit-norm atoms), from a 10 %-sparse code plus 0.01 noise"""
    g = torch.Generator().manual_seed(seed)
    w = F.normalize(torch.randn(d, k, generator=g), dim=0)
    code = torch.randn(n, k, generator=g) * (torch.rand(n, k, generator=g) < 0.1)
    x = code @ w.T + 0.01 * torch.randn(n, d, generator=g)
    return x, w


def case_inputs(spec):
    """x [n,d], W [d,k], z0 [n,k]"""
    n, k = spec["n"], spec["k"]
    x, w = recipe(n, spec["d"], k, spec["seed"])
    g = torch.Generator().manual_seed(1000 + spec["seed"])
    z0 = 0.3 * torch.randn(n, k, generator=g)
    keep = torch.rand(n, k, generator=g) >= 0.3
    if spec["start"] == "zero":
        z0 = torch.zeros(n, k)
    elif spec["start"] == "sparse":
        z0 = torch.where(keep, z0, torch.zeros(()))          # (+0: a product with the mask would leave -0)
        z0[n - 1] = 0
    return x, w, z0


def poisoned_inputs(entry):
    x, w, z0 = case_inputs(entry["case"])
    name, i, j, value = entry["poison"]
    {"x": x, "z0": z0}[name][i, j] = value
    return x, w, z0


def classes(z):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf, per entry"""
    z = torch.as_tensor(z)
    return torch.isnan(z).to(torch.int8) + 2 * (z == float("inf")).to(torch.int8) + 3 * (z == float("-inf")).to(torch.int8)


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
