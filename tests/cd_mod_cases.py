"""The coord_descent_mod golden cases (tests/golden/cd_mod_cases.npz): shapes, seeds and arguments, shared by the
generator (tests/golden/generate_golden_cd_mod.py) and the tests.  Inputs are re-created from the seeded recipe
below; the atoms' norms are drawn from 0.5 .. 1.5 (not unit) so that the division by ||w_i||^2 shows.

The n == d cases are the ones the reference itself can run (it allocates the code as [n_features, n_components]);
the generator requires the host model (tests/cd_mod_model.py) to equal the reference bit for bit there.  Every
case stores the model's float32 and float64 results and a per-row `certified` flag: same sweeps in both, converged
in both, and no evaluated gap within 5 % of tol * ||x_row||^2 in either -- and a `decisive` flag: certified, and the
check rule of :132 (max|change| / max|z| < tol) was never within 5e-3 of flipping at a sweep where that would have
changed the sweep count (tests/golden/generate_golden_cd_mod.py says why) -- rows on which rounding cannot flip a
decision."""
import torch

TOL = 1e-4
MAX_ITER = 1000

CASES = {
    "sq32": dict(n=32, d=32, k=80, alpha=0.3, seed=0),
    "sq48_zero_atom": dict(n=48, d=48, k=24, alpha=0.2, seed=0, zero_atoms=(3,)),
    "sq24_all_zero": dict(n=24, d=24, k=64, alpha=5.0, seed=0),
    "sq64": dict(n=64, d=64, k=160, alpha=0.8, seed=0),
    "one_row": dict(n=1, d=20, k=40, alpha=0.3, seed=0),
    "n300_a03": dict(n=300, d=20, k=40, alpha=0.3, seed=0),
    "n300_a08": dict(n=300, d=20, k=40, alpha=0.8, seed=0),
    # (seeds 0 and 1 were refused by the generator: fewer than 12 of 16 rows certified and decisive)
    "k257": dict(n=16, d=96, k=257, alpha=0.4, seed=2),          # one column past a 256 block
    # (seed 0 was refused: 4 of 8 rows decisive)
    "k1030": dict(n=8, d=200, k=1030, alpha=0.5, seed=1),        # past 1024: the 2048-column kernel
    "tiny": dict(n=40, d=7, k=5, alpha=0.1, seed=0),
    "d1": dict(n=12, d=1, k=9, alpha=0.1, seed=0),
    "k1": dict(n=12, d=6, k=1, alpha=0.1, seed=0),
}
REFERENCE_CASES = tuple(name for name, c in CASES.items() if c["n"] == c["d"])


def case_inputs(spec):
    """x [n,d] ~ N(0,1), W [d,k] with atom norms uniform in 0.5 .. 1.5 (the atoms in spec['zero_atoms'] zeroed)."""
    g = torch.Generator().manual_seed(spec["seed"])
    n, d, k = spec["n"], spec["d"], spec["k"]
    x = torch.randn(n, d, generator=g)
    w = torch.nn.functional.normalize(torch.randn(d, k, generator=g), dim=0)
    w = w * (0.5 + torch.rand(k, generator=g))
    for j in spec.get("zero_atoms", ()):
        w[:, j] = 0.0
    return x, w.contiguous()


def load_case(npz, name):
    pre = name + "/"
    return {key[len(pre):]: npz[key] for key in npz.files if key.startswith(pre)}


def tol_row(x, tol=TOL):
    """the threshold of :81 as the kernel forms it: float(tol) * float(sum of squares taken in double)"""
    return torch.tensor(tol, dtype=torch.float32) * x.double().pow(2).sum(1).float()


def gap_f64(z, x, w, alpha):
    """the reference's gap formula (:87-99) of a given code, everything in float64"""
    import cd_mod_model
    return cd_mod_model.duality_gap(z.double(), x.double(), w.double(), alpha)
