"""Staging of CPU-resident inputs through the HIP device (_native.pick_device): every public solver gives, from inputs on
the CPU, a result on the CPU that is bitwise the result of the same inputs on the device -- and that one stays on its
device.  Shapes n=5, d=8, k=12 (a 1x1x6x6 image with two 3x3 atoms for the convolution): a few milliseconds each."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, D, K = 5, 8, 12


def _linear(dtype):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, D, generator=g, dtype=torch.float64)
    w = torch.nn.functional.normalize(torch.randn(D, K, generator=g, dtype=torch.float64), dim=0)
    z0 = 0.1 * torch.randn(N, K, generator=g, dtype=torch.float64)
    return x.to(dtype), w.to(dtype), z0.to(dtype)


def _ista(dtype):
    def run(to):
        from lasso_amd.linear.solvers import ista
        x, w, z0 = (to(t) for t in _linear(dtype))
        return ista(x, z0, w, alpha=0.3, lr=0.1, maxiter=7, tol=0.0)
    return run


def _coord_descent(to):
    from lasso_amd.linear.solvers import coord_descent
    x, w, _ = (to(t) for t in _linear(torch.float32))
    return coord_descent(x, w, alpha=0.3, maxiter=20)


def _gpsr(to):
    from lasso_amd.linear.solvers import gpsr_basic
    x, w, _ = (to(t) for t in _linear(torch.float32))
    return gpsr_basic(x, w, 0.3, maxiter=10)


def _lasso_loss(to):
    from lasso_amd.linear import lasso_loss
    x, w, z = (to(t) for t in _linear(torch.float32))
    return lasso_loss(x, z, w, alpha=0.3)


def _lipschitz(to):
    from lasso_amd.linear.lipschitz import lipschitz_constant
    return torch.tensor(lipschitz_constant(to(_linear(torch.float32)[1])), dtype=torch.float64)   # (a python float)


def _ista_conv2d(to):
    from lasso_amd.conv2d import ista_conv2d
    g = torch.Generator().manual_seed(4)
    x = to(torch.randn(1, 1, 6, 6, generator=g))
    w = to(torch.randn(2, 1, 3, 3, generator=g) / 3)
    z0 = to(torch.zeros(1, 2, 4, 4))
    return ista_conv2d(x, z0, w, alpha=0.2, lr=0.05, maxiter=5, tol=0.0)


CASES = {"ista_f32": _ista(torch.float32), "ista_f64": _ista(torch.float64), "ista_bf16": _ista(torch.bfloat16),
         "coord_descent": _coord_descent, "gpsr_basic": _gpsr, "lasso_loss": _lasso_loss,
         "lipschitz_constant": _lipschitz, "ista_conv2d": _ista_conv2d}


@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_inputs_are_staged_and_come_back(name):
    dev = torch.device("cuda", torch.cuda.current_device())
    from_cpu = CASES[name](lambda t: t)
    from_dev = CASES[name](lambda t: t.to(dev))
    assert from_cpu.device.type == "cpu"
    if name != "lipschitz_constant":
        assert from_dev.device == dev
    assert from_cpu.dtype == from_dev.dtype and from_cpu.shape == from_dev.shape
    assert torch.isfinite(from_cpu.double()).all()
    assert torch.equal(from_cpu, from_dev.cpu())
    if name not in ("lasso_loss", "lipschitz_constant"):
        assert from_cpu.abs().max() > 0          # (a solve that did something)
