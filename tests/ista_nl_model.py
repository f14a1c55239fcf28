"""Host model of ``ista_nl`` for decoders ``act(z W^T + b)``: the closed form of everything the reference
(lasso/nonlinear/ista.py:55-128) takes from autograd, in torch on the CPU, float32 or float64.

With u = y W^T + b and a = act(u):
  gradient of the rss term   g = ((a - x) act'(u)) W
  its Hessian, row i         H_i = W^T diag(c_i) W,  c = act'(u)^2 + (a - x) act''(u)
and ``hessian_2norm`` (ista.py:26-52) is 2 power_iters + 1 products H v with F.normalize between them.

With order_seed=None and link64=False the arithmetic follows the operations autograd performs for the reference
(sigmoid_backward is grad (1 - y) y, tanh_backward grad (1 - y^2), the products are the same mm calls), so for the
identity activation the float32 run is the reference's bit for bit.  Two options turn it into "another correct float32
implementation", as tests/owlqn_glm_model.py does:
  order_seed  every contraction, row sum and the stop rule's sum run over a seeded permutation of their index, and the
              normalisation of the power iteration is applied as a per-row scale AFTER the next product (the product is
              linear in the vector), which is what the HIP path does
  link64      a, act' and act'' -- and r, c from them -- are evaluated in float64 from the float32 logits and rounded
              once, standing in for a device whose expf differs from torch's by ulps
The start vector of the power iteration is ``power_init`` at EVERY step (the reference draws a new one per step; the
golden generator patches ``torch.randn_like`` to return it)."""
import math

import torch
import torch.nn.functional as F

ACTIVATIONS = ("identity", "sigmoid", "tanh", "relu")
NORM_EPS = 1e-8


def act_terms(activation, u):
    """a, act'(u), act''(u) in u's dtype, in the order autograd's backward formulas use"""
    if activation == "identity":
        return u, torch.ones_like(u), torch.zeros_like(u)
    if activation == "sigmoid":
        a = torch.sigmoid(u)
        d1 = (1 - a) * a
        return a, d1, d1 * (1 - 2 * a)
    if activation == "tanh":
        a = torch.tanh(u)
        d1 = 1 - a * a
        return a, d1, -2 * a * d1
    if activation == "relu":
        return torch.relu(u), (u > 0).to(u.dtype), torch.zeros_like(u)
    raise ValueError(activation)


def decode(activation, z, w, b):
    u = z @ w.T
    if b is not None:
        u = u + b
    return act_terms(activation, u)[0]


def lasso_loss(activation, x, z, w, b, alpha):
    return float(0.5 * (decode(activation, z, w, b) - x).pow(2).sum() + alpha * z.abs().sum())


class Model:
    def __init__(self, x, weight, bias, activation, dtype=torch.float32, order_seed=None, link64=False):
        assert activation in ACTIVATIONS
        self.dtype = dtype
        self.x, self.w = x.to(dtype), weight.to(dtype)
        self.b = bias.to(dtype) if bias is not None else None
        self.activation = activation
        self.link64 = link64 and dtype == torch.float32
        self.permuted = order_seed is not None
        n, d = x.shape
        k = weight.shape[1]
        if self.permuted:
            g = torch.Generator().manual_seed(order_seed)
            self.pk, self.pd = torch.randperm(k, generator=g), torch.randperm(d, generator=g)
            self.pnk = torch.randperm(n * k, generator=g)
        self.wt = self.w.T.contiguous()

    # ---- the two products and the sums, in the reference's order or a permuted one
    def times_wt(self, v):              # v W^T, contraction over k
        if self.permuted:
            return v[:, self.pk] @ self.w[:, self.pk].T
        return v @ self.w.T

    def times_w(self, r):               # r W, contraction over d
        if self.permuted:
            return r[:, self.pd] @ self.w[self.pd, :]
        return r @ self.w

    def row_sum(self, v):
        if self.permuted:
            return v[:, self.pk].sum(dim=1)
        return v.sum(dim=1)

    def total(self, v):
        if self.permuted:
            return v.reshape(-1)[self.pnk].sum()
        return v.sum()

    def link(self, y):
        """r = (a - x) act'(u), c = act'(u)^2 + (a - x) act''(u) at u = y W^T + b"""
        u = self.times_wt(y)
        if self.b is not None:
            u = u + self.b
        if self.link64:
            a, d1, d2 = act_terms(self.activation, u.double())
            diff = a - self.x.double()
            return (diff * d1).float(), (d1 * d1 + diff * d2).float()
        a, d1, d2 = act_terms(self.activation, u)
        diff = a - self.x
        if self.activation == "sigmoid":
            r = diff * (1 - a) * a      # sigmoid_backward
        else:
            r = diff * d1
        return r, d1 * d1 + diff * d2

    def hessian_2norm(self, c, u0, niter):
        if not self.permuted:
            hv = lambda v: self.times_w(self.times_wt(v) * c)
            u = F.normalize(u0, dim=1, eps=NORM_EPS)
            for _ in range(niter):
                v = F.normalize(hv(u), dim=1, eps=NORM_EPS)
                u = F.normalize(hv(v), dim=1, eps=NORM_EPS)
            return torch.sum(v * hv(u), dim=1)
        # the normalisation as a per-row scale after the next product
        scale = lambda a: 1 / self.row_sum(a * a).sqrt().clamp_min(NORM_EPS)
        hv = lambda a, s: self.times_w((self.times_wt(a) * s[:, None]) * c)
        a_prev, s_prev = None, None
        a, s = u0, scale(u0)
        for _ in range(2 * niter):
            a_prev, s_prev, a = a, s, hv(a, s)
            s = scale(a)
        return s_prev * self.row_sum(a_prev * hv(a, s))

    def step(self, y, alpha, lr, power_iters, power_init):
        r, c = self.link(y)
        grad = self.times_w(r)
        L = None
        if lr == "auto":
            L = self.hessian_2norm(c, power_init.to(self.dtype), power_iters)
            t = (0.98 / L).unsqueeze(-1)
        else:
            t = lr
        v = y - t * grad
        return v.sign() * F.relu(v.abs() - alpha * t), L


def ista_nl(x, z0, weight, bias=None, activation="identity", alpha=1.0, fast=True, maxiter=10, lr="auto", power_iters=10,
            tol=1e-5, power_init=None, dtype=torch.float32, order_seed=None, link64=False, losses=False):
    """-> (z, info): info = dict(iterations, deltas, stopped, L, losses) -- deltas the per-iteration sum |z - z_next| as
    the stop rule saw it, L the [n] estimates of the last step under 'auto', losses (if asked) the objective of z0, of
    every z that did not stop the solve, and of the result"""
    if not (lr == "auto" or isinstance(lr, float)):
        raise ValueError('expected `lr` to be either float or "auto".')
    m = Model(x, weight, bias, activation, dtype, order_seed, link64)
    budget = z0.numel() * tol
    z = z0.to(dtype)
    y, t = z, 1
    info = dict(iterations=0, deltas=[], stopped=False, L=None, losses=[])
    if losses:
        info["losses"].append(lasso_loss(activation, m.x, z, m.w, m.b, alpha))
    for _ in range(maxiter):
        z_next, L = m.step(y if fast else z, alpha, lr, power_iters, power_init)
        info["L"] = L
        delta = m.total((z - z_next).abs())
        info["deltas"].append(float(delta))
        info["iterations"] += 1
        if tol > 0 and delta <= budget:
            z = z_next
            info["stopped"] = True
            break
        if fast:
            t_next = (1 + math.sqrt(1 + 4 * t ** 2)) / 2
            y = z_next + ((t - 1) / t_next) * (z_next - z)
            t = t_next
        z = z_next
        if losses:
            info["losses"].append(lasso_loss(activation, m.x, z, m.w, m.b, alpha))
    if losses:
        info["losses"].append(lasso_loss(activation, m.x, z, m.w, m.b, alpha))
    return z, info


def row_hessians(x, weight, bias, activation, y):
    """the [n][k][k] Hessians W^T diag(c_i) W of the rss term at y, in float64"""
    m = Model(x, weight, bias, activation, torch.float64)
    _, c = m.link(y.double())
    return torch.einsum("dk,nd,dl->nkl", m.w, c, m.w)
