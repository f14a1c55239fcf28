"""Host model of OWL-QN on the logistic objective (TEST INFRASTRUCTURE): what lasso/nonlinear/owlqn.py computes for
fun(z) = F.binary_cross_entropy_with_logits(z @ W.T, x, reduction='sum').  The solver is tests/owlqn_model.py's ``owlqn``
itself -- the memory, the projection, the line searches, the stop -- run on another ``Model``: the objective and its
gradient are the only parts of the reference that depend on ``fun``.  It keeps the knobs of owlqn_model (dtype,
accurate_f, order_seed) and adds one:

  link64  the link is evaluated in float64 from the float32 logits and rounded once (loss and sigmoid per element), in
          place of torch's float32 operations: "another correct float32 implementation" whose exp / log1p differ from
          torch's by ulps, as a device's do

With float32, accurate_f=False, order_seed=None and link64=False the arithmetic is the reference's operation for
operation (autograd's gradient of binary_cross_entropy_with_logits is (sigmoid(u) - x) * 1, then one product with W);
tests/golden/generate_golden_owlqn_glm.py checks torch.equal against the real reference when it writes the fixture."""
import functools
import types

import torch
import torch.nn.functional as F

import owlqn_model
from owlqn_model import CURV_MIN, LS_DEFAULTS, assert_robust, pseudo_gradient  # noqa: F401


def losses(u, x):
    """per-element softplus(u) - x u in the stable form: max(u, 0) - x u + log1p(exp(-|u|))"""
    return u.clamp(min=0) - x * u + torch.log1p(torch.exp(-u.abs()))


class Model(owlqn_model.Model):
    def __init__(self, weight, x, alpha, dtype=torch.float32, accurate_f=False, order_seed=None, link64=False):
        super().__init__(weight, x, alpha, dtype, accurate_f, order_seed)
        self.link64 = link64 and dtype == torch.float32

    def objective(self, z):
        """-> (f, r) with r = d loss / d u = sigmoid(u) - x; f a 0-dim tensor of dtype, or a python float folded in double"""
        u = self.mm(z, self.w.T)
        if self.link64:
            per = losses(u.double(), self.x.double()).to(self.dtype)
            r = (torch.sigmoid(u.double()) - self.x.double()).to(self.dtype)
        else:
            per = None
            r = torch.sigmoid(u) - self.x
        if self.accurate_f:
            if per is None:
                per = losses(u, self.x)
            return float(per.double().sum()) + self.alpha * float(z.double().abs().sum()), r
        loss = per.sum() if per is not None else F.binary_cross_entropy_with_logits(u, self.x, reduction='sum')
        return loss + self.alpha * z.norm(p=1), r


def owlqn(weight, x, z0, alpha=1., link64=False, model=Model, **kwargs):
    """owlqn_model.owlqn with the logistic ``Model`` (or a subclass of it): the same function object's code, its global
    ``Model`` rebound"""
    scope = dict(owlqn_model.__dict__, Model=functools.partial(model, link64=link64))
    run = types.FunctionType(owlqn_model.owlqn.__code__, scope, "owlqn", owlqn_model.owlqn.__defaults__)
    return run(weight, x, z0, alpha=alpha, **kwargs)


def first_line_objective(weight, x, z0, alpha, dtype=torch.float64, accurate_f=True):
    """t -> f(project(z0 + t d, eta)) of the first iteration's line search (d = v: the memory is empty), in ``dtype``"""
    m = Model(weight, x, alpha, dtype, accurate_f, None)
    z = z0.detach().to(dtype)
    _, _, pg = m.evaluate(z)
    v = pg.neg()
    eta = torch.where(z == 0, v.sign(), z.sign())
    return lambda t: float(m.objective(m.step(z, float(t), v.clone(), eta))[0])


def objective64(weight, x, z, alpha):
    """the objective of a code, in double"""
    u = torch.mm(z.double(), weight.double().T)
    return float(losses(u, x.double()).sum()) + alpha * float(z.double().abs().sum())
