"""``lasso.nonlinear`` on the HIP path: ``owlqn`` and ``iterative_ridge_bfgs`` for the residual-sum-of-squares objective
``rss(x, weight)``, ``owlqn`` for the logistic objective ``bernoulli(x, weight)`` as well, and ``ista_nl`` for decoders
of one affine layer and a pointwise activation (``nn.Linear``, ``nn.Sequential(nn.Linear, activation)``, ``affine``)."""
from .owlqn import bernoulli, owlqn, rss  # noqa: F401
from .iterative_ridge_bfgs import iterative_ridge_bfgs  # noqa: F401
from .ista import affine, ista_nl  # noqa: F401
