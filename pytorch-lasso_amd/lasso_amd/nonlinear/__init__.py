"""``lasso.nonlinear`` on the HIP path: ``owlqn`` and ``iterative_ridge_bfgs`` for the residual-sum-of-squares objective
``rss(x, weight)``, and ``owlqn`` for the logistic objective ``bernoulli(x, weight)`` as well."""
from .owlqn import bernoulli, owlqn, rss  # noqa: F401
from .iterative_ridge_bfgs import iterative_ridge_bfgs  # noqa: F401
