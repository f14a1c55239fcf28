"""``lasso.nonlinear`` on the HIP path: ``owlqn`` and ``iterative_ridge_bfgs`` for the residual-sum-of-squares objective
``rss(x, weight)``."""
from .owlqn import owlqn, rss  # noqa: F401
from .iterative_ridge_bfgs import iterative_ridge_bfgs  # noqa: F401
