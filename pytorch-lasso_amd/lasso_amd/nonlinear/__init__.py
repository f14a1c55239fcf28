"""``lasso.nonlinear`` on the HIP path: ``owlqn`` for the residual-sum-of-squares objective ``rss(x, weight)``."""
from .owlqn import owlqn, rss  # noqa: F401
