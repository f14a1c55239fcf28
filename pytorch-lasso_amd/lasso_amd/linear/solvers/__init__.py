"""Mirror of lasso/linear/solvers/__init__.py:1,5 -- the solvers on the HIP path:
'ista' (SURVEY.md section 8a), greedy coordinate descent 'cd' (8f row f2), GPSR-Basic 'gpsr', and the cyclic coordinate descent with a duality-gap
stop, `coord_descent_mod`, which the reference exports beside them without routing it through sparse_encode.
`orthant_wise_newton` is a function of its own as well (sparse_encode's algorithm='own' stays off the HIP path), and so
is `iterative_ridge` (algorithm='iter-ridge' stays off it too), and so is `split_bregman` (algorithm='split-bregman'
likewise), and so is `interior_point` (algorithm='interior-point' likewise): with it every solver the reference exports
has a HIP form."""
from .ista import ista  # noqa: F401
from .coordinate_descent import coord_descent, coord_descent_mod  # noqa: F401
from .gpsr import gpsr_basic  # noqa: F401
from .orthant_wise_newton import orthant_wise_newton  # noqa: F401
from .iterative_ridge import iterative_ridge  # noqa: F401
from .split_bregman import split_bregman  # noqa: F401
from .interior_point import interior_point  # noqa: F401
