"""Mirror of lasso/linear/sparse_encode.py:8-73 for the 'ista' arm."""
import torch

from .solvers import ista, coord_descent, gpsr_basic
from .utils import lstsq, ridge, _engine_for

_init_defaults = {'ista': 'zero'}                                   # sparse_encode.py:8-16

_OFF_PATH_ALGOS = ('iter-ridge', 'interior-point', 'split-bregman', 'own')


def _lstsq_init(x, weight):
    """init='lstsq' (sparse_encode.py:26-27): the reference's call, lstsq(x.T, weight).T"""
    return lstsq(x.T, weight).T


def _ridge_init(x, weight, alpha):
    """init='ridge' (sparse_encode.py:28-29): the reference's call, ridge(x.T, weight, alpha=alpha).T"""
    return ridge(x.T, weight, alpha=alpha).T


def initialize_code(x, weight, alpha, mode):
    """sparse_encode.py:19-35.  'zero' (:22-23) is the hot-path default; 'transpose' is a product on
    the library's own GEMM (lasso_init_transpose); 'ridge' and 'lstsq' are linear/utils.py's functions, on its Gram
    and Cholesky kernels (lasso_gram_accumulate + lasso_ridge_solve); 'unif' is torch's RNG like the reference."""
    n_samples = x.size(0)
    n_components = weight.size(1)
    if mode == 'zero':
        z0 = x.new_zeros(n_samples, n_components)
    elif mode == 'unif':
        z0 = x.new(n_samples, n_components).uniform_(-0.1, 0.1)
    elif mode == 'transpose':                                        # :24-25
        if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
            # part of the caller's autograd graph like the reference's torch.matmul: dL/dz0 reaches x, W
            z0 = torch.matmul(x, weight)
        else:                                                        # on the library's NT GEMM
            eng = _engine_for(x, weight)
            if x.dtype == torch.float64 and weight.dtype == torch.float64:       # in double on the fp64-MFMA GEMM
                z0 = eng.init_transpose(eng.to_device(x), eng.to_device(weight)).to(device=x.device)
            else:
                z0 = eng.init_transpose(eng.to_device(x).float().contiguous(),
                                        eng.to_device(weight).float().contiguous()).to(device=x.device, dtype=x.dtype)
    elif mode == 'lstsq':                                            # :26-27 (utils.py:13-25)
        z0 = lstsq(x.T, weight).T
    elif mode == 'ridge':                                            # :28-29 (utils.py:28-40)
        z0 = ridge(x.T, weight, alpha=alpha).T
    else:
        raise ValueError("invalid init parameter '{}'.".format(mode))   # :33
    return z0


def sparse_encode(x, weight, alpha=1.0, z0=None, algorithm='ista', init=None,
                  **kwargs):
    """Same call surface as lasso.linear.sparse_encode (sparse_encode.py:38-73);
    ``algorithm='ista'``, ``'cd'`` and ``'gpsr'`` run on the HIP engine, the other solver names raise
    NotImplementedError (they are outside the accelerated path), anything else
    raises ValueError like the reference (:71)."""
    n_samples = x.size(0)
    n_components = weight.size(1)
    if z0 is not None:
        assert z0.shape == (n_samples, n_components)                 # :44-45
    else:
        if init is None:
            init = _init_defaults.get(algorithm, 'zero')             # :47-48
        if init == 'zero' and algorithm == 'gpsr':
            z0 = None                                                # :22-23: the solver starts from its own zeros (init=0)
        elif init == 'zero' and algorithm == 'ista' and kwargs.get('maxiter', 10) != 0 and n_samples * n_components > 1:
            from .solvers.ista import lazy_zeros
            z0 = lazy_zeros(x, n_samples, n_components)              # :22-23 without the n*k fill (and read)
        else:
            z0 = initialize_code(x, weight, alpha, mode=init)        # :51
    if algorithm == 'ista':
        z = ista(x, z0, weight, alpha, **kwargs)                     # :62-63
    elif algorithm == 'cd':
        z = coord_descent(x, weight, z0, alpha, **kwargs)            # :54-55
    elif algorithm == 'gpsr':
        z = gpsr_basic(x, weight, tau=alpha, x0=z0, **kwargs)        # :56-59 (the dictionary in place of A / AT)
    elif algorithm in _OFF_PATH_ALGOS:
        raise NotImplementedError(
            "lasso_amd accelerates algorithm='ista', 'cd' and 'gpsr'; %r is not on the HIP path" % algorithm)
    else:
        raise ValueError("invalid algorithm parameter '{}'.".format(algorithm))  # :71
    return z
