"""HIP-backed coordinate descent: same signatures, defaults and side effects as
``lasso.linear.solvers.coordinate_descent.coord_descent`` (reference coordinate_descent.py:5-54)
and ``coord_descent_mod`` (:57-139), the cyclic variant that stops each row on its duality gap."""
import ctypes as C

import torch

from ... import _native as nat


def coord_descent(x, W, z0=None, alpha=1.0, maxiter=1000, tol=1e-6, verbose=False,
                  return_info=False):
    """x [n,d], W [d,k], z0 [n,k] or None -> z [n,k] = S_alpha(b) (:52).

    Like the reference, a caller-supplied ``z0`` is updated IN PLACE and ends up holding
    the tracked code (:14,47); ``b`` starts at ``x W`` whatever ``z0`` is (:19).  Every
    row stops on its own once its committed change is <= tol*k (:9,45-48).
    ``verbose`` prints the reference's line per step (:49-50) by stepping the HIP solver
    one step at a time.  ``return_info`` (extension) also returns
    ``dict(max_steps=..., n_active=...)``.  No CPU fallback.
    """
    nat.require_gpu()
    if x.dim() != 2 or W.dim() != 2:
        raise RuntimeError("coord_descent expects 2-D x and W")
    d, k = W.shape
    n, d1 = x.shape
    assert d1 == d                                                  # :8
    if z0 is not None:
        assert z0.shape == (n, k)                                   # :13
    if x.dtype != torch.float32 or W.dtype != torch.float32 or (z0 is not None and z0.dtype != torch.float32):
        raise NotImplementedError("lasso_amd: coord_descent is implemented for float32 tensors")
    out_device = x.device
    dev = nat.pick_device(x, W, z0)
    xg = x.detach().to(dev).contiguous()
    wg = W.detach().to(dev).contiguous()
    # the tracked z must land in the caller's z0 storage: work on it directly when it is a
    # row-major device tensor, else on a staged copy that is copied back at the end
    z0g = None
    if z0 is not None:
        z0g = z0.detach()
        if z0g.device != dev or z0g.stride(1) != 1 or (n > 1 and z0g.stride(0) < k):
            z0g = z0g.to(dev).contiguous()
    L = nat.lib()
    z = torch.empty((n, k), dtype=torch.float32, device=dev)
    n_active, max_steps = C.c_int32(0), C.c_int32(0)
    if n > 0:
        with torch.cuda.device(dev):
            ws = nat.workspace(dev, L.lasso_cd_workspace_bytes(n, d, k, nat.LASSO_F32), "cd")
            wsp, wsn, st = nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)
            ldz0 = z0g.stride(0) if z0g is not None else 0
            if n == 1 and z0g is not None:
                ldz0 = max(ldz0, k)
            if not verbose:
                nat.check(L.lasso_cd_solve(
                    nat.ptr(xg), xg.stride(0), nat.ptr(wg), wg.stride(0), nat.ptr(z0g), ldz0,
                    nat.ptr(z), z.stride(0), n, d, k, nat.LASSO_F32, float(alpha), int(maxiter),
                    float(tol), C.byref(n_active) if return_info else None,
                    C.byref(max_steps) if return_info else None, wsp, wsn, st))
            else:
                from ...engine import HipEngine
                eng = HipEngine(dev)
                nat.check(L.lasso_cd_prepare(nat.ptr(xg), xg.stride(0), nat.ptr(wg), wg.stride(0),
                                             nat.ptr(z0g), ldz0, n, d, k, nat.LASSO_F32, wsp, wsn, st))
                n_active.value = n
                for i in range(int(maxiter)):                       # :42-50
                    if n_active.value == 0:
                        break
                    nat.check(L.lasso_cd_run(n, d, k, float(alpha), float(tol) * k, 1,
                                             C.byref(n_active), C.byref(max_steps), wsp, wsn, st))
                    nat.check(L.lasso_cd_finish(nat.ptr(z), z.stride(0), None, 0, n, d, k,
                                                float(alpha), wsp, wsn, st))
                    _, sums = eng.objective_sums(xg, z, wg, alpha)
                    s = sums.tolist()
                    print('iter %i - loss: %0.4f' % (i, 0.5 * s[0] + alpha * s[1]))
                nat.check(L.lasso_cd_finish(nat.ptr(z), z.stride(0), nat.ptr(z0g), ldz0, n, d, k,
                                            float(alpha), wsp, wsn, st))
        if z0 is not None and z0g.data_ptr() != z0.data_ptr():
            z0.detach().copy_(z0g)                                   # :47 (in-place on the caller's z0)
    if z.device != out_device:
        z = z.to(out_device)
    if return_info:
        return z, dict(max_steps=max_steps.value, n_active=n_active.value)
    return z


def coord_descent_mod(x, W, z0=None, alpha=1.0, max_iter=1000, tol=1e-4, return_info=False):
    """x [n,d], W [d,k], z0 [n,k] or None -> (z [n,k], gap [n])  (reference coordinate_descent.py:57-139).

    Cyclic coordinate descent after sklearn's ``enet_coordinate_descent``: every sweep updates the coordinates in atom
    order (:110-129, atoms of zero norm are skipped and keep their start value); a row is checked after a sweep once
    its largest change is below ``tol`` times its largest coordinate, when its code is zero, or on the last sweep
    (:132), and stops when its duality gap (:87-99) is below ``tol * ||x_row||^2``.  ``gap`` is the last gap evaluated
    for each row (``tol + 1`` where none was, :78).  All rows are solved by ONE kernel launch (csrc/cd_mod.hip).

    Like the reference, a caller-supplied ``z0`` is the working tensor: it is updated IN PLACE and is what ``z``
    returns (:76,139).

    Deviation: the reference allocates ``z`` as ``[n_features, n_components]`` (:73) and asserts that shape on ``z0``
    (:75), so it only runs when ``n == d`` (or ``n == 1``).  Here ``z`` and ``z0`` are ``[n_samples, n_components]``,
    the evident intent and the same thing whenever the reference runs.

    ``return_info`` (extension): also returns ``dict(sweeps=<int32 [n]>, converged=<bool [n]>, committed=<int>)``,
    ``committed`` being the coordinate updates that changed a value, over all rows and sweeps.
    float32 tensors on any device (tensors on the CPU are staged); other dtypes and ``k > 4096`` raise
    ``NotImplementedError``.  No CPU fallback.
    """
    if x.dim() != 2 or W.dim() != 2:
        raise RuntimeError("coord_descent_mod expects 2-D x and W")
    d, k = W.shape
    n = x.shape[0]
    assert x.shape[1] == d                                          # :71
    if z0 is not None:
        assert z0.shape == (n, k)                                   # :75, with the [n_samples, n_components] shape
    for t in (x, W, z0):
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError("lasso_amd: coord_descent_mod is implemented for float32 tensors, got %s"
                                      % str(t.dtype).replace("torch.", ""))
    if k > 4096:
        raise NotImplementedError("lasso_amd: coord_descent_mod is implemented for k <= 4096, got k=%d" % k)
    max_iter = int(max_iter)
    if max_iter < 0 or not alpha >= 0:
        raise ValueError("coord_descent_mod: max_iter=%d alpha=%g" % (max_iter, alpha))
    nat.require_gpu()
    out_device = x.device if z0 is None else z0.device
    dev = nat.pick_device(x, W, z0)
    xg = x.detach().to(dev).contiguous()
    wg = W.detach().to(dev).contiguous()
    # the solve works on the caller's z0 storage when it is a row-major device tensor, else on a staged copy that is
    # copied back at the end
    if z0 is None:
        zg = torch.empty((n, k), dtype=torch.float32, device=dev)
    else:
        zg = z0.detach()
        if zg.device != dev or zg.stride(1) != 1 or (n > 1 and zg.stride(0) < k):
            zg = zg.to(dev).contiguous()
    gap = torch.empty(n, dtype=torch.float32, device=dev)
    sweeps = torch.zeros(n, dtype=torch.int32, device=dev) if return_info else None
    conv = torch.zeros(n, dtype=torch.uint8, device=dev) if return_info else None
    committed = C.c_int64(0)
    if n > 0 and k > 0:
        L = nat.lib()
        with torch.cuda.device(dev):
            ws = nat.workspace(dev, L.lasso_cd_mod_workspace_bytes(n, d, k, nat.LASSO_F32), "cd_mod")
            ldz = max(zg.stride(0), k) if n == 1 else zg.stride(0)
            nat.check(L.lasso_cd_mod_solve(
                nat.ptr(xg), xg.stride(0) if n > 1 else max(xg.stride(0), d), nat.ptr(wg),
                wg.stride(0) if d > 1 else max(wg.stride(0), k), nat.ptr(zg), ldz, 0 if z0 is None else 1,
                nat.ptr(gap), nat.ptr(sweeps), nat.ptr(conv), n, d, k, nat.LASSO_F32, float(alpha), max_iter,
                float(tol), None, C.byref(committed) if return_info else None, nat.ptr(ws), ws.numel(),
                nat.stream_ptr(dev)))
        if z0 is not None and zg.data_ptr() != z0.data_ptr():
            z0.detach().copy_(zg)                                    # :76 (in place on the caller's z0)
    else:
        gap.fill_(float(tol) + 1.0)                                  # :78, nothing to sweep
        if z0 is None:
            zg.zero_()
    z = z0 if z0 is not None else zg
    if z.device != out_device:
        z = z.to(out_device)
    if gap.device != out_device:
        gap = gap.to(out_device)
    if return_info:
        return z, gap, dict(sweeps=sweeps.to(out_device), converged=conv.to(out_device).bool(),
                            committed=committed.value)
    return z, gap
