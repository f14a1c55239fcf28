#!/usr/bin/env python3
"""coord_descent_mod on the HIP path (csrc/cd_mod.hip) on bench.py's config 2
(n = 4096, d = 256, k = 1024, fp32, alpha = 0.2) with the reference's defaults tol = 1e-4, max_iter = 1000:
  cd_mod      lasso_amd coord_descent_mod(return_info=True): ms per solve (the two setup products and the one solve
              launch; device events around the whole call, median with min .. max of --reps calls after --warmup),
              rows converged, total sweeps, and `committed` -- the coordinate updates that changed a value -- against
              k x total sweeps, the coordinate visits of the reference's loop over atoms
  ista        for context: FISTA (sparse_encode, lr='auto', no stop rule) at the smallest iteration count of a doubling
              ladder whose mean objective is at or below cd_mod's; ms per solve at that count, timed the same way and
              alternated with cd_mod
  model       for context: the reference's loop in plain torch on the CPU (tests/cd_mod_model.py) on the first
              --model-rows rows, wall-clock seconds, once
One JSON line.
  --shape n,d,k   another shape        --out PATH   also append the line to this file
  --profile       run only warm-up + one cd_mod solve (for a kernel trace: rocprofv3 --kernel-trace --stats -- python ...)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-lasso_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402


def _once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ms):
    ms = sorted(ms)
    return dict(ms_per_solve=statistics.median(ms), min=ms[0], max=ms[-1], calls=len(ms))


def objective(x, w, z, alpha):
    r = x.double() - z.double() @ w.double().T
    return float((0.5 * r.pow(2).sum() + alpha * z.double().abs().sum()) / x.shape[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", default="4096,256,1024")
    ap.add_argument("--alpha", type=float, default=0.2)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model-rows", type=int, default=64)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from lasso_amd.linear import sparse_encode
    from lasso_amd.linear.solvers import coord_descent_mod
    n, d, k = (int(v) for v in args.shape.split(","))
    g = torch.Generator().manual_seed(0)
    w = torch.nn.functional.normalize(torch.randn(d, k, generator=g), dim=0)
    x = torch.randn(n, d, generator=g)
    xg, wg = x.cuda(), w.cuda()

    def cd():
        return coord_descent_mod(xg, wg, alpha=args.alpha, max_iter=args.max_iter, tol=args.tol, return_info=True)
    for _ in range(args.warmup):
        z, gap, info = cd()
    torch.cuda.synchronize()
    if args.profile:
        cd()
        torch.cuda.synchronize()
        return
    z, gap, info = cd()
    sweeps = int(info["sweeps"].sum())
    obj_cd = objective(xg, wg, z, args.alpha)
    rec = {"shape": [n, d, k], "alpha": args.alpha, "tol": args.tol, "max_iter": args.max_iter,
           "rows_converged": int(info["converged"].sum()), "total_sweeps": sweeps,
           "max_sweeps": int(info["sweeps"].max()), "committed": int(info["committed"]),
           "atom_visits_k_x_sweeps": k * sweeps, "committed_share": info["committed"] / max(1, k * sweeps),
           "nonzeros_per_row": float((z != 0).sum()) / n, "mean_objective": obj_cd,
           "max_gap_over_tol_row": float((gap / (args.tol * xg.pow(2).sum(1))).max())}
    # FISTA to the same objective
    iters, z_i = None, None
    for m in (25, 50, 100, 200, 400, 800, 1600, 3200):
        z_i = sparse_encode(xg, wg, alpha=args.alpha, algorithm="ista", maxiter=m, tol=0.0)
        iters = m
        if objective(xg, wg, z_i, args.alpha) <= obj_cd:
            break
    rec["ista"] = {"iterations": iters, "mean_objective": objective(xg, wg, z_i, args.alpha),
                   "reached": objective(xg, wg, z_i, args.alpha) <= obj_cd}
    legs = {"cd_mod": cd,
            "ista": lambda: sparse_encode(xg, wg, alpha=args.alpha, algorithm="ista", maxiter=iters, tol=0.0)}
    times = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, fn in legs.items():
            times[name].append(_once(fn))
    rec["cd_mod"] = _stats(times["cd_mod"])
    rec["ista"].update(_stats(times["ista"]))
    # the reference's loop on the CPU
    if args.model_rows > 0:
        import cd_mod_model
        rows = min(n, args.model_rows)
        t0 = time.time()
        zm, _, im = cd_mod_model.coord_descent_mod(x[:rows].clone(), w, alpha=args.alpha, max_iter=args.max_iter,
                                                   tol=args.tol)
        rec["model_cpu"] = {"rows": rows, "seconds": time.time() - t0, "total_sweeps": int(im["sweeps"].sum()),
                            "max_abs_diff_vs_hip": float((zm - z[:rows].cpu()).abs().max())}
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
