#!/usr/bin/env python3
"""OWL-QN on the logistic objective: the HIP path (``owlqn(bernoulli(x, W), ...)``, csrc/owlqn.hip's link epilogues)
against the same operation sequence issued through torch on the same GPU -- tests/owlqn_glm_model.py on device tensors
with the objective as the reference's user writes it: ``F.binary_cross_entropy_with_logits(z @ W.T, x,
reduction='sum')`` and ``autograd.grad`` for its gradient, the two-loop recursion as 2m dependent dot / add_ pairs, one
host read per line-search trial and per memory update.

Legs alternate in one process, each run timed with device events around the whole solve; the median of --runs (>= 5)
runs per leg is reported with ms per iteration.  Fixed iteration counts (xtol = 0), ``line_search='none'`` (fixed step
0.05) and ``'backtrack'``.  The legs' final objectives are reported side by side and NOT asserted equal -- parity is
held by tests/test_owlqn_glm_gpu.py on certified cases, and these lines are not certifiable: from a zero start the first
step is lr / |pg|_1 ~ 5e-8 or less, every logit moves by ~1e-8, and torch's float32 sigmoid(u) - x does not move off
0.5 - x at all.  The first pair's y.s is then rounding: at 4096 x 256 x 8192 it is 1.17e-9 in float64, 1.15e-9 with the
link in float64 rounded once, and 6.3e-11 in torch's float32 -- below the 1e-10 at which a pair is dropped -- so after 10
fixed steps the host model ends at 473509 (float64), 459830 and 370162; at 4096 x 256 x 1024 the pair is kept but its
scaling is 0.043 against 0.66 in float64, and the runs end 5.6 % apart.  A dozen backtracking iterations flip a trial
sooner or later (87 against 91 evaluations at k = 8192).  Per shape, one more line
times what the new epilogues add: a solve of max_iter = 0 -- the transposition of W, the link (or residual) product,
the gradient product and the fold -- for ``bernoulli`` and for ``rss`` on the same operands, alternated, median of 20.
One JSON line each; --out also writes them to a file.  No threshold is asserted on a time.

  python tools/bench_owlqn_glm.py [--shapes 4096x256x1024,...] [--maxiters 10,20] [--runs 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-lasso_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import owlqn_glm_model as glm  # noqa: E402
from owlqn_glm_cases import recipe  # noqa: E402

FIXED_STEP = 0.05


class AutogradModel(glm.Model):
    """the torch leg's objective: the loss through torch's fused op, its gradient through autograd"""

    def objective(self, z):
        return F.binary_cross_entropy_with_logits(z @ self.w.T, self.x, reduction='sum') + self.alpha * z.norm(p=1), None

    def evaluate(self, z):
        zz = z.detach().requires_grad_(True)
        with torch.enable_grad():
            loss = F.binary_cross_entropy_with_logits(zz @ self.w.T, self.x, reduction='sum')
        g = torch.autograd.grad(loss, zz)[0]
        return loss.detach() + self.alpha * z.norm(p=1), g, glm.pseudo_gradient(z, g, self.alpha)


def torch_route(x, W, z0, alpha, max_iter, search, lr):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z, info = glm.owlqn(W, x, z0, alpha=alpha, lr=lr, max_iter=max_iter, xtol=0.0, line_search=search, model=AutogradModel)
    return z, info["objective"][-1], sum(info["ls_iters"]), info["pairs"][-1]


def hip_route(x, W, z0, alpha, max_iter, search, lr):
    from lasso_amd.nonlinear import bernoulli, owlqn
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z, info = owlqn(bernoulli(x, W), z0, alpha=alpha, lr=lr, max_iter=max_iter, xtol=0.0, line_search=search,
                        return_info=True)
    return z, info["objective"][-1], sum(info["ls_iters"]), info["pairs"][-1]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def evaluation_pair(x, W, z0, alpha, runs=20):
    """median ms of a max_iter = 0 solve (one evaluation of f and g) per objective, the two alternated"""
    from lasso_amd.nonlinear import bernoulli, owlqn, rss
    legs = {"bernoulli": lambda: owlqn(bernoulli(x, W), z0, alpha=alpha, max_iter=0),
            "rss": lambda: owlqn(rss(x, W), z0, alpha=alpha, max_iter=0)}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(runs):
        for name, fn in legs.items():
            ms[name].append(timed(fn)[0])
    return {name: dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v)) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x256x1024,4096x1280x1024,4096x256x8192")
    ap.add_argument("--searches", default="backtrack,none")
    ap.add_argument("--maxiters", default="10,20")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.runs >= 5
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    for shape in a.shapes.split(","):
        n, d, k = map(int, shape.split("x"))
        x, W = recipe(n, d, k, 0)
        x, W = x.cuda(), W.cuda()
        z0 = torch.zeros(n, k, device="cuda")
        # a random start, so that the link sees logits of every size, not sigmoid(0) alone
        z_rand = 0.3 * torch.randn(n, k, device="cuda") * (torch.rand(n, k, device="cuda") < 0.25)
        ev = evaluation_pair(x, W, z_rand, a.alpha)
        emit(dict(shape=[n, d, k], evaluation=ev, bernoulli_over_rss=ev["bernoulli"]["ms_median"] / ev["rss"]["ms_median"]))
        for max_iter in map(int, a.maxiters.split(",")):
            for search in a.searches.split(","):
                lr = FIXED_STEP if search == "none" else 1.0
                legs = {"hip": lambda: hip_route(x, W, z0, a.alpha, max_iter, search, lr),
                        "torch": lambda: torch_route(x, W, z0, a.alpha, max_iter, search, lr)}
                for fn in legs.values():                       # warm-up: workspaces, rocBLAS kernels
                    fn()
                torch.cuda.synchronize()
                ms = {name: [] for name in legs}
                last = {}
                for _ in range(a.runs):
                    for name, fn in legs.items():              # alternate the legs
                        t, last[name] = timed(fn)
                        ms[name].append(t)
                med = {name: statistics.median(v) for name, v in ms.items()}
                rec = dict(shape=[n, d, k], line_search=search, max_iter=max_iter, alpha=a.alpha, lr=lr, runs=a.runs)
                for name in legs:
                    z, f, evals, pairs = last[name]
                    rec[name] = dict(ms_median=med[name], ms_min=min(ms[name]), ms_max=max(ms[name]),
                                     ms_per_iteration=med[name] / max_iter, evaluations=evals, objective=f,
                                     pairs_held=pairs, nnz=int((z != 0).sum()))
                rec["speedup_over_torch"] = med["torch"] / med["hip"]
                rec["objective_rel_diff"] = abs(rec["hip"]["objective"] - rec["torch"]["objective"]) / abs(rec["torch"]["objective"])
                emit(rec)


if __name__ == "__main__":
    main()
