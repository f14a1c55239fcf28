#!/usr/bin/env python3
"""Generate tests/golden/conjgrad_cases.npz by running the REAL reference's conjugate gradients
(rfeinman/pytorch-lasso, lasso/conjgrad.py: cg, batch_cg, batch_cg_conv2d) on the CPU, in float32 AND in float64.

Runs only where the reference is mounted (/root/reference); the .npz it writes is data: the inputs are re-creatable
from the seeded recipes of tests/conjgrad_cases.py, the expected outputs are stored.  conjgrad.py imports only torch, so
it is loaded by path; no reference file is edited or copied.

Each run is observed with sys.settrace inside conjgrad(): per iteration sum|r| (at the line that tests exit 1),
curv_sum (at the line that tests exit 2) and sqrt(sum rs_new) (at the line that tests exit 0); the exit taken is the
``return terminate(k)`` line reached, the iteration its ``i``.  The printed text of one verbose=2 run is captured, and
the names and defaults of the three public functions are recorded.

Every case is CERTIFIED before it is written (the script exits non-zero otherwise -- choose another seed or tolerance):
  (a) every recorded sum|r| is at least 1 % away from termcond and every sqrt(sum rs) at least 1 % away from tol;
  (b) the float32 and float64 runs end with the same status at the same iteration (cases marked f64_only run in double
      alone: their tolerance cannot fire in float32);
  (c) the model in the reference's order (tests/conjgrad_model.py, every knob off) equals the float32 run bit for bit --
      or else the difference is reported and stored (model_gap) -- and the float64 run to 1e-9;
  (d) spread_x = the maximum over the model's variants (permuted summation orders of the dots, the batch sums and the
      products' contractions; sums folded in double and rounded once) of max|x_variant - x_ref|, spread_seq likewise for the three sequences, relative; every variant stops
      with the same status at the same iteration; a case needs spread_x <= 2.5e-3.

Usage:  python tests/golden/generate_golden_conjgrad.py
"""
import contextlib
import importlib.util
import inspect
import io
import json
import os
import sys
import time

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conjgrad_model as model  # noqa: E402
from conjgrad_cases import (CONV, DENSE, ORDER_SEEDS, SPREAD_X_CAP, VERBOSE_CASE, conv_inputs, conv_kwargs,  # noqa: E402
                            dense_inputs, rel)

_spec = importlib.util.spec_from_file_location("reference_conjgrad", "/root/reference/lasso/conjgrad.py")
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
_MAIN = ref.conjgrad


def _line_of(fragment):
    src, first = inspect.getsourcelines(_MAIN)
    hits = [first + i for i, s in enumerate(src) if fragment in s]
    assert len(hits) == 1, (fragment, hits)
    return hits[0]


L_EXIT1 = _line_of("if r.abs().sum() <= termcond:")
L_EXIT2 = _line_of("if 0 <= curv_sum <= 3 * float_eps:")
L_EXIT0 = _line_of("if rs_new.sum().sqrt() < tol:")
L_RETURN = {_line_of("return terminate(%d)" % k): k for k in range(5)}


class Observer:
    def __init__(self):
        self.r_abs, self.curv_sum, self.rs = [], [], []
        self.status, self.iterations, self.termcond = None, None, None

    def _local(self, frame, event, arg):
        if event == "line" and frame.f_code is _MAIN.__code__:
            loc, no = frame.f_locals, frame.f_lineno
            if no == L_EXIT1:
                self.r_abs.append(float(loc["r"].abs().sum()))
                self.termcond = float(loc["termcond"])
            elif no == L_EXIT2:
                self.curv_sum.append(float(loc["curv_sum"]))
            elif no == L_EXIT0:
                self.rs.append(float(loc["rs_new"].sum().sqrt()))
            elif no in L_RETURN:
                self.status = L_RETURN[no]
                self.iterations = int(loc["i"]) if self.status != 4 else int(loc["maxiter"])
                if self.termcond is None:
                    self.termcond = float(loc["termcond"])
        return self._local

    def __call__(self, frame, event, arg):
        return self._local if frame.f_code is _MAIN.__code__ else None


def observed(call):
    obs = Observer()
    sys.settrace(obs)
    try:
        x = call()
    finally:
        sys.settrace(None)
    return x, obs


def certify(name, spec, run_ref, run_model, tol):
    """run_ref(dtype) -> (x, Observer); run_model(dtype, **knobs) -> (x, info)"""
    t0 = time.time()
    f64_only = bool(spec.get("f64_only"))
    x64, o64 = run_ref(torch.float64)
    runs = [o64]
    if not f64_only:
        x32, o32 = run_ref(torch.float32)
        runs.append(o32)
        if (o32.status, o32.iterations) != (o64.status, o64.iterations):                      # (b)
            raise SystemExit("case %s refused: float32 ends with %d at %d, float64 with %d at %d"
                             % (name, o32.status, o32.iterations, o64.status, o64.iterations))
    for o in runs:                                                                            # (a)
        for v in o.r_abs:
            if abs(v - o.termcond) < 0.01 * o.termcond:
                raise SystemExit("case %s refused: sum|r| %r within 1%% of termcond %r" % (name, v, o.termcond))
        for v in o.rs:
            if abs(v - tol) < 0.01 * tol:
                raise SystemExit("case %s refused: rs %r within 1%% of tol" % (name, v))
    base_dtype = torch.float64 if f64_only else torch.float32
    xb, ob = (x64, o64) if f64_only else (x32, o32)
    m64, i64 = run_model(torch.float64)                                                       # (c)
    gap64 = float((m64 - x64).abs().max()) if x64.numel() else 0.0
    if (i64["status"], i64["iterations"]) != (o64.status, o64.iterations) or gap64 > 1e-9:
        raise SystemExit("case %s: the float64 model disagrees with the reference (gap %g)" % (name, gap64))
    mb, ib = run_model(base_dtype)
    model_gap = float((mb - xb).abs().max())
    exact = torch.equal(mb, xb) and ib["r_abs"] == ob.r_abs and ib["curv_sum"] == ob.curv_sum and ib["rs"] == ob.rs
    if not exact:
        print("case %s: the model is NOT the reference bit for bit (max|dx| = %g)" % (name, model_gap))
    if (ib["status"], ib["iterations"]) != (ob.status, ob.iterations):
        raise SystemExit("case %s: the model stops elsewhere than the reference" % name)
    spread_x, spread_seq = 0.0, 0.0                                                           # (d)
    for knobs in model.variants(ORDER_SEEDS):
        xm, im = run_model(base_dtype, **knobs)
        if (im["status"], im["iterations"]) != (ob.status, ob.iterations):
            raise SystemExit("case %s refused: variant %r stops with %d at %d" % (name, knobs, im["status"], im["iterations"]))
        spread_x = max(spread_x, float((xm - xb).abs().max()))
        spread_seq = max(spread_seq, rel(im["r_abs"], ob.r_abs), rel(im["curv_sum"], ob.curv_sum), rel(im["rs"], ob.rs))
    if not (spread_x <= SPREAD_X_CAP and np.isfinite(spread_seq)):
        raise SystemExit("case %s refused: spread_x = %.3g, spread_seq = %.3g" % (name, spread_x, spread_seq))
    # (x of the float64 run is stored for the float64 cases alone: the others need only its distance, gap_x)
    rec = {"status": np.int64(ob.status), "iterations": np.int64(ob.iterations),
           "r_abs": np.array(ob.r_abs), "curv_sum": np.array(ob.curv_sum), "rs": np.array(ob.rs),
           "termcond": np.float64(ob.termcond), "spread_x": np.float64(spread_x), "spread_seq": np.float64(spread_seq),
           "model_gap": np.float64(model_gap), "model_exact": np.bool_(exact)}
    if f64_only:
        rec["x64"] = x64.numpy()
    else:
        rec["x32"] = x32.numpy()
        rec["gap_x"] = np.float64(float((x32.double() - x64).abs().max()))
    print("%-22s status=%d iterations=%d max|x|=%.3g spread_x=%.2e spread_seq=%.2e model_gap=%.1e exact=%d  %.1fs"
          % (name, ob.status, ob.iterations, float(xb.abs().max()), spread_x, spread_seq, model_gap, exact, time.time() - t0))
    return rec


def dense_case(name, spec):
    kw = dict(spec["kwargs"])
    vector = bool(spec.get("vector"))
    fn_ref, fn_model = (ref.cg, model.cg) if vector else (ref.batch_cg, model.batch_cg)

    def run_ref(dtype):
        A, b = dense_inputs(spec, dtype)
        return observed(lambda: fn_ref(A, b, **kw))

    def run_model(dtype, **knobs):
        A, b = dense_inputs(spec, dtype)
        return fn_model(A, b, **kw, **knobs)

    return certify(name, spec, run_ref, run_model, kw.get("tol", 1e-10))


def conv_case(name, spec):
    kw = dict(spec["kwargs"])

    def run_ref(dtype):
        kernel, b = conv_inputs(spec, dtype)
        return observed(lambda: ref.batch_cg_conv2d(kernel, b, spec["tik"], **kw, **conv_kwargs(spec)))

    def run_model(dtype, **knobs):
        kernel, b = conv_inputs(spec, dtype)
        return model.batch_cg_conv2d(kernel, b, spec["tik"], **kw, **knobs, **conv_kwargs(spec))

    return certify(name, spec, run_ref, run_model, kw.get("tol", 1e-10))


def signatures():
    out = {}
    for fn in ("cg", "batch_cg", "batch_cg_conv2d"):
        sig = inspect.signature(getattr(ref, fn))
        out[fn] = [[p.name, p.default is not inspect.Parameter.empty, None if p.default is inspect.Parameter.empty else p.default,
                    p.kind.name] for p in sig.parameters.values()]
    return out


def main():
    arrays = {}
    for name, spec in DENSE.items():
        for key, val in dense_case(name, spec).items():
            arrays["%s/%s" % (name, key)] = val
    for name, spec in CONV.items():
        for key, val in conv_case(name, spec).items():
            arrays["%s/%s" % (name, key)] = val
    spec = DENSE[VERBOSE_CASE]
    A, b = dense_inputs(spec)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        ref.batch_cg(A, b, verbose=2, **spec["kwargs"])
    arrays["verbose2_text"] = np.array(text.getvalue())
    arrays["signatures_json"] = np.array(json.dumps(signatures()))
    arrays["status_messages_json"] = np.array(json.dumps({str(k): v for k, v in ref._status_messages.items()}))
    path = os.path.join(HERE, "conjgrad_cases.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
