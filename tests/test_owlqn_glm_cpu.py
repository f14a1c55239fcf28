"""owlqn on the logistic objective ``bernoulli(x, weight)`` without a GPU: the Python surface is owlqn's own, the new
description is a NamedTuple exported from the package, the C boundary declares and exports lasso_owlqn_glm_solve and
refuses an unknown family (and everything lasso_owlqn_solve refuses) before any HIP call, Python's refusals come before
any native call, the host model (tests/owlqn_glm_model.py) reproduces the fixture recorded from the reference (bit for
bit on the kind of CPU it was recorded on, within the stored spread elsewhere), and every stored case satisfies the
caps it was admitted under."""
import ctypes
import inspect
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import owlqn_glm_model as model
from owlqn_glm_cases import CASES, MID, RAGGED, SATURATION, SMALL, SPREAD_F_CAP, SPREAD_Z_CAP, TALL, WIDE
from owlqn_glm_cases import admitted_f, case_inputs, load_case
from test_owlqn_cpu import recorded_on_this_kind_of_cpu  # noqa: F401  (the fixture: this CPU rounds as the recording one)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    return golden("owlqn_glm_cases")


def test_python_surface():
    import lasso_amd.nonlinear as pkg
    from lasso_amd.nonlinear import bernoulli, owlqn, rss
    assert pkg.bernoulli is bernoulli and issubclass(bernoulli, tuple) and bernoulli._fields == ("x", "weight")
    assert bernoulli is not rss and not issubclass(bernoulli, rss)
    x, w = torch.rand(4, 3), torch.randn(3, 5)
    fun = bernoulli(x, w)
    assert fun.x is x and fun.weight is w and not callable(fun)
    with pytest.raises(AttributeError):
        fun.x = w                                                        # immutable
    # one function serves both objectives: the reference's names, order and defaults, plus return_info
    sig = inspect.signature(owlqn)
    assert list(sig.parameters) == ["fun", "x0", "alpha", "lr", "max_iter", "xtol", "history_size", "line_search",
                                    "ls_options", "verbose", "return_info"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["alpha"], d["lr"], d["max_iter"], d["xtol"], d["history_size"], d["line_search"], d["ls_options"],
            d["verbose"], d["return_info"]) == (1., 1, 20, 1e-5, 100, "brent", None, 0, False)
    doc = owlqn.__doc__
    assert "owlqn(bernoulli(x, weight), z0" in doc and "binary_cross_entropy_with_logits(z @ weight.T, x, reduction='sum')" in doc
    assert "double fold of per-element float32 losses" in doc and "exp(-|u|)" in doc


def test_symbol_declared_and_exported():
    from lasso_amd import _native
    text = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()
    assert "lasso_owlqn_glm_solve" in text and "#define LASSO_GLM_BERNOULLI 1" in text
    assert "#define LASSO_HIP_ABI_VERSION 7" in text          # additive: the version stays
    assert hasattr(ctypes.CDLL(_native.lib_path()), "lasso_owlqn_glm_solve")
    assert _native.GLM_BERNOULLI == 1 and _native.lib().lasso_hip_abi_version() == 7


def _solve_status(L, nat, family=1, n=4, d=3, k=5, dtype=None, ldx=None, x=1, ws=1, alpha=0.1, opts=1, result=1, **fields):
    """lasso_owlqn_glm_solve with fake (never dereferenced) pointers: every refusal comes before the first HIP call"""
    p = lambda on: ctypes.c_void_p(0x1000 if on else 0)                                  # noqa: E731
    o = nat.OwlqnOptions(fields.get("maxiter", 3), fields.get("line_search", 0), fields.get("ls_maxiter", 500),
                         fields.get("history_size", 100), 1.0, 1e-5, 0.1, 0.95, 0)
    r = nat.OwlqnResult()
    return L.lasso_owlqn_glm_solve(p(x), d if ldx is None else ldx, p(1), k, p(1), k, p(1), k, n, d, k,
                                   nat.LASSO_F32 if dtype is None else dtype, alpha, family,
                                   ctypes.byref(o) if opts else None, ctypes.byref(r) if result else None, p(ws), 0, None)


def test_c_abi_refusals_need_no_device():
    from lasso_amd import _native as nat
    L = nat.lib()
    bad, unsup = nat.LASSO_ERR_BAD_ARG, nat.LASSO_ERR_UNSUPPORTED
    for family in (0, 2, -1, 7):
        assert _solve_status(L, nat, family=family) == unsup, family
        assert "family" in L.lasso_hip_last_error().decode()
    assert _solve_status(L, nat, dtype=nat.LASSO_F64) == unsup
    assert _solve_status(L, nat, maxiter=5000, history_size=5000) == unsup
    for kw in (dict(x=0), dict(ws=0), dict(ldx=2), dict(n=-1), dict(d=0), dict(k=0), dict(alpha=-1.0),
               dict(alpha=float("nan")), dict(line_search=3), dict(maxiter=-1), dict(history_size=0),
               dict(line_search=1, ls_maxiter=0), dict(opts=0), dict(result=0)):
        assert _solve_status(L, nat, **kw) == bad, kw
    assert _solve_status(L, nat, n=0, x=0, ws=0) == nat.LASSO_OK                      # nothing to do, nothing written
    # a well-formed call gets as far as the workspace check (0 bytes given), still without a launch -- k beyond 4096 too
    for mode in (0, 1, 2):
        assert _solve_status(L, nat, line_search=mode) == nat.LASSO_ERR_WORKSPACE
    assert _solve_status(L, nat, k=4100) == nat.LASSO_ERR_WORKSPACE


def test_refusals_come_before_any_native_call(monkeypatch):
    from lasso_amd import _native
    from lasso_amd.nonlinear import bernoulli, iterative_ridge_bfgs, owlqn

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_native, "lib", boom)
    monkeypatch.setattr(_native, "require_gpu", boom)
    w, x, z0 = torch.randn(16, 40), torch.rand(24, 16), torch.zeros(24, 40)
    fun = bernoulli(x, w)
    # any other fun keeps the message it had; iterative_ridge_bfgs keeps refusing everything but rss
    with pytest.raises(NotImplementedError, match=r"only rss\(x, weight\) objectives run on the HIP path"):
        owlqn(lambda z: F.binary_cross_entropy_with_logits(z @ w.T, x, reduction='sum'), z0)
    with pytest.raises(NotImplementedError, match=r"only rss\(x, weight\) objectives run on the HIP path \(got bernoulli\)"):
        iterative_ridge_bfgs(fun, z0)
    with pytest.raises(RuntimeError) as e:
        owlqn(fun, z0, line_search="armijo")
    assert type(e.value) is RuntimeError
    with pytest.raises(TypeError, match="shrink"):
        owlqn(fun, z0, line_search="backtrack", ls_options=dict(shrink=0.5))
    with pytest.raises(RuntimeError, match=r"bernoulli\(x, weight\) expects 2-D tensors"):
        owlqn(bernoulli(x[0], w), z0)
    with pytest.raises(AssertionError) as e:
        owlqn(fun, z0[0])                                                # assert x0.dim() == 2
    assert "native call" not in str(e.value)
    with pytest.raises(AssertionError) as e:
        owlqn(fun, torch.zeros(24, 39))
    assert "native call" not in str(e.value)
    for f, z in ((bernoulli(x.double(), w.double()), z0.double()), (fun, z0.double()), (bernoulli(x, w.double()), z0)):
        with pytest.raises(NotImplementedError, match="float64"):
            owlqn(f, z)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        owlqn(bernoulli(x.bfloat16(), w.bfloat16()), z0.bfloat16())
    with pytest.raises(ValueError):
        owlqn(fun, z0, history_size=0)
    with pytest.raises(ValueError):
        owlqn(fun, z0, alpha=-1.0)
    with pytest.raises(NotImplementedError, match="pairs"):
        owlqn(fun, z0, history_size=4000, max_iter=4000)
    # a well-formed call reaches the native layer: targets are not validated, k beyond 4096 is no refusal
    with pytest.raises(AssertionError, match="native call"):
        owlqn(bernoulli(3.0 * x - 1.0, w.requires_grad_()), z0)
    with pytest.raises(AssertionError, match="native call"):
        owlqn(bernoulli(torch.rand(2, 3), torch.randn(3, 4100)), torch.zeros(2, 4100))


def test_no_gpu_is_a_native_error_not_a_cpu_result():
    from lasso_amd import _native
    from lasso_amd.nonlinear import bernoulli, owlqn
    if torch.cuda.is_available():        # a GPU is visible: tests/test_owlqn_glm_gpu.py covers the solve
        return
    with pytest.raises(_native.NativeError):
        owlqn(bernoulli(torch.rand(4, 3), torch.randn(3, 5)), torch.zeros(4, 5), max_iter=2)


def test_the_model_is_the_formula_and_stays_finite_where_it_saturates():
    """the model's objective is binary_cross_entropy_with_logits, its residual autograd's gradient, in either link; at
    logits of +-120 both are finite while log(1 + exp(u)) written naively is not"""
    spec = CASES["sat_bt"]
    x, w, z0 = case_inputs(spec)
    u = z0 @ w.T
    assert float(u.abs().max()) >= 100.0 and abs(float(u.abs().max()) - SATURATION) <= 1e-3 * SATURATION
    assert not torch.isfinite(torch.log(1 + torch.exp(u))).all()
    zg = z0.clone().requires_grad_()
    f = F.binary_cross_entropy_with_logits(zg @ w.T, x, reduction='sum')
    (g,) = torch.autograd.grad(f, zg)
    for link64 in (False, True):
        m = model.Model(w, x, spec["alpha"], link64=link64)
        fm, gm, _ = m.evaluate(z0)
        assert torch.isfinite(fm) and torch.isfinite(gm).all()
        assert abs(float(fm) - float(f) - spec["alpha"] * float(z0.abs().sum())) <= 1e-6 * float(fm)
        assert float((gm - g).abs().max()) <= 1e-5 * float(g.abs().max())
    assert abs(model.objective64(w, x, z0, spec["alpha"]) - float(m.evaluate(z0)[0])) <= 1e-6 * float(f)


def test_every_stored_case_satisfies_its_caps(cases):
    assert {key.split("/")[0] for key in cases.files} == set(CASES)
    by_codes = set()
    for name, spec in CASES.items():
        g = load_case(cases, name)
        n, k = spec["n"], spec["k"]
        kw = spec["kwargs"]
        assert g["z32"].shape == (n, k) and g["z32"].dtype == np.float32
        assert g["z64"].shape == (n, k) and g["z64"].dtype == np.float64
        its = len(g["f32"])
        assert its <= kw["max_iter"] and len(g["t32"]) == len(g["ls32"]) == len(g["dx32"]) == len(g["pairs"]) == its
        assert np.isfinite(g["f32"]).all() and np.isfinite(g["f64"]).all()
        if spec["compare"] == "z":
            by_codes.add((n, spec["d"], k))
            assert float(g["spread_z"]) <= SPREAD_Z_CAP, name                # (c)
        if spec["compare"] == "f":
            assert float(g["spread_f"]) <= SPREAD_F_CAP, name                # (d)
        for fn, bound, f in g["decisions32"]:                                # (a)
            assert abs(fn - bound) >= 1e-4 * abs(f), name
        for _, ys in g["curvature32"]:
            assert ys >= 10 * model.CURV_MIN or ys <= model.CURV_MIN / 10, name
        xtol = kw.get("xtol", 1e-5)
        assert (np.abs(g["dx32"] - xtol) >= 0.01 * xtol).all(), name
        assert (g["pairs"] <= kw.get("history_size", 100)).all()
    # every shape has a case compared by its codes; at most a third of the cases are compared by properties alone
    assert by_codes == {(c["n"], c["d"], c["k"]) for c in CASES.values()}
    assert 3 * sum(c["compare"] == "props" for c in CASES.values()) <= len(CASES)
    # every line search on every shape
    for shape in (SMALL, MID, TALL, RAGGED, WIDE):
        runs = [(c["kwargs"]["line_search"], c["kwargs"]["max_iter"]) for c in CASES.values()
                if (c["n"], c["d"], c["k"]) == shape]
        assert {ls for ls, _ in runs} == {"none", "backtrack", "brent"}, shape
        assert ("brent", 1) in runs and any(ls == "brent" and its >= 8 for ls, its in runs), shape
    # the cases that are there for a path took it
    assert 1 <= len(cases["bt_xtol/f32"]) < CASES["bt_xtol"]["kwargs"]["max_iter"]         # stopped by xtol ...
    assert not cases["bt_xtol/pairs"][-1] and not cases["bt_xtol/skipped"][-1]                # ... and no update followed
    assert str(cases["bt_runout/warnings"]).count("line search did not converge.") >= 1
    assert len(cases["iter0/f32"]) == 0 and len(cases["brent_small/f32"]) == 1
    assert cases["all_dropped/skipped"].all() and not cases["all_dropped/pairs"].any()
    assert len(cases["sat_none/f32"]) == 1 and len(cases["sat_bt/f32"]) == 1
    assert CASES["bt_wide"]["k"] > 4096
    soft = case_inputs(CASES["bt_soft"])[0]
    assert ((soft > 0) & (soft < 1)).any() and set(case_inputs(CASES["bt_mid"])[0].unique().tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_reproduces_fixture(cases, name, recorded_on_this_kind_of_cpu):  # noqa: F811
    """On the kind of CPU the fixture was recorded on the float32 model IS the reference: bit for bit, and within 1e-6
    in float64.  Another CPU's BLAS sums in another order -- it is "another correct float32 implementation", which is
    what spread_z / spread_f measured when the fixture was made: there the codes are held to the GPU tests' bar,
    max(5e-5, 4 x spread_z), with equal trial counts, and the objective-only cases to max(1e-6, 4 x spread_f)."""
    spec, g = CASES[name], load_case(cases, name)
    brent = spec["kwargs"]["line_search"] == "brent"
    if brent:
        pytest.importorskip("scipy")
    x, w, z0 = case_inputs(spec)
    keep = x.clone(), w.clone(), z0.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z, info = model.owlqn(w, x, z0, alpha=spec["alpha"], **spec["kwargs"])
        z64, info64 = model.owlqn(w, x, z0, alpha=spec["alpha"], dtype=torch.float64, **spec["kwargs"])
    assert torch.equal(x, keep[0]) and torch.equal(w, keep[1]) and torch.equal(z0, keep[2])
    assert len(info["warnings"]) == len([m for m in str(g["warnings"]).split("\n") if m])
    assert info["iterations"] == len(g["f32"]) and torch.isfinite(z).all()
    assert info["pairs"] == list(g["pairs"]) and [int(s) for s in info["skipped"]] == list(g["skipped"])
    dz = float((z - torch.from_numpy(g["z32"])).abs().max())
    dz64 = float((z64 - torch.from_numpy(g["z64"])).abs().max())
    if recorded_on_this_kind_of_cpu:
        assert torch.equal(z, torch.from_numpy(g["z32"])), dz
        assert info["ls_iters"] == list(g["ls32"]) and info["t"] == list(g["t32"])
        assert dz64 <= 1e-6
        assert info64["ls_iters"] == list(g["ls64"])
        return
    if info["iterations"] == 0:
        assert torch.equal(z, z0)
        return
    f_rel = abs(info["objective"][-1] - float(g["f32"][-1])) / float(g["f32"][-1])
    f64_rel = abs(info64["objective"][-1] - float(g["f64"][-1])) / float(g["f64"][-1])
    if spec["compare"] == "z":
        assert dz <= max(5e-5, 4.0 * float(g["spread_z"])), (name, dz)
        if not brent:
            assert info["ls_iters"] == list(g["ls32"]) and info64["ls_iters"] == list(g["ls64"])
            assert dz64 <= 1e-6, (name, dz64)
    elif admitted_f(g):
        assert f_rel <= max(1e-6, 4.0 * float(g["spread_f"])), (name, f_rel)
    assert f64_rel <= 1e-6 or not admitted_f(g), (name, f64_rel)
