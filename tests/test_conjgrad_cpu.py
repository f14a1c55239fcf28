"""lasso_amd.conjgrad without a GPU: the signatures and defaults are the reference's (read from the fixture's recorded list,
not from the reference tree), the host model reproduces the recorded runs, every refusal fires before a native call, the
default maxiter is computed as the reference computes it, and the exit arithmetic of csrc/conjgrad_host.hpp passes its
stand-alone program (tests/c_host/conjgrad_host_main.cpp), also under AddressSanitizer + UBSan."""
import inspect
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import conjgrad_model as model
from conjgrad_cases import (CONV, DENSE, SPREAD_X_CAP, VERBOSE_CASE, conv_inputs, conv_kwargs, dense_inputs, load_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    return golden("conjgrad_cases")


@pytest.fixture()
def no_native(monkeypatch):
    """any native call, any look for a GPU, fails the test"""
    from lasso_amd import _native as nat

    def boom(*a, **k):
        raise AssertionError("a native call was reached")
    for name in ("lib", "require_gpu", "workspace", "pick_device"):
        monkeypatch.setattr(nat, name, boom)


def test_signatures_and_defaults_are_the_references(cases):
    import lasso_amd.conjgrad as cgm
    recorded = json.loads(str(cases["signatures_json"]))
    assert sorted(recorded) == ["batch_cg", "batch_cg_conv2d", "cg"]
    for fn, params in recorded.items():
        sig = inspect.signature(getattr(cgm, fn))
        ours = [(p.name, p.default, p.kind.name) for p in sig.parameters.values()]
        positional = [(n, d if has else inspect.Parameter.empty, k) for n, has, d, k in params if k != "VAR_KEYWORD"]
        # the reference's parameters in its order, then return_info=False, then (where the reference has it) **conv_kwargs
        assert ours[:len(positional)] == positional, fn
        assert ours[len(positional)] == ("return_info", False, "POSITIONAL_OR_KEYWORD"), fn
        rest = ours[len(positional) + 1:]
        assert rest == [(n, inspect.Parameter.empty, k) for n, has, d, k in params if k == "VAR_KEYWORD"], fn
    assert json.loads(str(cases["status_messages_json"])) == {str(k): v for k, v in cgm._status_messages.items()}
    assert not hasattr(cgm, "conjgrad")                           # the closure-taking form is not provided
    assert "closure" in cgm.__doc__


@pytest.mark.parametrize("name", sorted(DENSE))
def test_model_reproduces_the_dense_runs(cases, name):
    spec, g = DENSE[name], load_case(cases, name)
    f64 = bool(spec.get("f64_only"))
    A, b = dense_inputs(spec, torch.float64 if f64 else torch.float32)
    x, info = (model.cg if spec.get("vector") else model.batch_cg)(A, b, **spec["kwargs"])
    assert info["status"] == int(g["status"]) and info["iterations"] == int(g["iterations"])
    assert float(g["spread_x"]) <= SPREAD_X_CAP
    want = torch.from_numpy(g["x64" if f64 else "x32"])
    if f64:
        assert float((x - want).abs().max()) <= 1e-9
    else:
        # bit for bit on the CPU that made the fixture; within the recorded spread on another one
        assert float((x - want).abs().max()) <= max(5e-5, 4.0 * float(g["spread_x"]))
        assert np.allclose(info["r_abs"], g["r_abs"], rtol=max(1e-5, 4.0 * float(g["spread_seq"])), atol=0)


@pytest.mark.parametrize("name", sorted(CONV))
def test_model_reproduces_the_conv_runs(cases, name):
    spec, g = CONV[name], load_case(cases, name)
    kernel, b = conv_inputs(spec)
    x, info = model.batch_cg_conv2d(kernel, b, spec["tik"], **spec["kwargs"], **conv_kwargs(spec))
    assert info["status"] == int(g["status"]) and info["iterations"] == int(g["iterations"])
    assert float((x - torch.from_numpy(g["x32"])).abs().max()) <= max(5e-5, 4.0 * float(g["spread_x"]))
    assert len(info["r_abs"]) == len(g["r_abs"]) and len(info["rs"]) == len(g["rs"])


def test_fixture_covers_every_exit_and_holds_the_verbose_text(cases):
    statuses = {name: int(load_case(cases, name)["status"]) for name in list(DENSE) + list(CONV)}
    assert statuses["maxiter_2"] == 4 and statuses["abs_tol"] == 0 and statuses["f64_abs_tol"] == 0
    assert statuses[VERBOSE_CASE] == 1
    text = str(cases["verbose2_text"]).split("\n")
    assert text[0].startswith("iter: 0 - rs: ") and text[-2] == "Relative tolerance reached." and text[-1] == ""
    for name in list(DENSE) + list(CONV):
        g = load_case(cases, name)
        # the certified margins: 1 % around termcond (and around tol, by the generator)
        assert all(abs(v - float(g["termcond"])) >= 0.01 * float(g["termcond"]) for v in g["r_abs"]), name


def test_refusals_fire_before_any_native_call(no_native):
    from lasso_amd.conjgrad import batch_cg, batch_cg_conv2d, cg
    A, b = torch.eye(6), torch.ones(4, 6)
    w, bc = torch.ones(5, 2, 3, 3), torch.ones(2, 5, 7, 7)
    for dt in (torch.bfloat16, torch.float16):
        for call in (lambda: cg(A.to(dt), b[0].to(dt)), lambda: batch_cg(A.to(dt), b.to(dt)),
                     lambda: batch_cg_conv2d(w.to(dt), bc.to(dt))):
            with pytest.raises(NotImplementedError, match=str(dt).replace(".", r"\.")):
                call()
    with pytest.raises(NotImplementedError, match=r"torch\.float64"):
        batch_cg_conv2d(w.double(), bc.double())
    for call in (lambda: batch_cg(A.double(), b), lambda: batch_cg(A, b.double()), lambda: cg(A, b[0].double()),
                 lambda: batch_cg_conv2d(w, bc.double())):
        with pytest.raises(NotImplementedError, match=r"torch\.float64"):
            call()
    with torch.enable_grad():
        for call in (lambda: batch_cg(A.clone().requires_grad_(), b), lambda: cg(A, b[0].clone().requires_grad_()),
                     lambda: batch_cg_conv2d(w.clone().requires_grad_(), bc)):
            with pytest.raises(NotImplementedError, match="requires_grad"):
                call()
    for call in (lambda: cg(A, b), lambda: cg(A[0], b[0]), lambda: batch_cg(A, b[0]), lambda: batch_cg(A[:, :5], b),
                 lambda: batch_cg(torch.eye(5), b), lambda: batch_cg_conv2d(w[0], bc), lambda: batch_cg_conv2d(w, bc[0]),
                 lambda: batch_cg_conv2d(w, torch.ones(2, 4, 7, 7))):
        with pytest.raises(AssertionError):
            call()
    for kw in (dict(maxiter=-1), dict(tol=-1e-3), dict(rtol=-1.0), dict(tol=float("nan"))):
        for call in (lambda: cg(A, b[0], **kw), lambda: batch_cg(A, b, **kw), lambda: batch_cg_conv2d(w, bc, **kw)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        batch_cg_conv2d(w, bc, tik=-0.5)
    for key in ("output_padding", "dilation", "groups", "bias"):
        with pytest.raises(NotImplementedError, match=key):
            batch_cg_conv2d(w, bc, **{key: 1})
    # n = 0: an empty tensor without a native call
    x, info = batch_cg(A, b[:0], return_info=True)
    assert x.shape == (0, 6) and info["status"] == 1 and info["iterations"] == 0
    z = batch_cg_conv2d(w, bc[:0])
    assert z.shape == (0, 5, 7, 7)


def test_default_maxiter_is_the_references(monkeypatch):
    """20 * len(b), 20 * b.size(1), 20 * b[0].numel(): what reaches the request"""
    import lasso_amd.conjgrad as cgm
    from lasso_amd import _native as nat
    seen = []

    class Stop(Exception):
        pass

    def request(maxiter, *a):
        seen.append(maxiter)
        raise Stop

    monkeypatch.setattr(cgm, "_request", request)
    for name in ("require_gpu",):
        monkeypatch.setattr(nat, name, lambda: None)
    monkeypatch.setattr(nat, "pick_device", lambda *t: torch.device("cpu"))
    A, b = torch.eye(6), torch.ones(4, 6)
    w, bc = torch.ones(5, 2, 3, 3), torch.ones(2, 5, 7, 7)
    for call in (lambda: cgm.cg(A, b[0]), lambda: cgm.batch_cg(A, b), lambda: cgm.batch_cg_conv2d(w, bc),
                 lambda: cgm.batch_cg(A, b, maxiter=3)):
        with pytest.raises(Stop):
            call()
    assert seen == [120, 120, 20 * 5 * 7 * 7, 3]


SRC = os.path.join(ROOT, "tests", "c_host", "conjgrad_host_main.cpp")
INC = os.path.join(ROOT, "pytorch-lasso_amd", "csrc")


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + INC, *extra, SRC, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    return run.stdout


def test_exit_arithmetic_host_program(tmp_path):
    out = _build_and_run(tmp_path, "conjgrad_host", [])
    assert out.startswith("ok ") and int(out.split()[1]) >= 70
    san = _build_and_run(tmp_path, "conjgrad_host_san",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert san == out
