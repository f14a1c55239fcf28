"""lasso_amd.conv2d.lip_constant without a GPU: the surface (import, signature and defaults: the reference's four
positional names first, read from the fixture's recorded list), every refusal before a native call, the header, export
and binding of the two symbols, the tridiagonal arithmetic of csrc/lanczos_host.hpp through its stand-alone program
(tests/c_host/lanczos_host_main.cpp), also under AddressSanitizer + UBSan, and the host model against the fixture."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import conv_lip_model as model
from conv_lip_cases import (CASES, FINITE, code_size, conv_kwargs, dims, imsize_of, kernel_of, load_case, parity_bar,
                            tol_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lasso_conv_lip_constant_workspace_bytes", "lasso_conv_lip_constant")


@pytest.fixture(scope="module")
def cases(golden):
    return golden("conv_lip_cases")


@pytest.fixture()
def no_native(monkeypatch):
    """any native call, any look for a GPU, fails the test"""
    from lasso_amd import _native as nat

    def boom(*a, **k):
        raise AssertionError("a native call was reached")
    for name in ("lib", "require_gpu", "workspace", "pick_device"):
        monkeypatch.setattr(nat, name, boom)


def test_surface(cases):
    from lasso_amd.conv2d import lip_constant
    from lasso_amd.conv2d.lip_const import lip_constant as direct
    assert lip_constant is direct
    recorded = json.loads(str(cases["signature_json"]))
    assert [p[0] for p in recorded] == ["kernel", "imsize", "transpose", "sqrt", "kwargs"]
    params = list(inspect.signature(lip_constant).parameters.values())
    for ours, (name, has_default, default, kind) in zip(params[:4], recorded[:4]):
        assert ours.name == name and ours.kind.name == kind
        assert (ours.default is not inspect.Parameter.empty) == has_default
        if has_default:
            assert ours.default == default
    extra = {p.name: p for p in params[4:]}
    assert list(extra) == ["tol", "maxiter", "return_info", "kwargs"]
    assert all(extra[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("tol", "maxiter", "return_info"))
    assert extra["tol"].default is None and extra["maxiter"].default is None and extra["return_info"].default is False
    assert extra["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert inspect.signature(__import__("lasso_amd.conv2d", fromlist=["x"]).ista_conv2d).parameters["lr"].default == "auto"


def test_refusals_fire_before_any_native_call(no_native):
    from lasso_amd.conv2d import lip_constant
    w = torch.ones(4, 2, 3, 3)
    for key in ("dilation", "groups", "output_padding", "bias"):
        with pytest.raises(NotImplementedError, match=key):
            lip_constant(w, (8, 8), **{key: 1})
    for dtype in (torch.bfloat16, torch.float16, torch.int32):
        with pytest.raises(NotImplementedError, match=str(dtype).replace("torch.", "")):
            lip_constant(w.to(dtype), (8, 8))
    # (H + 2p - kh) % stride != 0: the image does not round-trip -- height, width, and a pair of strides
    for imsize, kw in (((8, 9), dict(stride=2)), ((9, 8), dict(stride=2)), ((9, 9), dict(stride=(1, 3), padding=1)),
                       ((2, 8), dict())):
        with pytest.raises(ValueError, match="round-trip"):
            lip_constant(w, imsize, **kw)
    with pytest.raises(ValueError):
        lip_constant(w, (1, 1), transpose=True, padding=2)       # conv_transpose2d of the code would be empty
    with pytest.raises(ValueError):
        lip_constant(w, (8, 8), tol=-1.0)
    with pytest.raises(ValueError):
        lip_constant(w, (8, 8), tol=float("nan"))
    with pytest.raises(ValueError):
        lip_constant(w, (8, 8), maxiter=0)
    with pytest.raises(ValueError):
        lip_constant(w[0], (8, 8))
    # what is accepted gets as far as the first native call: transpose=True needs no round trip, a kernel that requires
    # grad is detached
    for call in (lambda: lip_constant(w, (8, 8)), lambda: lip_constant(w, (4, 5), transpose=True, stride=2),
                 lambda: lip_constant(w.double().requires_grad_(), (9, 9), stride=2, padding=(1, 1), sqrt=True)):
        with pytest.raises(AssertionError, match="native call"):
            call()


def test_header_export_and_binding():
    header = open(os.path.join(ROOT, "include", "lasso_hip.h")).read()
    assert re.search(r"#define LASSO_HIP_ABI_VERSION 7\b", header)
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header), sym
    for word in ("lasso_conv_lip_options", "lasso_conv_lip_result", "LASSO_LIP_CONVERGED", "LASSO_LIP_BREAKDOWN",
                 "LASSO_LIP_MAXITER", "LASSO_LIP_SPACE_CODE"):
        assert word in header
    from lasso_amd import _native as nat
    assert C.sizeof(nat.ConvLipOptions) == 16 and C.sizeof(nat.ConvLipResult) == 64
    assert nat.ConvLipResult.history.offset == 56 and nat.ConvLipResult.dim.offset == 16
    assert nat.LIP_STATUS[:3] == ("converged", "breakdown", "maxiter") and nat.LIP_SPACES == ("image", "code")
    path = nat.lib_path()
    assert os.path.exists(path), "the library is not built"
    lib = C.CDLL(path)
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
    nat._declare(lib)
    assert lib.lasso_conv_lip_constant.argtypes[-5:-3] == [C.POINTER(nat.ConvLipOptions), C.POINTER(nat.ConvLipResult)]
    # the query refuses without a device: a bad dtype, maxiter < 1, an image that does not round-trip -> 0
    q = lib.lasso_conv_lip_constant_workspace_bytes
    assert q(4, 2, 3, 3, 8, 8, 1, 1, 1, 1, 0, nat.LASSO_BF16, 8) == 0
    assert q(4, 2, 3, 3, 8, 8, 1, 1, 1, 1, 0, nat.LASSO_F32, 0) == 0
    assert q(4, 2, 3, 3, 8, 9, 2, 2, 0, 0, 0, nat.LASSO_F32, 8) == 0
    small, large = q(4, 2, 3, 3, 8, 8, 1, 1, 1, 1, 0, nat.LASSO_F32, 8), q(4, 2, 3, 3, 8, 8, 1, 1, 1, 1, 0, nat.LASSO_F32, 64)
    assert 0 < small < large
    assert q(4, 2, 3, 3, 8, 8, 1, 1, 1, 1, 0, nat.LASSO_F64, 64) > large
    # ... and the call itself, before any HIP call
    res, opt = nat.ConvLipResult(), nat.ConvLipOptions(8, 0, 1e-5)
    assert lib.lasso_conv_lip_constant(None, 4, 2, 3, 3, 8, 8, 1, 1, 1, 1, 0, nat.LASSO_F32, C.byref(opt), C.byref(res),
                                       None, 0, None) == nat.LASSO_ERR_BAD_ARG
    assert lib.lasso_conv_lip_constant(None, 4, 2, 3, 3, 8, 8, 1, 1, 1, 1, 0, nat.LASSO_BF16, C.byref(opt), C.byref(res),
                                       None, 0, None) == nat.LASSO_ERR_UNSUPPORTED


SRC = os.path.join(ROOT, "tests", "c_host", "lanczos_host_main.cpp")
INC = os.path.join(ROOT, "pytorch-lasso_amd", "csrc")


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + INC, *extra, SRC, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    return run.stdout


def test_tridiagonal_host_program(tmp_path):
    out = _build_and_run(tmp_path, "lanczos_host", [])
    assert out.startswith("ok ") and int(out.split()[1]) >= 80
    san = _build_and_run(tmp_path, "lanczos_host_san",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert san == out


def test_cases_cover_what_they_are_for(cases):
    assert dims(CASES["one"]) == (1, 1)
    assert dims(CASES["exhaust"])[0] == 64 and CASES["exhaust"]["tol"] == 0.0
    assert min(dims(CASES["few_atoms"])) == dims(CASES["few_atoms"])[1]            # the code space is the smaller one
    assert dims(CASES["rgb"])[0] == 1440 and dims(CASES["c16"])[0] == 4096
    assert code_size(CASES["rect_s2"]) == (5, 4)
    for name in FINITE:
        g = load_case(cases, name)
        assert abs(g["ref64"][0] - g["ref64"][1]) <= 1e-10 * g["ref64"][0]         # what the generator certified
        assert abs(float(g["model64"]) - g["ref64"][0]) <= 1e-9 * g["ref64"][0]
    assert float(cases["exact_lr/ratio"]) >= 1.5 and float(cases["exact_lr/loss_exact"]) < float(cases["exact_lr/loss_auto"])
    for name in ("zero", "nan"):                                                    # the reference raises on both
        assert "ArpackError" in str(load_case(cases, name)["reference32"])
        assert "ArpackError" in str(load_case(cases, name)["reference64"])


@pytest.mark.parametrize("name", [n for n in FINITE if n != "c16"])
def test_model_against_the_fixture(cases, name):
    spec, g = CASES[name], load_case(cases, name)
    ref64 = float(g["ref64"][0])
    for transpose in (False, True):
        w = kernel_of(spec)
        v, info = model.lip_constant(w, imsize_of(spec, transpose), transpose=transpose, tol=tol_of(spec, w.dtype),
                                     return_info=True, **conv_kwargs(spec))
        assert info["dim"] == min(dims(spec)) and info["status"] in ("converged", "breakdown")
        assert abs(v - ref64) / ref64 <= parity_bar(g, torch.float32, tol_of(spec, torch.float32)), (v, ref64)
        if not transpose:
            assert abs(v - float(g["model32"])) <= 1e-6 * ref64 and info["steps"] == int(g["steps32"])
    if name == "delta":
        assert info["status"] == "breakdown" and info["steps"] == 1 and abs(v - 1.0) <= 4 * 1.2e-7


def test_model_on_the_special_kernels():
    for name, want in (("zero", 0.0), ("nan", float("nan"))):
        spec = CASES[name]
        v, info = model.lip_constant(kernel_of(spec), spec["imsize"], return_info=True, **conv_kwargs(spec))
        assert (np.isnan(v) and info["status"] == "nonfinite") if np.isnan(want) else (v == want and info["status"] == "breakdown")
    with pytest.raises(ValueError):
        model.lip_constant(kernel_of(CASES["rect_s2"]), (8, 7), stride=2, padding=1)
