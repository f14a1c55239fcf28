"""csrc/brent_host.hpp -- the resumable bounded Brent minimiser behind the orthant-wise Newton solver's default line
search -- against scipy.optimize.minimize_scalar(method='bounded', bounds=(0, 10)) on the same functions: the sequence
of abscissae, the evaluation count and the result, bit for bit (the algorithm is + - * / sqrt and comparisons in
double; both sides are built / run without fused multiply-adds).  A stand-alone program
(tests/c_host/brent_host_main.cpp, host compiler only) prints the bit patterns; it is built a second time with
AddressSanitizer + UBSan and must come back clean with the same output."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "brent_host_main.cpp")
INC = os.path.join(ROOT, "pytorch-lasso_amd", "csrc")

# (mode, a, b, k1, p1, k2, p2, c, level):  g(t) = a (t - b)^2 + k1 |t - p1| + k2 |t - p2| + c
FUNCTIONS = [
    (0, 1.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),                    # smooth quadratics
    (0, 0.37, 7.123456789, 0.0, 0.0, 0.0, 0.0, -2.5, 0.0),
    (0, 250.0, 0.8125, 0.0, 0.0, 0.0, 0.0, 1234.5, 0.0),
    (0, 1e-3, 9.99, 0.0, 0.0, 0.0, 0.0, 5.0, 0.0),
    (0, 1.0, 2.0, 3.0, 1.5, 0.7, 2.5, 10.0, 0.0),                   # |.| kinks, like the line objective
    (0, 12.5, 0.9, 40.0, 1.0, 25.0, 0.6, 500.0, 0.0),               # the minimum AT a kink
    (0, 0.5, 4.0, 2.0, 4.0, 0.0, 0.0, 0.0, 0.0),
    (0, 3.0, 1.2, 1.0, 0.3, 1.0, 6.0, 2000.0, 0.0),
    (0, 1.0, -3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),                   # the minimum at the lower bound
    (0, 1.0, 14.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),                   # ... at the upper bound
    (0, 0.0, 0.0, 1.0, -1.0, 0.0, 0.0, 0.0, 0.0),                   # linear, increasing
    (0, 0.0, 0.0, 1.0, 11.0, 0.0, 0.0, 0.0, 0.0),                   # linear, decreasing
    (1, 12.5, 0.9, 40.0, 1.0, 25.0, 0.6, 2505.0, 0.0),              # rounded through float32 on every call
    (1, 250.0, 0.8125, 3.0, 0.5, 0.0, 0.0, 6696.75, 0.0),
    (1, 1.0, 3.0, 0.0, 0.0, 0.0, 0.0, 1e4, 0.0),
    (2, 1.0, 5.0, 0.0, 0.0, 0.0, 0.0, 0.0, 4.0),                    # a plateau around the minimum
    (2, 1.0, 5.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1e3),                    # a plateau everywhere
]


def _script():
    return "".join("%d %s\n" % (f[0], " ".join(float(v).hex() for v in f[1:])) for f in FUNCTIONS)


def _python_function(spec, seen):
    mode, a, b, k1, p1, k2, p2, c, level = spec

    def g(t):
        t = float(t)
        u = t - b
        f = a * u * u + k1 * abs(t - p1) + k2 * abs(t - p2) + c
        if mode == 1:
            f = float(np.float32(f))
        if mode == 2:
            f = max(f, level)
        seen.append((t, f))
        return f
    return g


def _bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + INC, *extra, SRC, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], input=_script(), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    return run.stdout


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("brent_host"), "brent_host", [])


def test_abscissae_count_and_result_equal_scipy_bit_for_bit(printed):
    minimize_scalar = pytest.importorskip("scipy.optimize").minimize_scalar
    want = []
    for i, spec in enumerate(FUNCTIONS):
        seen = []
        res = minimize_scalar(_python_function(spec, seen), bounds=(0, 10), method="bounded")
        assert res.nfev == len(seen)
        want += ["%d x %s %s" % (i, _bits(t), _bits(f)) for t, f in seen]
        want.append("%d result %s %s %d" % (i, _bits(res.x), _bits(res.fun), res.nfev))
    got = printed.splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g, w)


def test_the_script_reaches_both_kinds_of_step_and_both_bounds(printed):
    """the functions are what they claim: searches of several lengths, results at either bound and in the interior"""
    results = [l.split() for l in printed.splitlines() if " result " in l]
    assert len(results) == len(FUNCTIONS)
    xs = [struct.unpack("<d", struct.pack("<Q", int(r[2], 16)))[0] for r in results]
    counts = [int(r[4]) for r in results]
    assert abs(xs[0] - 3.0) < 1e-5 and abs(xs[5] - 1.0) < 1e-4           # a smooth minimum, and one at a kink
    assert xs[8] < 1e-4 and xs[9] > 10 - 1e-4 and xs[10] < 1e-4 and xs[11] > 10 - 1e-4
    assert min(counts) >= 5 and max(counts) <= 60 and len(set(counts)) > 3
    assert all(0.0 < x < 10.0 for x in xs)


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path, printed):
    out = _build_and_run(tmp_path, "brent_host_san",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert out == printed
