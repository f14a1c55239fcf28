"""csrc/linesearch_host.hpp -- the momentum recurrence, the step ladder and the F <= Q verdict every host-side line
search shares -- bit for bit against the same arithmetic in numpy, in the reference's operation order (ista.py:23,28,
32-35,45,47,98-99).  A stand-alone program (tests/c_host/linesearch_host_main.cpp, host compiler only) prints the bit
patterns; it is built a second time with AddressSanitizer + UBSan and must come back clean with the same output."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "linesearch_host_main.cpp")
INC = os.path.join(ROOT, "pytorch-lasso_amd", "csrc")

LADDERS = ((1.0, 1.5, 0.5), (30.0, 2.0, 0.3), (1e3, 1.000001, 0.5))
f32, f64 = np.float32, np.float64


def _verdict_rows(T):
    """(five sums, alpha, lr_t, force): the edge cases by construction, then seeded ordinary ones"""
    eps = np.finfo(T).eps
    up = float(T(1.0) + T(eps))                # one ulp above 1 in T
    rows = [
        ((3.0, 3.0, 1.25, 0.0, 0.0), 0.5, 1.0, 0),              # exact tie F == Q, and dz2 = 0
        ((2.0, 2.0 * up, 0.0, 0.0, 0.0), 0.5, 1.0, 0),          # F one ulp above Q: rejected
        ((2.0 * up, 2.0, 0.0, 0.0, 0.0), 0.5, 1.0, 0),          # F one ulp below Q: accepted
        ((2.0, 2.0 * up, 0.0, 0.0, 0.0), 0.5, 1.0, 1),          # force = 1 with F > Q
        ((1.0, 9.0, 2.0, -0.5, 0.25), 0.3, 30.0, 1),            # force = 1, F far above Q
        ((5.0, 4.0, 7.0, -1.5, 0.0), 0.3, 0.4, 0),              # dz2 = 0 with the other sums alive
        ((0.0, 0.0, 0.0, 0.0, 0.0), 0.0, 1e3, 0),               # all zero: a tie
    ]
    rng = np.random.default_rng(11)
    for _ in range(200):       # sums as doubles that are NOT representable in float: T = float must round them first
        rss0, rss1, l1, dz2 = rng.uniform(0.0, 1e4, 4)
        dzg = rng.uniform(-1e3, 1e3)
        rows.append(((rss0, rss1, l1, dzg, dz2), float(rng.uniform(0.0, 2.0)), float(rng.uniform(1e-3, 30.0)), 0))
    return rows


def _script():
    lines = ["coef"]
    for lr0, eta, alpha in LADDERS:
        lines.append("ladder %s %s %s" % (float(lr0).hex(), float(eta).hex(), float(alpha).hex()))
    for T, tag in ((f32, "f"), (f64, "d")):
        for sums, alpha, lr_t, force in _verdict_rows(T):
            lines.append("verdict %s %s %s %s %d" % (tag, " ".join(float(s).hex() for s in sums), float(alpha).hex(),
                                                     float(lr_t).hex(), force))
    return "\n".join(lines) + "\n"


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
    return _build_and_run(tmp_path_factory.mktemp("linesearch_host"), "linesearch_host", [])


def _bits(v):
    v = np.asarray(v)
    return "%0*x" % (2 * v.itemsize, int(v.view(np.uint32 if v.dtype == f32 else np.uint64)))


def _expected():
    out = []
    t = 1.0                                                     # python floats: IEEE doubles, like the reference's
    for i in range(64):
        tn = (1.0 + float(np.sqrt(f64(1.0 + 4.0 * t * t)))) / 2.0                      # ista.py:98
        c = (t - 1.0) / tn                                                              # :99
        out.append("coef %d %s %s %s" % (i, _bits(f32(c)), _bits(f32(0.0)), _bits(f64(c))))
        t = tn
    for lr0, eta, alpha in LADDERS:
        lr = float(lr0)
        for r in range(8):
            out.append("ladder %d %s %s %s" % (r, _bits(f32(lr)), _bits(f32(alpha * lr)), _bits(f32(0.5 / lr))))
            lr = lr / eta                                                               # :47
        out.append("ladder_lr %s" % _bits(f64(lr)))
    for T in (f32, f64):
        for sums, alpha, lr_t, force in _verdict_rows(T):
            rss0, rss1, l1, dzg, dz2 = (T(s) for s in sums)
            f0 = T(0.5) * rss0                                                          # :23
            al1 = T(alpha) * l1
            F = T(0.5) * rss1 + al1                                                     # :28
            Q = ((f0 + dzg) + T(0.5 / lr_t) * dz2) + al1                                # :32-35
            assert type(F) is T and type(Q) is T
            out.append("verdict %s %s %d" % (_bits(F), _bits(Q), 1 if (force or F <= Q) else 0))     # :45
    return out


def test_momentum_ladder_and_verdict_bit_for_bit(printed):
    got, want = printed.splitlines(), _expected()
    assert len(got) == len(want) == 64 + 3 * 9 + 2 * 207
    for g, w in zip(got, want):
        assert g == w, (g, w)


def test_the_edge_cases_are_what_they_claim():
    """the constructed rows really are a tie, one ulp apart, and a forced acceptance of F > Q -- in both precisions"""
    for T in (f32, f64):
        v = [l.split() for l in _expected() if l.startswith("verdict")]
        v = v[:207] if T is f32 else v[207:]
        as_int = lambda h: int(h, 16)
        assert v[0][1] == v[0][2] and v[0][3] == "1"                                   # tie: accepted
        assert as_int(v[1][1]) == as_int(v[1][2]) + 1 and v[1][3] == "0"              # (positive floats: bit patterns order)
        assert as_int(v[2][1]) + 1 == as_int(v[2][2]) and v[2][3] == "1"
        assert as_int(v[3][1]) == as_int(v[3][2]) + 1 and v[3][3] == "1"              # forced
        assert as_int(v[4][1]) > as_int(v[4][2]) and v[4][3] == "1"
        assert {r[3] for r in v[7:]} == {"0", "1"}                                     # the ordinary rows fall both ways


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path, printed):
    out = _build_and_run(tmp_path, "linesearch_host_san",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert out == printed
