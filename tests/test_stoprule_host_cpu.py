"""csrc/stoprule_host.hpp -- the budget of the stop rule, the two chunk sizers, the speculate-and-replay loop and the four
result words that the host drivers share -- against the same arithmetic in Python: bit for bit where it computes
floats, integer for integer where it schedules, event for event where it drives a solve.  A stand-alone program
(tests/c_host/stoprule_host_main.cpp, host compiler only) prints what the header computes; it is built a second time
with AddressSanitizer + UBSan and must come back clean with the same output.  The sizers are compared against ports
that use math.log / math.log2 -- the same libm as the C++ -- and next_tile_chunk against its twin in
lasso_amd.parallel.  Every function also gets chunks of non-finite sums (NONFINITE_CHUNKS: what a batch with a NaN or
Inf sample produces): no stop, a chunk size in [1, 64], maxiter iterations with a NaN last sum, no undefined cast."""
import math
import os
import subprocess

import numpy as np
import pytest

from lasso_amd import _native as nat
from lasso_amd import parallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "stoprule_host_main.cpp")
INC = os.path.join(ROOT, "pytorch-lasso_amd", "csrc")

f32, f64 = np.float32, np.float64
CHUNK_MAX = 64


def _hex(v):
    return float(v).hex()


def _bits(v):
    v = np.asarray(v)
    return "%0*x" % (2 * v.itemsize, int(v.view(np.uint32 if v.dtype == f32 else np.uint64)))


# ---- stop_budget --------------------------------------------------------------------------------------------------
BUDGET_ROWS = [
    (300, 160, 1e-5), (60, 40, 1e-4), (100, 40, 1e-4),          # products that no float holds
    (3, 7, 0.1), (65536, 1024, 1e-5),                           # 2^26 elements: rows * k above 2^24
    (16777217, 3, 1e-7),                                        # rows itself is no float
    (300, 160, 0.0), (1, 1, 0.0),                               # tol = 0
    (1, 1, 1.0), (4096, 4096, 2.0 ** -30),                      # exact ones
]


def _budget_expected():
    return ["budget %s %s" % (_bits(f32(float(r) * float(k) * tol)), _bits(f64(float(r) * float(k) * tol)))
            for r, k, tol in BUDGET_ROWS]


# ---- chunks of non-finite sums ------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")


def _nonfinite_chunks(c):
    """name -> c sums above a budget of 1: all NaN; NaN from some index on (a NaN code stays NaN); all +Inf; finite then
    +Inf; +Inf then finite (an Inf sample's first sum is +Inf) -- and, for the sizers, a NaN in front of finite sums"""
    fin = [50.0 - 0.5 * i for i in range(c)]
    out = {"all NaN": [NAN] * c, "all +Inf": [INF] * c}
    for at in sorted({1, c // 2 - 1, c // 2, c // 2 + 1, c - 1} & set(range(1, c))):
        out["NaN from %d on" % at] = fin[:at] + [NAN] * (c - at)
        out["finite then +Inf from %d" % at] = fin[:at] + [INF] * (c - at)
        out["+Inf then finite from %d" % at] = [INF] * at + fin[at:]
        out["NaN then finite from %d" % at] = [NAN] * at + fin[at:]
    return out


NONFINITE_CHUNKS = [(name, sums) for c in (1, 8, 9, 64) for name, sums in sorted(_nonfinite_chunks(c).items())]


# ---- next_tile_chunk ----------------------------------------------------------------------------------------------
def _decaying(left, c=8, lo=8.0, budget=1.0):
    """a chunk of c sums whose halves' maxima predict about `left` iterations to the budget"""
    h = c // 2
    hi = lo * math.exp(math.log(lo / budget) * h / left)
    sums = [hi] * h + [lo] * (c - h)
    sums[1] *= 0.9                        # (the maxima, not the first / last sums, are what counts)
    sums[-1] *= 0.8
    return budget, [float(f32(s)) for s in sums]


def _tile_rows():
    rows = [_decaying(left) for left in (127.9, 128.1, 13.5, 14.5, 70.5, 71.5, 30.5, 6.5, 200.0)]
    rows += [_decaying(40.5, c=c) for c in (9, 33, 64)]
    rows.append((1.0, [3.0, 3.5, 3.9, 3.0, 4.0, 3.0, 2.0, 1.5]))          # lo <= 4 budget, no decay
    rows.append((1.0, [9.0, 9.0, 9.0, 9.0, 4.0, 3.0, 2.0, 1.5]))          # lo <= 4 budget behind a decaying half
    rows.append((1.0, [5.0, 6.0, 7.0, 8.0, 8.0, 7.0, 6.0, 5.0]))          # hi == lo: no decay
    rows.append((1.0, [5.0, 5.0, 5.0, 5.0, 6.0, 7.0, 8.0, 9.0]))          # growing
    rows.append((1.0, [50.0, 40.0, 30.0, 20.0, 10.0, 8.0, 6.0]))          # c < 8
    rows.append((1.0, [50.0]))
    rows.append((0.0, [50.0, 40.0, 30.0, 20.0, 10.0, 8.0, 6.0, 5.0]))     # budget = 0
    rows.append((0.0, [0.0] * 8))
    rng = np.random.default_rng(23)
    for _ in range(300):
        c = int(rng.integers(1, 65))
        rate = rng.uniform(0.0, 0.3)
        s = rng.uniform(1.0, 1e4) * np.exp(-rate * np.arange(c)) * rng.uniform(0.8, 1.2, c)
        budget = float(f32(s[-1] * rng.choice([0.9, 0.3, 0.05, 1e-3, 1e-6])))
        rows.append((budget, [float(v) for v in s.astype(f32)]))
    return rows + _tile_rows_nonfinite()


def _tile_rows_nonfinite():
    return [(budget, sums) for budget in (1.0, 20.0, 0.0) for _, sums in NONFINITE_CHUNKS]


def _left(budget, sums):
    h = len(sums) // 2
    hi, lo = max(sums[:h]), max(sums[h:])
    return math.log(lo / budget) / (math.log(hi / lo) / h)


# ---- next_stop_chunk ----------------------------------------------------------------------------------------------
def _next_stop_chunk(first, last, budget, c, it, chunk_max):
    """stoprule_host.hpp, line for line (the arguments hold values of T; the logarithms are taken in double)"""
    nxt = 1
    if last > 2 * budget:
        nxt = min(chunk_max, max(2, it))
        if c > 1 and first > 0 and last < first and budget > 0:
            rate = math.log(first / last) / float(c - 1)
            away = math.log(last / budget) / rate
            nxt = max(1, int(math.ceil(away))) if away <= 8.0 else int(min(float(chunk_max), away / 2.0))
        lg = int(min(float(chunk_max), math.log2(last / budget))) if budget > 0 else chunk_max
        nxt = max(lg, min(nxt, max(2, it // 2)))
    return nxt


def _chunk_rows(T):
    values = [T(v) for v in (0.0, 1e-3, 0.7, 1.0, 1.9, 2.0, 2.1, 3.3, 17.0, 1e3, 1e6, 1e30)]
    rows = []
    for budget in (T(0.0), T(1e-4), T(1.0), T(2.5)):
        for first in values:
            for last in values:
                for c, it in ((1, 1), (2, 3), (5, 10), (64, 64), (64, 200), (7, 2)):
                    rows.append((float(first), float(last), float(budget), c, it))
    return rows + _chunk_rows_nonfinite(T)


def _chunk_rows_nonfinite(T):
    """first / last sums of the non-finite chunks (and every pairing of NaN, +Inf and finite values)"""
    pairs = {(sums[0], sums[-1], len(sums)) for _, sums in NONFINITE_CHUNKS}
    pairs |= {(a, b, c) for a in (NAN, INF, 0.0, 3.0, 1e30) for b in (NAN, INF, 0.0, 3.0, 1e30) for c in (1, 2, 64)
              if a != a or b != b or INF in (a, b)}
    rows = []
    for first, last, c in sorted(pairs, key=repr):
        for budget in (0.0, 1e-4, 1.0):
            for it in (c, 3 * c, 200):
                rows.append((float(T(first)), float(T(last)), float(T(budget)), c, it))
    return rows


# ---- speculate_stop_rule ------------------------------------------------------------------------------------------
def _speculate(T, maxiter, budget, sums):
    """Today's loop (speculate_stop_rule of lasso_hip.hip, f64::solve of gemm_f64.hip), transcribed: chunk, save,
    iterate, read, first hit, restore, replay.  Returns the event log and the result line the program prints."""
    log = []
    state = {"pos": 0, "saved": 0, "t": 1.0}
    slots = [None] * CHUNK_MAX

    def iterate(slot):
        log.append("iterate %d %d %s" % (-1 if slot is None else slot, state["pos"], _bits(f64(state["t"]))))
        state["t"] = (1.0 + math.sqrt(1.0 + 4.0 * state["t"] * state["t"])) / 2.0
        if slot is not None:
            slots[slot] = sums[state["pos"]]
        state["pos"] += 1

    last = T(np.nan)
    it, chunk = 0, 1
    while it < maxiter:
        c = min(chunk, maxiter - it)
        t_head = state["t"]
        if c > 1:
            state["saved"] = state["pos"]
            log.append("save")
        for j in range(c):
            iterate(j)
        log.append("flush")
        log.append("read %d" % c)
        deltas = slots[:c]
        hit = next((j for j in range(c) if deltas[j] <= budget), -1)
        if hit < 0:
            it += c
            last = deltas[c - 1]
            chunk = _next_stop_chunk(deltas[0], last, budget, c, it, CHUNK_MAX)
            continue
        last = deltas[hit]
        if hit < c - 1:
            state["pos"] = state["saved"]
            log.append("restore")
            state["t"] = t_head
            for j in range(hit + 1):
                iterate(None)
            log.append("flush")
        it += hit + 1
        break
    log.append("spec %d %s %d %s" % (it, _bits(T(last)), state["pos"], _bits(f64(state["t"]))))
    return log


def _spec_scripts(T):
    """(name, maxiter, budget, sums): sums[i] is iteration i's; all values of T"""
    b = T(1.0)
    up = np.nextafter(b, T(2.0))
    decay = [T(200.0) * T(0.8) ** i for i in range(80)]            # crosses 1 at iteration 24

    def with_stop(at, value=T(0.5)):
        s = list(decay)
        s[at] = value
        return s
    flat = [T(100.0) - T(i) * T(0.01) for i in range(300)]
    scripts = [
        ("no stop within maxiter", 20, b, decay),
        ("no stop, many chunks", 150, T(1e-3), flat),
        ("stop at iteration 1", 50, b, [T(0.25)] + decay),
        ("maxiter below the first chunks", 2, b, decay),
        ("maxiter 1", 1, b, decay),
        ("decay to the stop", 80, b, decay),
        ("sum equal to the budget stops", 80, b, with_stop(9, b)),
        ("sum one ulp above the budget does not", 80, b, with_stop(9, up)),
    ]
    # a stop at every place of the early chunks: their last iteration (no restore) and strictly inside (restore + replay)
    scripts += [("stop at iteration %d" % (at + 1), 80, b, with_stop(at)) for at in range(1, 24)]
    # non-finite sums: never a stop, maxiter iterations
    for maxiter in (1, 2, 12, 70):
        for name, sums in sorted(_nonfinite_chunks(max(maxiter, 2)).items()):
            if "then finite" not in name:           # (finite sums behind them are covered by the scripts above)
                scripts.append(("nonfinite: %s, maxiter %d" % (name, maxiter), maxiter, b, [T(v) for v in sums]))
    return [(name, maxiter, float(T(budget)), [float(T(v)) for v in sums]) for name, maxiter, budget, sums in scripts]


FIRST_BUDGETS = (1.0, 0.0, 1e30)


WORDS = [(7, 0x3F800000, 0, 0), (64, 0x7FC00000, 1, 0), (0, 0, 0, 1), (12, 0x00000001, 5, 9)]


def _script():
    lines = ["budget %d %d %s" % (r, k, _hex(tol)) for r, k, tol in BUDGET_ROWS]
    for budget, sums in _tile_rows():
        lines.append("tile %s %d %s" % (_hex(budget), len(sums), " ".join(_hex(s) for s in sums)))
    for T, tag in ((f32, "f"), (f64, "d")):
        for first, last, budget, c, it in _chunk_rows(T):
            lines.append("chunk %s %s %s %s %d %d" % (tag, _hex(first), _hex(last), _hex(budget), c, it))
    for T, tag in ((f32, "f"), (f64, "d")):
        for _, maxiter, budget, sums in _spec_scripts(T):
            lines.append("spec %s %d %s %d %s" % (tag, maxiter, _hex(budget), len(sums), " ".join(_hex(s) for s in sums)))
    for tag in ("f", "d"):
        for budget in FIRST_BUDGETS:
            for _, sums in NONFINITE_CHUNKS:
                lines.append("first %s %s %d %s" % (tag, _hex(budget), len(sums), " ".join(_hex(s) for s in sums)))
    lines += ["words %d %d %d %d" % w for w in WORDS]
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
    return _build_and_run(tmp_path_factory.mktemp("stoprule_host"), "stoprule_host", []).splitlines()


def _section(printed, tag):
    return [l for l in printed if l.split()[0] == tag]


def test_stop_budget_bit_for_bit(printed):
    got, want = _section(printed, "budget"), _budget_expected()
    assert got == want
    for (r, k, tol), line in zip(BUDGET_ROWS, want):            # the Python sites round the same product the same way
        assert _bits(f32(nat.stop_budget(r * k, tol))) == line.split()[1]
    inexact = [(r, k, tol) for r, k, tol in BUDGET_ROWS if float(f32(float(r) * float(k) * tol)) != float(r) * float(k) * tol]
    assert len(inexact) >= 5 and any(r * k > 2 ** 24 for r, k, _ in inexact)
    assert any(tol == 0.0 for _, _, tol in BUDGET_ROWS)


def test_next_tile_chunk_equals_its_python_twin(printed):
    rows = _tile_rows()
    got = [int(l.split()[1]) for l in _section(printed, "tile")]
    want = [parallel._next_tile_chunk(sums, len(sums), budget) for budget, sums in rows]
    assert got == want
    # the constructed rows are what they claim: predicted `left` on either side of 128, guesses of 7, 8, 64 and 65
    lefts = [_left(*rows[i]) for i in range(6)]
    assert 127.5 < lefts[0] < 128 < lefts[1] < 128.5
    assert [int(l) - 6 for l in lefts[2:6]] == [7, 8, 64, 65]
    assert want[:9] == [64, 64, 8, 8, 64, 64, 24, 8, 64]
    assert want[12:20] == [8, 8, 64, 64, 64, 64, 64, 64]
    assert set(want[20:]) >= {8, 64} and len(set(want[20:])) > 10     # the seeded rows spread over the range
    # non-finite sums: the twins agree (asserted above, row for row), stay in [1, 64], and a chunk with a NaN anywhere --
    # in front, where Python's max() alone keeps it, or behind, where std::max alone never takes it -- is followed by a
    # full one: no stop is coming
    nf_rows = _tile_rows_nonfinite()
    nf_got = got[len(rows) - len(nf_rows):]
    assert rows[len(rows) - len(nf_rows):] == nf_rows and all(1 <= v <= CHUNK_MAX for v in got)
    for (budget, sums), v in zip(nf_rows, nf_got):
        if any(s != s for s in sums):
            assert v == CHUNK_MAX, (budget, sums, v)
    assert {8, 64} <= set(nf_got)                                      # (+Inf then finite: a steep decay, short chunks)


@pytest.mark.parametrize("T,tag", [(f32, "f"), (f64, "d")])
def test_next_stop_chunk_equals_its_port(printed, T, tag):
    rows = _chunk_rows(T)
    lines = _section(printed, "chunk")
    got = [int(l.split()[1]) for l in (lines[:len(rows)] if T is f32 else lines[len(rows):])]
    want = [_next_stop_chunk(first, last, budget, c, it, CHUNK_MAX) for first, last, budget, c, it in rows]
    assert len(got) == len(want) and got == want
    assert set(want) >= {1, 2, 64} and len(set(want)) > 8 and min(want) >= 1 and max(want) <= CHUNK_MAX
    nf_rows = _chunk_rows_nonfinite(T)
    for (first, last, budget, c, it), v in zip(nf_rows, got[len(rows) - len(nf_rows):]):
        assert 1 <= v <= CHUNK_MAX
        if last != last:
            assert v == 1, (first, last, budget, c, it)              # a NaN last sum: the reference's own cadence
    assert len(nf_rows) > 100


@pytest.mark.parametrize("tag", ["f", "d"])
def test_first_stop_on_nonfinite_sums(printed, tag):
    """ista.py:93: NaN <= budget is False and +Inf <= budget is False for every finite budget -- no stop in a chunk of
    such sums; a finite sum among them stops like any other"""
    lines = [int(l.split()[1]) for l in _section(printed, "first")]
    per = len(FIRST_BUDGETS) * len(NONFINITE_CHUNKS)
    assert len(lines) == 2 * per
    got = lines[:per] if tag == "f" else lines[per:]
    want = [next((i for i, v in enumerate(sums) if v <= budget), -1) for budget in FIRST_BUDGETS for _, sums in NONFINITE_CHUNKS]
    assert got == want
    for (budget, (name, sums)), v in zip(((b, ns) for b in FIRST_BUDGETS for ns in NONFINITE_CHUNKS), got):
        finite = [i for i, s in enumerate(sums) if s == s and s != INF]
        assert v == (finite[0] if finite and budget == 1e30 else -1), (budget, name)     # (every finite sum is > 1)
    assert any(v > 0 for v in got) and got.count(-1) > len(got) // 2


def _spec_logs(printed):
    """the program's event logs, one list per spec command"""
    logs, cur = [], []
    for l in printed:
        if l.split()[0] in ("save", "iterate", "flush", "read", "restore", "spec"):
            cur.append(l)
            if l.startswith("spec"):
                logs.append(cur)
                cur = []
    assert not cur
    return logs


@pytest.mark.parametrize("T", [f32, f64])
def test_speculate_stop_rule_event_for_event(printed, T):
    scripts = _spec_scripts(T)
    logs = _spec_logs(printed)
    logs = logs[:len(scripts)] if T is f32 else logs[len(scripts):]
    assert len(logs) == len(scripts)
    seen = set()
    for (name, maxiter, budget, sums), got in zip(scripts, logs):
        want = _speculate(T, maxiter, budget, sums)
        assert got == want, name
        it, last = int(got[-1].split()[1]), got[-1].split()[2]
        ref = next((i for i, v in enumerate(sums[:maxiter]) if v <= budget), -1)       # the reference's loop, one by one
        assert it == (ref + 1 if ref >= 0 else maxiter), name
        assert last == _bits(T(sums[it - 1])), name
        assert int(got[-1].split()[3]) == it, name                # the state is the one iteration `it` left behind
        if "restore" in got:
            at = got.index("restore")
            head = got[max(i for i in range(at) if got[i] == "save") + 1].split()     # the chunk's first iterate
            replay = [l.split() for l in got[at + 1:-2]]
            assert replay[0][2:] == head[2:], name                 # from the chunk's head, momentum t back bit for bit
            assert len(replay) == it - int(head[2]), name          # exactly hit + 1 iterates ...
            assert all(r[0] == "iterate" and r[1] == "-1" for r in replay), name      # ... with a null slot
            assert got[-2] == "flush", name
            seen.add("replay")
        elif ref >= 0:
            seen.add("stop at a chunk's end")
        else:
            seen.add("no stop")
        if name.startswith("nonfinite"):
            # exactly maxiter iterations, one `iterate` each (nothing replayed), and the last sum as it came
            assert ref < 0 and it == maxiter and sum(l.startswith("iterate") for l in got) == maxiter, name
            assert "restore" not in got, name
            if sums[maxiter - 1] != sums[maxiter - 1]:
                assert np.isnan(T(sums[maxiter - 1])) and last == _bits(T(np.nan)), name
            chunks = [int(l.split()[1]) for l in got if l.startswith("read")]
            assert all(1 <= ch <= CHUNK_MAX for ch in chunks) and sum(chunks) == maxiter, name
            if all(v != v for v in sums[:maxiter]):
                assert chunks == [1] * maxiter, name                   # one host round trip per iteration: slow, bounded
    assert seen == {"replay", "stop at a chunk's end", "no stop"}
    by_name = {s[0]: l for s, l in zip(scripts, logs)}
    assert by_name["sum equal to the budget stops"][-1].split()[1] == "10"
    assert by_name["sum one ulp above the budget does not"][-1].split()[1] == "25"
    assert by_name["stop at iteration 1"] == ["iterate 0 0 %s" % _bits(f64(1.0)), "flush", "read 1",
                                              by_name["stop at iteration 1"][-1]]
    assert "save" not in by_name["maxiter 1"] and by_name["maxiter 1"][-1].split()[1] == "1"


def test_stop_words(printed):
    want = ["words %d %08x %d %d" % (w0, w1, 1 if w2 else 0, 1 if w3 else 0) for w0, w1, w2, w3 in WORDS]
    assert _section(printed, "words") == want


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path, printed):
    out = _build_and_run(tmp_path, "stoprule_host_san",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    assert out.splitlines() == printed
