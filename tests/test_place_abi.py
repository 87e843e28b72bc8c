"""Placement of reads, the part that needs no GPU: the C entries are declared, exported and bound; the host statement wfa_hip_place_host
equals the Python restatement of the rule (place_common.py_place) on hand-written edges and on random hit lists full of ties and of
empty and exactly-half-overlapping intervals; its refusals; and the conditions on the corpus of the GPU tests, from the oracle's
results alone."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import loader
from place_common import COLUMNS, INT32_MIN, as_arrays, corpus, hits_of, py_place
from pywfa_amd import _native, datagen
from test_windows_gpu import materialise

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
INT32_MAX = 2**31 - 1
ENTRIES = ("wfa_hip_placer_create", "wfa_hip_placer_add", "wfa_hip_placer_add_hits", "wfa_hip_placer_run", "wfa_hip_placer_count",
           "wfa_hip_placer_clear", "wfa_hip_placer_kernel_ms", "wfa_hip_placer_destroy", "wfa_hip_place_host")


def H(*hits):
    """A hit list from tuples (i, j, reverse, score, status, text_start, text_end)."""
    cols = list(zip(*hits)) if hits else [[]] * 7
    return dict(zip(("i", "j", "reverse", "score", "status", "text_start", "text_end"), cols))


def host(hits, nreads, min_score, full_gap):
    a = as_arrays(hits)
    return _native.place_host(nreads, a["i"], a["j"], a["reverse"], a["score"], a["status"], a["text_start"], a["text_end"], min_score, full_gap)


def test_header_binding_and_shim_declare_the_entries():
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    pxd = open(os.path.join(ROOT, "pywfa_amd", "cython_shim", "wfa_hip.pxd")).read()
    L = _native.lib()
    for name in ENTRIES:
        assert name + "(" in txt and name in _native.SYMBOLS and hasattr(L, name) and name + "(" in pxd, name
    assert "#define WFA_HIP_PLACE_COLS 8 " in txt and "typedef struct wfa_hip_placer wfa_hip_placer_t;" in txt
    assert "IS SERVED BY ONE WAVE" in raw and "2 * ov >= min(te_h - ts_h, te_p - ts_p)" in raw
    assert _native.PLACE_COLUMNS == COLUMNS and _native.PLACE_COLS == 8 and L.wfa_hip_abi_version() == 4
    assert L.wfa_hip_placer_run.argtypes == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]


# (name, hits, nreads, min_score, full_gap, rows by hand, flags by hand)
NONE = [-1, INT32_MIN, INT32_MIN, 0, 0, 0, 0, 0]
EDGES = [
    ("no hits", H(), 2, INT32_MIN, 24, [NONE, NONE], []),
    ("all ineligible: a status, a score below min_score", H((0, 0, 0, -4, 1, 0, 100), (0, 0, 0, -9, 0, 0, 100)), 1, -8, 24, [NONE], [0, 0]),
    ("one hit", H((1, 2, 1, -12, 0, 30, 180)), 2, INT32_MIN, 24, [NONE, [0, -12, INT32_MIN, 60, 1, 0, 30, 180]], [3]),
    ("a tie broken by the hit number; the loser is a runner-up that ties",
     H((0, 0, 0, -8, 0, 500, 650), (0, 0, 0, -8, 0, 0, 150)), 1, INT32_MIN, 24, [[0, -8, -8, 0, 2, 1, 500, 650]], [3, 1]),
    ("2 ov == min to the right of the primary, and one base less",
     H((0, 0, 0, 0, 0, 0, 100), (0, 0, 0, -4, 0, 50, 150), (0, 0, 0, -8, 0, 51, 151)), 1, INT32_MIN, 24,
     [[0, 0, -8, 20, 3, 0, 0, 100]], [3, 2, 1]),
    ("2 ov == min to the left of the primary, and one base less",
     H((0, 0, 0, -8, 0, 49, 149), (0, 0, 0, -4, 0, 50, 150), (0, 0, 0, 0, 0, 100, 200)), 1, INT32_MIN, 24,
     [[2, 0, -8, 20, 3, 0, 100, 200]], [1, 2, 3]),
    ("the shorter interval decides: 10 of 20 bases, 9 of 20; an empty interval inside the primary",
     H((0, 0, 0, 0, 0, 0, 100), (0, 0, 0, -1, 0, 90, 110), (0, 0, 0, -2, 0, 91, 111), (0, 0, 0, -3, 0, 40, 40)), 1, INT32_MIN, 1,
     [[0, 0, -2, 60, 4, 0, 0, 100]], [3, 2, 1, 1]),
    ("another strand, another text at the same place",
     H((0, 1, 0, -4, 0, 10, 160), (0, 1, 1, -6, 0, 10, 160), (0, 2, 0, -7, 0, 10, 160)), 1, INT32_MIN, 4, [[0, -4, -6, 30, 3, 0, 10, 160]], [3, 1, 1]),
    ("full_gap - 1 behind", H((0, 0, 0, -10, 0, 0, 9), (0, 0, 0, -33, 0, 50, 59)), 1, INT32_MIN, 24, [[0, -10, -33, 57, 2, 0, 0, 9]], [3, 1]),
    ("full_gap behind", H((0, 0, 0, -10, 0, 0, 9), (0, 0, 0, -34, 0, 50, 59)), 1, INT32_MIN, 24, [[0, -10, -34, 60, 2, 0, 0, 9]], [3, 1]),
    ("full_gap + 1 behind", H((0, 0, 0, -10, 0, 0, 9), (0, 0, 0, -35, 0, 50, 59)), 1, INT32_MIN, 24, [[0, -10, -35, 60, 2, 0, 0, 9]], [3, 1]),
    ("a runner-up whose score is INT32_MIN is still a runner-up",
     H((0, 0, 0, INT32_MIN + 5, 0, 0, 9), (0, 1, 0, INT32_MIN, 0, 0, 9)), 1, INT32_MIN, 24, [[0, INT32_MIN + 5, INT32_MIN, 12, 2, 0, 0, 9]], [3, 1]),
    ("the extremes: 2 ov and 60 (score - second) need 64 bits",
     H((0, 0, 0, INT32_MAX, 0, 0, INT32_MAX), (0, 0, 0, INT32_MIN, 0, 1, INT32_MAX), (0, 1, 0, INT32_MIN, 0, 0, INT32_MAX)), 1, INT32_MIN,
     INT32_MAX, [[0, INT32_MAX, INT32_MIN, 60, 3, 0, 0, INT32_MAX]], [3, 2, 1]),
    ("the same under a gap no score difference reaches",
     H((0, 0, 0, 1000, 0, 0, 5), (0, 1, 0, 999, 0, 0, 5)), 1, INT32_MIN, INT32_MAX, [[0, 1000, 999, 0, 2, 0, 0, 5]], [3, 1]),
    ("min_score takes the best hit's rival away; reads interleaved",
     H((1, 0, 0, -4, 0, 0, 9), (0, 0, 0, -5, 0, 0, 9), (1, 1, 0, -6, 0, 0, 9), (0, 1, 0, -5, 2, 0, 9)), 2, -5, 24,
     [[1, -5, INT32_MIN, 60, 1, 0, 0, 9], [0, -4, INT32_MIN, 60, 1, 0, 0, 9]], [3, 3, 0, 0]),
]


@pytest.mark.parametrize("case", EDGES, ids=[e[0] for e in EDGES])
def test_edges_by_hand(case):
    """The restatement and the host statement, each against values worked out by hand from the header's text."""
    _, hits, nreads, min_score, full_gap, rows, flags = case
    want = np.array(rows, np.int64).reshape(nreads, 8)
    for what, (r, f) in (("python", py_place(hits, nreads, min_score, full_gap)), ("host", host(hits, nreads, min_score, full_gap))):
        assert r.dtype == np.int32 and r.shape == (nreads, 8) and f.dtype == np.uint8, what
        assert np.array_equal(r, want), (what, r.tolist())
        assert f.tolist() == flags, (what, f.tolist())


def random_hits(rng):
    nreads = int(rng.integers(1, 7))
    n = int(rng.integers(0, 26))
    ts = 5 * rng.integers(0, 9, n)
    ln = rng.choice([0, 10, 20, 20], n)
    return nreads, dict(i=rng.integers(0, nreads, n), j=rng.integers(0, 2, n), reverse=rng.integers(0, 2, n), score=-rng.integers(0, 4, n),
                        status=(rng.random(n) < 0.15).astype(np.int32) * rng.integers(1, 3, n), text_start=ts, text_end=ts + ln)


def test_host_statement_equals_the_restatement_on_random_lists():
    rng = np.random.default_rng(2024)
    seen = {"ties": 0, "same": 0, "none": 0, "mid": 0, "half": 0}
    for _ in range(2000):
        nreads, hits = random_hits(rng)
        min_score = int(rng.choice([INT32_MIN, -2, -1]))
        full_gap = int(rng.choice([1, 2, 3, 24]))
        want = py_place(hits, nreads, min_score, full_gap)
        got = host(hits, nreads, min_score, full_gap)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (hits, min_score, full_gap, got, want)
        rows, flags = want
        seen["ties"] += int((rows[:, 5] > 0).sum())
        seen["same"] += int((flags == 2).sum())
        seen["none"] += int((rows[:, 0] < 0).sum())
        seen["mid"] += int(((rows[:, 3] > 0) & (rows[:, 3] < 60)).sum())
        for r in np.flatnonzero(rows[:, 0] >= 0):        # a hit whose overlap with its read's primary is exactly half of the shorter
            p = rows[r, 0]
            for h in np.flatnonzero((np.asarray(hits["i"]) == r) & (flags > 0) & (np.arange(len(flags)) != p)):
                ov = min(hits["text_end"][h], hits["text_end"][p]) - max(hits["text_start"][h], hits["text_start"][p])
                seen["half"] += int(ov > 0 and 2 * ov == min(hits["text_end"][h] - hits["text_start"][h], hits["text_end"][p] - hits["text_start"][p]))
    assert all(v >= 100 for v in seen.values()), seen


def test_reverse_may_be_left_out():
    hits = H((0, 0, 0, -4, 0, 0, 100), (0, 0, 0, -6, 0, 10, 110))
    rows, flags = _native.place_host(1, hits["i"], hits["j"], None, hits["score"], hits["status"], hits["text_start"], hits["text_end"], INT32_MIN, 24)
    assert rows.tolist() == [[0, -4, INT32_MIN, 60, 2, 0, 0, 100]] and flags.tolist() == [3, 2]


def test_refusals():
    ok = [(0, 0, 0, -4, 0, 0, 100), (1, 0, 0, -4, 0, 0, 100), (2, 1, 1, -4, 0, 5, 100)]

    def bad(pos, **change):
        rows = [list(h) for h in ok]
        for k, v in change.items():
            rows[pos]["i j reverse score status text_start text_end".split().index(k)] = v
        return H(*rows)

    for hits, full_gap, msg in (
            (bad(2, i=3), 24, r"read index out of range at position 2 of the hit list: i = 3 over 3 reads"),
            (bad(1, i=-1), 24, r"position 1 of the hit list: i = -1 over 3 reads"),
            (bad(1, j=-2), 24, r"negative text index at position 1 of the hit list: j = -2"),
            (bad(0, text_start=-7), 24, r"negative text start at position 0 of the hit list: text_start = -7"),
            (bad(2, text_end=4), 24, r"text_end below text_start at position 2 of the hit list: \[5, 4\)"),
            (H(*ok), 0, r"full_gap = 0 is out of range \(at least 1\)"),
            (H(*ok), -3, r"full_gap = -3 is out of range")):
        with pytest.raises(ValueError, match=msg):
            host(hits, 3, INT32_MIN, full_gap)
    with pytest.raises(ValueError, match="one value per hit"):
        _native.place_host(3, [0, 1], [0], None, [0, 0], [0, 0], [0, 0], [1, 1])
    # straight at the C entry: missing arrays, negative counts, a list longer than a hit number can be; nothing is written
    L = _native.lib()
    a = as_arrays(H(*ok))
    rows = np.full((3, 8), 7, np.int32)
    flags = np.full(3, 9, np.uint8)
    msg = ctypes.create_string_buffer(256)
    ptr = {k: (v.ctypes.data if v is not None else None) for k, v in a.items()}

    def call(nreads=3, nhits=3, rows_p=rows.ctypes.data, full_gap=24, **drop):
        p = dict(ptr, **drop)
        return L.wfa_hip_place_host(nreads, nhits, p["i"], p["j"], p["reverse"], p["score"], p["status"], p["text_start"], p["text_end"],
                                    INT32_MIN, full_gap, rows_p, flags.ctypes.data, msg, 256)

    for name in ("i", "j", "score", "status", "text_start", "text_end"):
        assert call(**{name: None}) == _native.EINVAL and b"missing" in msg.value, name
    assert call(rows_p=None) == _native.EINVAL and b"missing" in msg.value
    assert call(nreads=-1) == _native.EINVAL and call(nhits=-1) == _native.EINVAL
    assert call(nhits=2**31) == _native.EINVAL and b"more than 2^31 - 1" in msg.value
    assert call(full_gap=0) == _native.EINVAL
    assert (rows == 7).all() and (flags == 9).all()
    assert call() == _native.OK and msg.value == b"" and rows[:, 0].tolist() == [0, 1, 2] and flags.tolist() == [3, 3, 3]
    assert L.wfa_hip_place_host(0, 0, None, None, None, None, None, None, None, 0, 1, None, None, None, 0) == _native.OK


KW = dict(span="ends-free", text_begin_free=20, text_end_free=20)
KW_STEPS = dict(KW, max_steps=50)
REFS, READS, W, ORIGIN = corpus()
MIN_SCORE = -24


def oracle_hits(kw, full=True):
    pats, txts = materialise(READS, REFS, W)
    o = loader.run(loader.oracle(), loader.make_config(**dict(kw, scope="full" if full else "score")), datagen.from_strings(pats, txts, upper=True))
    return o, hits_of(o, W, full)


def test_corpus_covers_what_it_should():
    """No GPU: the conditions on the inputs, from the oracle's results."""
    assert len(READS) == 200 and 650 <= len(W["i"]) <= 800 and 0.4 <= W["reverse"].mean() <= 0.6
    assert {len(r) for r in REFS} == {4000, 4200, 3800} and REFS[0][600:900] == REFS[1][2500:2800]
    assert sum(a != b for a, b in zip(REFS[1][800:1100], REFS[2][1500:1800])) == 2
    o, hits = oracle_hits(KW)
    assert (np.asarray(o["status"]) == 0).all()
    gap = 6 * 4
    rows, flags = py_place(hits, len(READS), INT32_MIN, gap)
    mapq = rows[:, 3]
    assert (rows[:, 0] >= 0).all() and (rows[:, 4] >= 3).all()
    assert (mapq == 60).sum() >= 80 and ((mapq == 0) & (rows[:, 5] > 0)).sum() >= 15 and ((mapq > 0) & (mapq < 60)).sum() >= 15, np.bincount(mapq)
    assert (flags == 2).sum() >= 150 and (flags == 1).sum() >= 200 and (flags == 3).sum() == 200
    # the primary of a read from a unique region is one of the two windows over its true locus, which the core covers exactly
    for k, (r, pos, n, _, touches) in enumerate(ORIGIN):
        if not touches:
            assert mapq[k] == 60 and W["j"][rows[k, 0]] == r and (rows[k, 6], rows[k, 7]) == (pos, pos + n), (k, rows[k])
    rows, flags = py_place(hits, len(READS), MIN_SCORE, gap)
    assert 5 <= (rows[:, 0] < 0).sum() <= 100 and (flags == 0).sum() >= 200
    # scope score: the same scores, the windows as intervals
    o2, hits2 = oracle_hits(KW, full=False)
    assert np.array_equal(o2["score"], o["score"]) and (np.asarray(hits2["text_end"]) - np.asarray(hits2["text_start"]) == W["t_len"]).all()
    # a step limit some pairs run into
    o3, _ = oracle_hits(KW_STEPS)
    stopped = int((np.asarray(o3["status"]) != 0).sum())
    assert 100 <= stopped <= len(W["i"]) - 100, stopped
