"""Pairing of reads, the part that needs no GPU: the C entries are declared, exported and bound; the host statement wfa_hip_pair_host
equals the Python restatement of the rule (pair_common.py_pair) on random hit lists in which every clause occurs and on hand-written
edges, each against a row worked out by hand from the header's text; its refusals, with the outputs untouched."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import loader
from pair_common import INT32_MAX, INT32_MIN, PAIR_COLUMNS, as_hit_arrays, pair_corpus, py_pair, random_case
from place_common import hits_of
from pywfa_amd import _native, datagen
from test_windows_gpu import materialise

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
MIN, MAX = INT32_MIN, INT32_MAX
ENTRIES = ("wfa_hip_placer_run_pairs", "wfa_hip_pair_host")
PAR = dict(min_score=MIN, full_gap=24, min_insert=0, max_insert=1000, unpaired=0)


def H(*hits):
    """A hit list from tuples (i, j, reverse, score, status, text_start, text_end)."""
    cols = list(zip(*hits)) if hits else [[]] * 7
    return dict(zip(("i", "j", "reverse", "score", "status", "text_start", "text_end"), cols))


def host(hits, nreads, mates, **par):
    a = as_hit_arrays(hits)
    return _native.pair_host(nreads, a["i"], a["j"], a["reverse"], a["score"], a["status"], a["text_start"], a["text_end"], mates, **par)


def test_header_binding_and_shim_declare_the_entries():
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    pxd = open(os.path.join(ROOT, "pywfa_amd", "cython_shim", "wfa_hip.pxd")).read()
    L = _native.lib()
    for name in ENTRIES:
        assert name + "(" in txt and name in _native.SYMBOLS and hasattr(L, name) and name + "(" in pxd, name
    assert "#define WFA_HIP_PAIR_COLS 12 " in txt and "#define WFA_HIP_PAIR_MAX_PAIRINGS 65536 " in txt
    assert raw.index("---- placement:") < raw.index("---- pairing:") < raw.index("---- seed finder:")
    assert "A FRAGMENT IS SERVED BY ONE WAVE" in raw and "pairscore(best) + unpaired >= se(mate1).score + se(mate2).score" in raw
    assert _native.PAIR_COLUMNS == PAIR_COLUMNS and _native.PAIR_COLS == 12 and _native.PAIR_MAX_PAIRINGS == 65536
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert L.wfa_hip_placer_run_pairs.argtypes == [vp] + [i32] * 5 + [i64] + [vp] * 6
    assert L.wfa_hip_pair_host.argtypes == [i64, i64] + [vp] * 7 + [i32] * 5 + [i64] + [vp] * 6 + [ctypes.c_char_p, ctypes.c_size_t]
    assert hasattr(_native.Placer, "run_pairs") and L.wfa_hip_abi_version() == _native.ABI_VERSION


F, R = (0, 0, 0), (1, 0, 1)          # (i, j, reverse) of a forward hit of read 0 and of a reverse hit of read 1, both on text 0
ONE = H(F + (-4, 0, 100, 250), R + (-4, 0, 300, 450))                    # one proper pairing, insert 350
ALONE = [0, 1, 0, MIN, MIN, 0, 60, 60, 0, 0, 0, 0]                       # two placed reads, nothing to join
UNPAIRED = H((0, 0, 0, -4, 0, 100, 250), (0, 1, 0, -20, 0, 100, 250), (1, 1, 1, -6, 0, 300, 450), (1, 0, 0, 0, 0, 5000, 5150))
PLACES = H(F + (-4, 0, 100, 250), F + (-8, 0, 110, 260), R + (-4, 0, 300, 450), F + (-8, 0, 600, 750), R + (-6, 0, 800, 950))
OFF_LOCUS = H(F + (0, 0, 5000, 5150), F + (-10, 0, 100, 250), R + (-4, 0, 300, 450), R + (-4, 0, 700, 850))


def block(n1, n2):
    """n1 hits of read 0 and n2 of read 1, every one of them at one place of its mate; the first of each a point better."""
    return H(*([F + (-1 if h else 0, 0, 100, 250) for h in range(n1)] + [R + (-1 if g else 0, 0, 300, 450) for g in range(n2)]))


# (name, hits, nreads, mates, parameters that differ from PAR, pair rows by hand, pair_flags by hand or None)
EDGES = [
    ("no hits at all", H(), 2, 1, {}, [[-1, -1, 0, MIN, MIN, 0, 0, 0, 0, 0, 0, 0]], []),
    ("a mate without a hit", H(F + (-4, 0, 100, 250)), 2, 1, {}, [[0, -1, 0, MIN, MIN, 0, 60, 0, 0, 0, 0, 0]], [3]),
    ("a mate without an eligible hit", H(F + (-4, 0, 100, 250), R + (-4, 1, 300, 450)), 2, 1, {}, [[0, -1, 0, MIN, MIN, 0, 60, 0, 0, 0, 0, 0]], [3, 0]),
    ("no proper pairing: two texts", H(F + (-4, 0, 100, 250), (1, 1, 1, -8, 0, 300, 450)), 2, 1, {}, [ALONE], [3, 3]),
    ("one proper pairing", ONE, 2, 1, {}, [[0, 1, 1, -8, MIN, 60, 60, 60, 350, 1, 0, 0]], [3, 3]),
    ("the same, mate 1 being the reverse one", H((0, 0, 1, -4, 0, 300, 450), (1, 0, 0, -4, 0, 100, 250)), 2, 1, {},
     [[0, 1, 1, -8, MIN, 60, 60, 60, 350, 1, 0, 0]], [3, 3]),
    ("the same strand", H(F + (-4, 0, 100, 250), (1, 0, 0, -4, 0, 300, 450)), 2, 1, {}, [ALONE], [3, 3]),
    ("wrong order: the reverse hit in front of the forward one", H(F + (-4, 0, 300, 450), R + (-4, 0, 100, 250)), 2, 1, {}, [ALONE], [3, 3]),
    ("wrong order, mate 1 being the reverse one", H((0, 0, 1, -4, 0, 100, 250), (1, 0, 0, -4, 0, 300, 450)), 2, 1, {}, [ALONE], [3, 3]),
    ("the reverse hit starts in front of the forward one", H(F + (-4, 0, 100, 250), R + (-4, 0, 99, 300)), 2, 1, {}, [ALONE], [3, 3]),
    ("the forward hit ends behind the reverse one", H(F + (-4, 0, 100, 400), R + (-4, 0, 200, 399)), 2, 1, {}, [ALONE], [3, 3]),
    ("equal starts and equal ends are in order", H(F + (-4, 0, 100, 250), R + (-4, 0, 100, 250)), 2, 1, {},
     [[0, 1, 1, -8, MIN, 60, 60, 60, 150, 1, 0, 0]], [3, 3]),
    ("an empty interval", H(F + (-4, 0, 100, 100), R + (-4, 0, 300, 450)), 2, 1, {}, [ALONE], [3, 3]),
    ("insert at min_insert and at max_insert", ONE, 2, 1, dict(min_insert=350, max_insert=350), [[0, 1, 1, -8, MIN, 60, 60, 60, 350, 1, 0, 0]], [3, 3]),
    ("insert one below min_insert", ONE, 2, 1, dict(min_insert=351), [ALONE], [3, 3]),
    ("insert one above max_insert", ONE, 2, 1, dict(max_insert=349), [ALONE], [3, 3]),
    ("rejected by unpaired: the best pairing 22 behind the single-end primaries", UNPAIRED, 2, 1, dict(unpaired=21),
     [[0, 3, 0, MIN, MIN, 0, 40, 15, 0, 1, 0, 0]], [3, 1, 1, 3]),
    ("accepted at exactly unpaired = 22; neither chosen hit is at its read's single-end locus", UNPAIRED, 2, 1, dict(unpaired=22),
     [[1, 2, 1, -26, MIN, 60, 60, 60, 350, 1, 0, 0]], [1, 3, 3, 1]),
    ("a second pairing at the same place is no runner-up", H(F + (-4, 0, 100, 250), F + (-8, 0, 110, 260), R + (-4, 0, 300, 450)), 2, 1, {},
     [[0, 2, 1, -8, MIN, 60, 60, 60, 350, 2, 0, 0]], [3, 2, 3]),
    ("runner-ups at other places; mate 1's own mapq is the greater one", PLACES, 2, 1, {}, [[0, 2, 1, -8, -10, 5, 10, 5, 350, 5, 0, 0]], [3, 2, 3, 1, 1]),
    ("a tie at another place; the smallest hit numbers win",
     H(F + (-4, 0, 100, 250), (0, 1, 0, -4, 0, 100, 250), R + (-4, 0, 300, 450), (1, 1, 1, -4, 0, 300, 450)), 2, 1, {},
     [[0, 2, 1, -8, -8, 0, 0, 0, 350, 2, 1, 0]], [3, 1, 3, 1]),
    ("a chosen hit off its read's single-end locus takes the pair mapq, below its own of 25", OFF_LOCUS, 2, 1, dict(unpaired=24),
     [[1, 2, 1, -14, -14, 0, 0, 0, 350, 2, 1, 0]], [1, 3, 3, 1]),
    ("pair scores above INT32_MAX saturate, the mapq does not", H(F + (MAX, 0, 100, 250), R + (MAX, 0, 300, 450), R + (MAX - 1, 0, 700, 850)), 2, 1, {},
     [[0, 1, 1, MAX, MAX, 2, 60, 2, 350, 2, 0, 0]], [3, 3, 1]),
    ("a pair score below INT32_MIN saturates to INT32_MIN + 1", H(F + (MIN, 0, 100, 250), R + (MIN, 0, 300, 450)), 2, 1, {},
     [[0, 1, 1, MIN + 1, MIN, 60, 60, 60, 350, 1, 0, 0]], [3, 3]),
    ("... and so does a runner-up, which INT32_MIN + 1 tells from none", H(F + (MIN, 0, 100, 250), R + (MIN, 0, 300, 450), R + (MIN, 0, 700, 850)), 2, 1, {},
     [[0, 1, 1, MIN + 1, MIN + 1, 0, 60, 0, 350, 2, 1, 0]], [3, 3, 1]),
    ("256 x 256 pairings are joined", block(256, 256), 2, 1, {}, [[0, 256, 1, 0, MIN, 60, 60, 60, 350, 65536, 0, 0]], [3] + [2] * 255 + [3] + [2] * 255),
    ("257 x 256 pairings are not", block(257, 256), 2, 1, {}, [[0, 257, 0, MIN, MIN, 0, 60, 60, 0, 0, 0, 1]], [3] + [2] * 256 + [3] + [2] * 255),
    ("ineligible hits do not count towards the overflow", dict(block(257, 256), status=[0] * 256 + [1] + [0] * 256), 2, 1, {},
     [[0, 257, 1, 0, MIN, 60, 60, 60, 350, 65536, 0, 0]], [3] + [2] * 255 + [0] + [3] + [2] * 255),
    ("no fragment", ONE, 2, 0, {}, np.zeros((0, 12)), [3, 3]),
    ("mates as an array, a read in no fragment", H((2, 0, 0, -4, 0, 100, 250), (0, 0, 1, -4, 0, 300, 450), (1, 0, 1, 0, 0, 300, 450)), 3, [[2, 0]], {},
     [[0, 1, 1, -8, MIN, 60, 60, 60, 350, 1, 0, 0]], [3, 3, 3]),
    ("two fragments, the second first", H((2, 0, 0, -4, 0, 100, 250), (0, 0, 1, -4, 0, 300, 450), (1, 0, 1, 0, 0, 300, 450)), 4, [[3, 1], [0, 2]], {},
     [[-1, 2, 0, MIN, MIN, 0, 0, 60, 0, 0, 0, 0], [1, 0, 1, -8, MIN, 60, 60, 60, 350, 1, 0, 0]], [3, 3, 3]),
]


@pytest.mark.parametrize("case", EDGES, ids=[e[0] for e in EDGES])
def test_edges_by_hand(case):
    """The restatement and the host statement, each against values worked out by hand from the header's text."""
    _, hits, nreads, mates, change, rows, pair_flags = case
    par = dict(PAR, **change)
    want = np.array(rows, np.int64).reshape(-1, 12)
    for what, got in (("python", py_pair(hits, nreads, mates, **par)), ("host", host(hits, nreads, mates, **par))):
        r, f, pr, pf = got
        assert pr.dtype == np.int32 and pr.shape == want.shape and pf.dtype == np.uint8 and pf.shape == f.shape, what
        assert np.array_equal(pr, want), (what, pr.tolist())
        assert pf.tolist() == list(pair_flags), (what, pf.tolist())


def test_host_statement_equals_the_restatement_on_random_lists():
    rng = np.random.default_rng(2025)
    seen = dict(proper=0, improper=0, given_up=0, runner=0, ties=0, mid=0, moved=0, off_locus=0, arrays=0, loose=0, big=0)
    for _ in range(600):
        nreads, hits, mates, par = random_case(rng)
        want = py_pair(hits, nreads, mates, **par)
        got = host(hits, nreads, mates, **par)
        for name, w, g in zip(("rows", "flags", "pair_rows", "pair_flags"), want, got):
            assert w.dtype == g.dtype and w.shape == g.shape and np.array_equal(w, g), (name, hits, mates, par, w.tolist(), g.tolist())
        rows, flags, pr, pf = want
        ok = pr[:, 2] == 1
        seen["proper"] += int(ok.sum())
        seen["improper"] += int((~ok).sum())
        seen["given_up"] += int((~ok & (pr[:, 9] > 0)).sum())               # a proper pairing that `unpaired` did not buy
        seen["runner"] += int((ok & (pr[:, 4] != MIN)).sum())
        seen["ties"] += int((pr[:, 10] > 0).sum())
        seen["mid"] += int(((pr[:, 5] > 0) & (pr[:, 5] < 60)).sum())
        seen["moved"] += int((pf != flags).sum())                           # hits whose flag the pairing changed
        seen["off_locus"] += int((flags[pr[ok, 0]] == 1).sum())              # a chosen hit away from its read's single-end locus
        seen["arrays"] += int(not isinstance(mates, int))
        seen["loose"] += int(nreads > 2 * len(pr))
        seen["big"] += int(len(flags) > 64)
    assert all(v >= 30 for v in seen.values()), sorted(seen.items())


def test_reverse_may_be_left_out_and_then_nothing_pairs():
    r, f, pr, pf = _native.pair_host(2, [0, 1], [0, 0], None, [-4, -4], [0, 0], [100, 300], [250, 450], 1, **PAR)
    assert pr.tolist() == [ALONE] and pf.tolist() == [3, 3] and f.tolist() == [3, 3] and r[:, 0].tolist() == [0, 1]


def test_refusals():
    ok = H((0, 0, 0, -4, 0, 100, 250), (1, 0, 1, -4, 0, 300, 450), (2, 0, 0, -4, 0, 5, 100), (3, 0, 0, -4, 0, 5, 100))
    for hits, mates, change, msg in (
            (H((0, 0, 0, -4, 0, 100, 250), (4, 0, 1, -4, 0, 300, 450)), 2, {}, r"read index out of range at position 1 of the hit list: i = 4 over 4 reads"),
            (H((0, 0, 0, -4, 0, 100, 99)), 2, {}, r"text_end below text_start at position 0 of the hit list: \[100, 99\)"),
            (ok, 2, dict(full_gap=0), r"full_gap = 0 is out of range"),
            (ok, 2, dict(min_insert=-1), r"min_insert = -1, max_insert = 1000 are out of range"),
            (ok, 2, dict(min_insert=500, max_insert=499), r"min_insert = 500, max_insert = 499 are out of range"),
            (ok, 2, dict(unpaired=-1), r"unpaired = -1 is out of range \(at least 0\)"),
            (ok, -1, {}, r"a negative number of fragments \(-1\)"),
            (ok, 3, {}, r"3 interleaved fragments need 6 reads, there are 4"),
            (ok, [[0, 1], [2, 4]], {}, r"mate out of range at fragment 1: mate2 = 4 over 4 reads"),
            (ok, [[-1, 1]], {}, r"mate out of range at fragment 0: mate1 = -1 over 4 reads"),
            (ok, [[0, 1], [3, 3]], {}, r"the mates of fragment 1 are one read: mate1 = mate2 = 3"),
            (ok, [[0, 1], [2, 0]], {}, r"read 0 is named by two fragments, the second time at fragment 1 as mate2"),
            (ok, [[0, 1], [1, 2]], {}, r"read 1 is named by two fragments, the second time at fragment 1 as mate1")):
        with pytest.raises(ValueError, match=msg):
            host(hits, 4, mates, **dict(PAR, **change))
    with pytest.raises(ValueError, match=r"shape \(F, 2\)"):
        host(ok, 4, [0, 1], **PAR)
    # straight at the C entry: one mate array without the other, a missing pair_rows, the refusals above; nothing is written
    L = _native.lib()
    a = as_hit_arrays(ok)
    rows, flags = np.full((4, 8), 7, np.int32), np.full(4, 9, np.uint8)
    pair_rows, pair_flags = np.full((2, 12), 7, np.int32), np.full(4, 9, np.uint8)
    m1, m2 = np.array([2, 0], np.int32), np.array([3, 1], np.int32)
    msg = ctypes.create_string_buffer(256)
    hit_ptrs = [a[k].ctypes.data for k in ("i", "j", "reverse", "score", "status", "text_start", "text_end")]

    def call(nfrag=2, mate1=m1.ctypes.data, mate2=m2.ctypes.data, pair_rows_p=pair_rows.ctypes.data, full_gap=24, min_insert=0, max_insert=1000,
             unpaired=0, nreads=4):
        return L.wfa_hip_pair_host(nreads, 4, *hit_ptrs, MIN, full_gap, min_insert, max_insert, unpaired, nfrag, mate1, mate2,
                                   rows.ctypes.data, flags.ctypes.data, pair_rows_p, pair_flags.ctypes.data, msg, 256)

    assert call(mate2=None) == _native.EINVAL and b"mate2 is missing" in msg.value
    assert call(mate1=None) == _native.EINVAL and b"mate1 is missing" in msg.value
    assert call(pair_rows_p=None) == _native.EINVAL and b"missing" in msg.value
    assert call(nfrag=3, mate1=None, mate2=None) == _native.EINVAL and b"interleaved" in msg.value
    assert call(nfrag=-1) == _native.EINVAL and call(full_gap=0) == _native.EINVAL and call(min_insert=-1) == _native.EINVAL
    assert call(max_insert=-1) == _native.EINVAL and call(unpaired=-5) == _native.EINVAL
    assert call(nreads=3) == _native.EINVAL and b"i = 3 over 3 reads" in msg.value
    m2[1] = 2
    assert call() == _native.EINVAL and b"read 2 is named by two fragments" in msg.value
    m2[1] = 1
    assert (rows == 7).all() and (flags == 9).all() and (pair_rows == 7).all() and (pair_flags == 9).all()
    assert call() == _native.OK and msg.value == b""
    assert pair_rows.tolist() == [[2, 3, 0, MIN, MIN, 0, 60, 60, 0, 0, 0, 0], [0, 1, 1, -8, MIN, 60, 60, 60, 350, 1, 0, 0]]
    assert rows[:, 0].tolist() == [0, 1, 2, 3] and flags.tolist() == [3, 3, 3, 3] and pair_flags.tolist() == [3, 3, 3, 3]
    # the nullable outputs left out; no reads at all
    pair_rows[:] = 7
    assert L.wfa_hip_pair_host(4, 4, *hit_ptrs, MIN, 24, 0, 1000, 0, 2, None, None, None, None, pair_rows.ctypes.data, None, msg, 256) == _native.OK
    assert pair_rows[:, :3].tolist() == [[0, 1, 1], [2, 3, 0]]
    assert L.wfa_hip_pair_host(0, 0, *([None] * 7), 0, 1, 0, 0, 0, 0, None, None, None, None, None, None, None, 0) == _native.OK


def test_corpus_covers_what_it_should():
    """No GPU: the conditions on the paired corpus of the GPU tests, from the oracle's results and the restatement."""
    refs, reads, W, truth = pair_corpus()
    assert len(reads) == 200 and len(truth) == 100 and len(W["i"]) == 420 and refs[0][600:900] == refs[1][2500:2800]
    assert all(200 <= t[2] <= 500 for t in truth) and sum(t[4] for t in truth) == 20 and sum(t[3] for t in truth) == 50
    pats, txts = materialise(reads, refs, W)
    kw = dict(span="ends-free", text_begin_free=20, text_end_free=20)
    for full in (True, False):
        o = loader.run(loader.oracle(), loader.make_config(**dict(kw, scope="full" if full else "score")), datagen.from_strings(pats, txts, upper=True))
        assert (np.asarray(o["status"]) == 0).all()
        rows, flags, pr, pf = py_pair(hits_of(o, W, full), len(reads), len(truth), INT32_MIN, 24, 0, 1000, 24)
        assert (pr[:, 2] == 1).all() and (pr[:, 9] >= 1).all() and not pr[:, 11].any() and (pf != flags).sum() >= 5
        for f, (r, left, outer, flip, repeat, (r1, pos1), (r2, pos2), image) in enumerate(truth):
            h1, h2 = pr[f, 0], pr[f, 1]
            assert (W["i"][h1], W["i"][h2]) == (2 * f, 2 * f + 1) and W["j"][h1] == r1 == W["j"][h2] and abs(int(W["t_start"][h1]) - pos1) <= 10, f
            if full:
                assert pr[f, 8] == outer, (f, pr[f].tolist())
            # a repeat fragment: mate 1 alone cannot tell the copies apart, the fragment can
            assert (rows[2 * f, 3] == 0 and rows[2 * f, 5] == 1 and pr[f, 6] > 0) if repeat else rows[2 * f, 3] == 60, (f, rows[2 * f].tolist())
