"""Duplicate marking, the part that needs no GPU: the C entries are declared, exported and bound; the host statement
wfa_hip_duplicates_host equals the Python restatement of the rule (dup_common.py_duplicates) on random cases in which every clause
occurs and on hand-written edges; the overflow bucket; its refusals, with the outputs untouched; the single-end form.
(tools/dup_host_check.cpp is the stand-alone program for the sanitizers.)"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from dup_common import CLAUSES, DUP_COLUMNS, MAX_BUCKET, as_arrays, py_duplicates, random_dup_case
from pair_common import INT32_MIN
from pywfa_amd import _native

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRIES = ("wfa_hip_placer_duplicates", "wfa_hip_duplicates_host")
PAR = dict(min_score=INT32_MIN, full_gap=24, min_insert=0, max_insert=1000, unpaired=0)
NO, ALONE = [-1, 0, 0, 0], None


def H(*hits):
    """A hit list from tuples (i, j, reverse, score, status, text_start, text_end)."""
    cols = list(zip(*hits)) if hits else [[]] * 7
    return dict(zip(("i", "j", "reverse", "score", "status", "text_start", "text_end"), cols))


def host(hits, nreads, mates, par, text_len):
    return _native.duplicates_host(nreads, *as_arrays(hits), mates, text_len, **par)


def test_header_binding_shim_and_build_declare_the_entries():
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    pxd = open(os.path.join(ROOT, "pywfa_amd", "cython_shim", "wfa_hip.pxd")).read()
    L = _native.lib()
    for name in ENTRIES:
        assert name + "(" in txt and name in _native.SYMBOLS and hasattr(L, name) and name + "(" in pxd, name
    assert "#define WFA_HIP_DUP_COLS 4 " in txt and "#define WFA_HIP_DUP_MAX_BUCKET 4096 " in txt
    assert raw.index("---- rescue:") < raw.index("---- duplicates:") < raw.index("---- seed finder:")
    for phrase in ("PAIR UNIT", "READ UNIT", "REPRESENTATIVE", "BUCKET", "OVERFLOW", "WHAT IT DOES NOT DO"):
        assert phrase in raw[raw.index("---- duplicates:"):raw.index("---- seed finder:")], phrase
    assert _native.DUP_COLUMNS == DUP_COLUMNS and _native.DUP_COLS == 4 and _native.DUP_MAX_BUCKET == MAX_BUCKET == 4096
    assert hasattr(_native.Placer, "duplicates") and callable(_native.duplicates_host)
    assert L.wfa_hip_abi_version() == _native.ABI_VERSION == 4
    build = open(os.path.join(ROOT, "pywfa_amd", "csrc", "build.sh")).read()
    assert "host_dup.cpp" in build and "k_*.hip" in build and os.path.exists(os.path.join(ROOT, "pywfa_amd", "csrc", "k_dup.hip"))
    import pywfa_amd
    for fn in (pywfa_amd.WavefrontAligner.place_pairs, pywfa_amd.WavefrontAligner.place_windows):
        assert inspect.signature(fn).parameters["duplicates"].default is False, fn


def test_host_statement_equals_the_restatement_on_random_cases():
    rng = np.random.default_rng(2027)
    seen = {}
    for k in range(2000):
        nreads, hits, mates, par, text_len = random_dup_case(rng)
        want_r, want_p = py_duplicates(hits, nreads, mates, par, text_len, seen)
        got_r, got_p = host(hits, nreads, mates, par, text_len)
        assert got_r.dtype == got_p.dtype == np.int32 and got_r.shape == want_r.shape and got_p.shape == want_p.shape, k
        assert np.array_equal(got_r, want_r) and np.array_equal(got_p, want_p), (k, mates, par, text_len.tolist(), got_r.tolist(), want_r.tolist(),
                                                                                 got_p.tolist(), want_p.tolist())
    # the generator itself: every clause of the rule occurred somewhere
    assert set(seen) == set(CLAUSES) and all(seen[c] >= 5 for c in CLAUSES), sorted(seen.items())


def frag(f, ts, te, s1, s2, flip=False, j=0):
    """Fragment f = reads (2 f, 2 f + 1): 50-base mates whose forward one starts at ts and whose reverse one ends at te; `flip`: mate
    1 is the reverse one."""
    fwd, rev = (j, 0, s2 if flip else s1, 0, ts, ts + 50), (j, 1, s1 if flip else s2, 0, te - 50, te)
    return [(2 * f + (1 if flip else 0),) + fwd, (2 * f + (0 if flip else 1),) + rev]


def test_edges_by_hand():
    for what in ("python", "host"):
        def run(hits, nreads, mates, text_len=(500,), par=PAR):
            r, p = py_duplicates(hits, nreads, mates, par, list(text_len)) if what == "python" else host(hits, nreads, mates, par, list(text_len))
            return r.tolist(), p.tolist()
        # one fragment alone; its mates are no read units
        assert run(H(*frag(0, 100, 350, -4, -4)), 2, 1) == ([NO, NO], [[0, 1, 0, 0]]), what
        # two copies: the better pair score is the representative, and the mates carry the fragment's dup
        two = H(*(frag(0, 100, 350, -4, -4) + frag(1, 100, 350, 0, -4)))
        assert run(two, 4, 2) == ([[-1, 0, 1, 0]] * 2 + [NO] * 2, [[1, 2, 1, 0], [1, 2, 0, 0]]), what
        # a tie: the smaller fragment number
        tie = H(*(frag(0, 100, 350, -4, 0) + frag(1, 100, 350, 0, -4) + frag(2, 100, 350, -2, -2)))
        assert run(tie, 6, 3) == ([NO] * 2 + [[-1, 0, 1, 0]] * 4, [[0, 3, 0, 0], [0, 3, 1, 0], [0, 3, 1, 0]]), what
        # F1R2 against F2R1 with the same ends; the same start with another end; another text
        for other in (frag(1, 100, 350, 0, 0, flip=True), frag(1, 100, 351, 0, 0), frag(1, 100, 350, 0, 0, j=1)):
            assert run(H(*(frag(0, 100, 350, -4, -4) + other)), 4, 2, (500, 500)) == ([NO] * 4, [[0, 1, 0, 0], [1, 1, 0, 0]]), (what, other)
        # mates as an array, backwards: mate 1 is the reverse one in both fragments, so they group
        assert run(two, 4, [[1, 0], [3, 2]]) == ([[-1, 0, 1, 0]] * 2 + [NO] * 2, [[1, 2, 1, 0], [1, 2, 0, 0]]), what
        # a fragment that lost to its single-end primaries (unpaired = 0) is not proper: its mates are read units
        lost = H((0, 0, 0, 0, 0, 10, 60), (0, 0, 0, -30, 0, 100, 150), (1, 0, 1, -4, 0, 300, 350), (1, 1, 1, 0, 0, 400, 450), (2, 0, 0, -1, 0, 10, 70))
        assert run(lost, 3, 1, (500, 500)) == ([[0, 2, 0, 0], [1, 1, 0, 0], [0, 2, 1, 0]], [NO]), what
        # single-end: forward reads group by their start, whatever their length
        fwd = H((0, 0, 0, -4, 0, 10, 60), (1, 0, 0, -2, 0, 10, 50), (2, 0, 0, 0, 0, 11, 60))
        assert run(fwd, 3, 0) == ([[1, 2, 1, 0], [1, 2, 0, 0], [2, 1, 0, 0]], []), what
        # reverse reads of different lengths group by their last base; a forward read that starts there is another group
        rev = H((0, 0, 1, -4, 0, 10, 60), (1, 0, 1, -4, 0, 20, 60), (2, 0, 0, 0, 0, 59, 99), (3, 0, 1, 0, 0, 10, 61))
        assert run(rev, 4, 0) == ([[0, 2, 0, 0], [0, 2, 1, 0], [2, 1, 0, 0], [3, 1, 0, 0]], []), what
        # a read unit and a pair unit in one bucket are never one group
        mixed = H(*(frag(0, 100, 350, -4, -4) + [(2, 0, 0, 0, 0, 100, 150), (3, 0, 0, -1, 0, 100, 150)]))
        assert run(mixed, 4, 1) == ([NO, NO, [2, 2, 0, 0], [2, 2, 1, 0]], [[0, 1, 0, 0]]), what
        # te == tlen on the reverse strand is inside (p5 = tlen - 1); position 0; ts == tlen is outside: alone, no overflow
        ends = H((0, 0, 1, -4, 0, 450, 500), (1, 0, 1, 0, 0, 470, 500), (2, 0, 0, -4, 0, 0, 50), (3, 0, 0, 0, 0, 0, 20), (4, 0, 0, 0, 0, 500, 550),
                 (5, 0, 0, 0, 0, 500, 550))
        assert run(ends, 6, 0) == ([[1, 2, 1, 0], [1, 2, 0, 0], [3, 2, 1, 0], [3, 2, 0, 0], [4, 1, 0, 0], [5, 1, 0, 0]], []), what
        # a pair unit whose start lies outside its text: alone, and its mates follow it
        out = H(*(frag(0, 600, 850, -4, -4) + frag(1, 600, 850, 0, 0)))
        assert run(out, 4, 2) == ([NO] * 4, [[0, 1, 0, 0], [1, 1, 0, 0]]), what
        # no eligible hit (status, min_score), an empty interval, no hit at all: no units
        none = H((0, 0, 0, -4, 1, 10, 60), (1, 0, 0, -4, 0, 10, 10), (2, 0, 0, -9, 0, 10, 60), (3, 0, 0, -4, 0, 10, 60))
        assert run(none, 5, 0, par=dict(PAR, min_score=-5)) == ([NO, NO, NO, [3, 1, 0, 0], NO], []), what
        # the score is the saturated int32 of the pair row: two fragments far below INT32_MIN + 1 tie, the smaller number wins
        low = H(*(frag(0, 100, 350, INT32_MIN, INT32_MIN) + frag(1, 100, 350, INT32_MIN + 5, INT32_MIN)))
        assert run(low, 4, 2) == ([NO] * 2 + [[-1, 0, 1, 0]] * 2, [[0, 2, 0, 0], [0, 2, 1, 0]]), what
        # nothing at all
        assert run(H(), 0, 0, ()) == ([], []) and run(H(), 3, 1) == ([NO] * 3, [NO]), what


def test_overflow_bucket_4097_units_against_4096():
    """4 096 units in one bucket are resolved — here two groups, forward reads and proper fragments that start at one base — and one
    unit more leaves every unit of the bucket alone with overflow = 1; a unit in the next bucket is untouched."""
    nfrag = 10
    for extra in (0, 1):
        nsingle = MAX_BUCKET - nfrag + extra
        rows = []
        for f in range(nfrag):
            rows += frag(f, 100, 350, -f, 0)
        rows += [(2 * nfrag + r, 0, 0, 0 if r == 7 else -4, 0, 100, 150) for r in range(nsingle)]
        rows.append((2 * nfrag + nsingle, 0, 0, 0, 0, 101, 150))
        nreads = 2 * nfrag + nsingle + 1
        hits = H(*rows)
        want = py_duplicates(hits, nreads, nfrag, PAR, [500])
        got = host(hits, nreads, nfrag, PAR, [500])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), extra
        reads, pairs = got
        assert reads[-1].tolist() == [nreads - 1, 1, 0, 0]
        if extra:
            assert (pairs == np.c_[np.arange(nfrag), np.ones(nfrag), np.zeros(nfrag), np.ones(nfrag)]).all()
            assert (reads[:2 * nfrag] == [-1, 0, 0, 1]).all()
            assert (reads[2 * nfrag:-1] == np.c_[np.arange(2 * nfrag, nreads - 1), np.ones(nsingle), np.zeros(nsingle), np.ones(nsingle)]).all()
        else:
            assert (pairs[:, 0] == 0).all() and (pairs[:, 1] == nfrag).all() and pairs[:, 2].tolist() == [0] + [1] * (nfrag - 1) and not pairs[:, 3].any()
            assert (reads[2 * nfrag:-1, 0] == 2 * nfrag + 7).all() and (reads[2 * nfrag:-1, 1] == nsingle).all() and not reads[:, 3].any()
            assert reads[2 * nfrag:-1, 2].sum() == nsingle - 1 and reads[2:2 * nfrag, 2].all() and not reads[:2, 2].any()


def test_refusals_leave_the_outputs_untouched():
    ok = H(*(frag(0, 100, 350, -4, -4) + [(2, 1, 0, -4, 0, 5, 100)]))

    def call(hits=ok, mates=2, text_len=(500, 300), **change):
        return host(hits, 4, mates, dict(PAR, **change), list(text_len))

    assert call()[1].tolist() == [[0, 1, 0, 0], NO]
    for kw, msg in ((dict(text_len=[500, -3]), r"negative length of text 1: text_len = -3"),
                    (dict(text_len=[500]), r"text index out of range at position 2 of the hit list: j = 1 over 1 texts"),
                    (dict(text_len=[]), r"text index out of range at position 0 of the hit list: j = 0 over 0 texts"),
                    # whatever wfa_hip_pair_host refuses
                    (dict(hits=H((4, 0, 0, -4, 0, 1, 2))), r"read index out of range at position 0 of the hit list: i = 4 over 4 reads"),
                    (dict(hits=H((0, 0, 0, -4, 0, 100, 99))), r"text_end below text_start at position 0"),
                    (dict(full_gap=0), r"full_gap = 0 is out of range"), (dict(min_insert=-1), r"min_insert = -1, max_insert = 1000 are out of range"),
                    (dict(min_insert=1700), r"min_insert = 1700, max_insert = 1000 are out of range"), (dict(unpaired=-1), r"unpaired = -1 is out of range"),
                    (dict(mates=-1), r"a negative number of fragments"), (dict(mates=3), r"3 interleaved fragments need 6 reads, there are 4"),
                    (dict(mates=[[0, 1], [2, 4]]), r"mate out of range at fragment 1"), (dict(mates=[[0, 0]]), r"the mates of fragment 0 are one read"),
                    (dict(mates=[[0, 1], [1, 2]]), r"read 1 is named by two fragments")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    # straight at the C entry: missing pointers and the refusals above; nothing is written
    L = _native.lib()
    arrays = as_arrays(ok)                      # (kept alive behind the pointers)
    ptrs = [a.ctypes.data for a in arrays]
    tlen = np.array([500, 300], np.int32)
    reads, pairs = np.full((4, 4), 7, np.int32), np.full((2, 4), 7, np.int32)
    msg = ctypes.create_string_buffer(256)

    def raw(nfrag=2, ntexts=2, text_len=tlen.ctypes.data, reads_p=reads.ctypes.data, pairs_p=pairs.ctypes.data, max_insert=1000, full_gap=24,
            mate1=None, mate2=None):
        return L.wfa_hip_duplicates_host(4, 3, *ptrs, INT32_MIN, full_gap, 0, max_insert, 0, nfrag, mate1, mate2, ntexts, text_len, reads_p, pairs_p,
                                         msg, 256)

    m = np.array([0, 2], np.int32)
    assert raw(reads_p=None) == _native.EINVAL and b"missing array (read_rows)" in msg.value
    assert raw(pairs_p=None) == _native.EINVAL and b"missing array (pair_rows)" in msg.value
    assert raw(text_len=None) == _native.EINVAL and b"missing array (text_len)" in msg.value
    assert raw(ntexts=-1) == _native.EINVAL and b"a negative number of texts" in msg.value
    assert raw(mate1=m.ctypes.data) == _native.EINVAL and b"mate2 is missing" in msg.value
    for kw in (dict(ntexts=1), dict(nfrag=3), dict(nfrag=-1), dict(max_insert=-1), dict(full_gap=0)):
        assert raw(**kw) == _native.EINVAL and msg.value, kw
    assert (reads == 7).all() and (pairs == 7).all()
    assert raw() == _native.OK and msg.value == b""
    assert pairs.tolist() == [[0, 1, 0, 0], NO] and reads.tolist() == [NO, NO, [2, 1, 0, 0], NO]
    # a message buffer is optional
    assert L.wfa_hip_duplicates_host(4, 3, *ptrs, INT32_MIN, 24, 0, 1000, 0, 2, None, None, 1, tlen.ctypes.data, reads.ctypes.data, pairs.ctypes.data,
                                     None, 0) == _native.EINVAL


def test_single_end_form_nfrag_0():
    hits = H((0, 0, 0, -4, 0, 10, 60), (1, 0, 0, -2, 0, 10, 50), (2, 0, 1, 0, 0, 11, 60), (3, 0, 1, -1, 0, 30, 60))
    want = [[1, 2, 1, 0], [1, 2, 0, 0], [2, 2, 0, 0], [2, 2, 1, 0]]
    for mates in (0, np.zeros((0, 2), np.int32)):   # (both mate arrays NULL, and two empty arrays)
        reads, pairs = host(hits, 4, mates, PAR, [500])
        assert reads.tolist() == want and pairs.shape == (0, 4)
    # straight at the C entry with NULL pair_rows, and with no reads at all
    L = _native.lib()
    arrays = as_arrays(hits)                    # (kept alive behind the pointers)
    ptrs = [a.ctypes.data for a in arrays]
    tlen = np.array([500], np.int32)
    reads = np.full((4, 4), 7, np.int32)
    assert L.wfa_hip_duplicates_host(4, 4, *ptrs, INT32_MIN, 24, 0, 1000, 0, 0, None, None, 1, tlen.ctypes.data, reads.ctypes.data, None, None, 0) == _native.OK
    assert reads.tolist() == want
    assert L.wfa_hip_duplicates_host(0, 0, *([None] * 7), 0, 1, 0, 0, 0, 0, None, None, 0, None, None, None, None, 0) == _native.OK
