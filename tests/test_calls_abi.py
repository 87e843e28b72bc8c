"""Calls and sites of a pileup, without a GPU: the host statements wfa_hip_calls_host / wfa_hip_sites_host against the Python
restatement of the rule (calls_common), on hand-written rows that take every branch and on the tables the ORACLE's op strings of the
corpus give; their refusals; and the conditions on the corpus itself, from the oracle-derived expectation alone."""
import ctypes

import numpy as np
import pytest

from calls_common import REF_COL, expectation, expected_calls, expected_sites, py_calls, py_sites
from pywfa_amd import _native
from pywfa_amd.align import Pileup

BIG = 2**31 - 1
# (counters A C G T other del ins mismatch, reference byte): what the row is there for
HAND = [
    ([3, 3, 0, 0, 0, 0, 0, 0], "C"),          # 0  a tie, the reference among the tied: C
    ([3, 3, 0, 0, 0, 0, 0, 0], "A"),          # 1  the same tie, the other reference: A
    ([0, 3, 3, 0, 0, 0, 0, 0], "A"),          # 2  a tie without the reference: the smallest, C
    ([0, 0, 3, 3, 0, 0, 0, 0], "N"),          # 3  reference N, tied reads: G; a site of reference 4
    ([2, 0, 0, 0, 0, 2, 0, 0], "T"),          # 4  a base ties with `deleted`: A
    ([0, 0, 0, 2, 0, 2, 0, 0], "T"),          # 5  the reference ties with `deleted`: T
    ([3, 0, 0, 0, 0, 0, 0, 0], "A"),          # 6  depth 3 = min_depth - 1 at min_depth 4
    ([4, 0, 0, 0, 0, 0, 0, 0], "A"),          # 7  depth 4 = min_depth
    ([1, 0, 0, 0, 0, 0, 5, 0], "A"),          # 8  below min_depth 4 with many insertions: no call, no flag, no site
    ([4, 0, 0, 0, 0, 0, 2, 0], "A"),          # 9  2 * c6 = depth: no flag
    ([5, 0, 0, 0, 0, 0, 3, 0], "A"),          # 10 2 * c6 = depth + 1: the flag
    ([6, 2, 0, 0, 0, 0, 0, 2], "A"),          # 11 1000 * 2 = 250 * 8 exactly: a site at 250 permille, none at 251
    ([7, 1, 0, 0, 0, 0, 0, 1], "A"),          # 12 1000 * 1 < 250 * 8
    ([1500000000, 600000000, 0, 0, 0, 0, 700000000, 0], "A"),   # 13 near 2^31: 6e11 against 250 * 2.1e9 needs 64 bits
    ([BIG, BIG, 0, 0, 0, 0, BIG, 0], "C"),    # 14 a depth beyond int32 (the row holds its low 32 bits)
    ([8, 0, 0, 0, 0, 0, 5, 0], "A"),          # 15 an ins-only site: alt -1, alt_count 0
    ([8, 0, 0, 0, 0, 0, 0, 0], "a"),          # 16 a lower-case reference byte is `other`: the reads' A is the alternative
    ([0, 0, 0, 0, 6, 0, 0, 0], "N"),          # 17 reads and reference both `other`: no alternative at all
    ([0, 0, 0, 0, 0, 6, 0, 0], "G"),          # 18 deleted by every read: call 5, alt 5
    ([0, 0, 0, 0, 0, 0, 4, 0], "G"),          # 19 depth 0 with insertion counts: nothing
    ([2, 2, 2, 2, 2, 2, 7, 0], "x"),          # 20 everything tied over another byte; the flag
]
COUNTS = np.array([c for c, _ in HAND], np.int32)
REF = "".join(b for _, b in HAND).encode()
PARAMS = [(1, 250), (4, 250), (4, 251), (1, 500), (1, 1000), (1, 1), (BIG, 500)]


def sites_raw(counts, ref, seq, start, min_depth, permille, cap, fill=-7):
    """wfa_hip_sites_host on a prefilled rows array of `cap` rows: (rc, count, rows)."""
    counts = np.ascontiguousarray(counts, np.int32)
    refa = np.frombuffer(ref, np.uint8)
    rows = np.full((cap, 8), fill, np.int32)
    count = ctypes.c_int64(-1)
    rc = _native.lib().wfa_hip_sites_host(counts.ctypes.data if counts.size else None, refa.ctypes.data if refa.size else None, len(counts),
                                          seq, start, min_depth, permille, cap, ctypes.byref(count), rows.ctypes.data if cap else None)
    return rc, count.value, rows


def test_python_rule_on_the_hand_rows():
    """The restatement itself, pinned to values worked out by hand from the header's text."""
    assert py_calls(COUNTS, REF, 4).tolist() == [1, 0, 1, 2, 0, 3, 6, 0, 6, 0, 8, 0, 0, 0, 1, 8, 0, 4, 5, 6, 12]
    assert py_calls(COUNTS, REF, 1)[[6, 8, 19]].tolist() == [0, 8, 6]
    rows = py_sites(COUNTS, REF, 3, 100, 4, 250)
    by_pos = {int(r[1]) - 100: r.tolist() for r in rows}
    assert sorted(by_pos) == [0, 1, 2, 3, 4, 5, 9, 10, 11, 13, 14, 15, 16, 18, 20]
    assert by_pos[0] == [3, 100, 1, 0, 6, 3, 3, 0] and by_pos[2] == [3, 102, 0, 1, 6, 0, 3, 0]
    assert by_pos[3] == [3, 103, 4, 2, 6, 0, 3, 0] and by_pos[5] == [3, 105, 3, 5, 4, 2, 2, 0]
    assert by_pos[10] == [3, 110, 0, -1, 5, 5, 0, 3] and by_pos[11] == [3, 111, 0, 1, 8, 6, 2, 0]
    assert by_pos[13] == [3, 113, 0, 1, 2100000000, 1500000000, 600000000, 700000000]
    assert by_pos[14] == [3, 114, 1, 0, -2, BIG, BIG, BIG]
    assert by_pos[15] == [3, 115, 0, -1, 8, 8, 0, 5] and by_pos[16] == [3, 116, 4, 0, 8, 0, 8, 0]
    assert by_pos[18] == [3, 118, 2, 5, 6, 0, 6, 0] and by_pos[20] == [3, 120, 4, -1, 12, 2, 0, 7]
    assert 11 not in {int(r[1]) - 100 for r in py_sites(COUNTS, REF, 3, 100, 4, 251)}
    assert 13 not in {int(r[1]) - 100 for r in py_sites(COUNTS, REF, 3, 100, 4, 500)}
    assert 17 not in by_pos and len(py_sites(COUNTS, REF, 0, 0, BIG, 500)) == 1      # (only the row whose depth passes 2^31 - 1)


@pytest.mark.parametrize("min_depth,permille", PARAMS)
def test_host_statements_on_the_hand_rows(min_depth, permille):
    assert np.array_equal(_native.calls_host(COUNTS, REF, min_depth), py_calls(COUNTS, REF, min_depth))
    want = py_sites(COUNTS, REF, 3, 100, min_depth, permille)
    count, rows = _native.sites_host(COUNTS, REF, 3, 100, min_depth, permille)
    assert count == len(want) and rows.dtype == np.int32 and np.array_equal(rows, want)


def test_host_sites_capacity():
    want = py_sites(COUNTS, REF, 3, 100, 1, 250)
    n = len(want)
    assert n >= 6
    for cap in (0, 1, n - 1, n, n + 5):
        rc, count, rows = sites_raw(COUNTS, REF, 3, 100, 1, 250, cap)
        k = min(n, cap)
        assert rc == _native.OK and count == n, cap
        assert np.array_equal(rows[:k], want[:k]) and (rows[k:] == -7).all(), cap
    # an empty range
    rc, count, rows = sites_raw(COUNTS[:0], b"", 0, 0, 1, 500, 4)
    assert rc == _native.OK and count == 0 and (rows == -7).all()
    assert _native.calls_host(COUNTS[:0], b"", 1).shape == (0,)


def test_host_statements_on_the_corpus_tables():
    """Every row of the oracle-derived tables, every parameter pair of the GPU tests."""
    e = expectation()
    for md in (1, 8):
        for j, (t, r) in enumerate(zip(e["tables"], e["refs"])):
            assert np.array_equal(_native.calls_host(t, r.encode(), md), expected_calls(md)[j]), (md, j)
        for pm in (200, 500, 1000):
            want = expected_sites(md, pm)
            got = [_native.sites_host(t, r.encode(), j, 0, md, pm)[1] for j, (t, r) in enumerate(zip(e["tables"], e["refs"]))]
            assert np.array_equal(np.concatenate(got), want), (md, pm)
    # a range of one reference, numbered from its start
    t, r = e["tables"][2], e["refs"][2].encode()
    want = expected_sites(1, 500)
    want = want[(want[:, 0] == 2) & (want[:, 1] >= 1001) & (want[:, 1] < 3334)]
    count, rows = _native.sites_host(t[1001:3334], r[1001:3334], 2, 1001, 1, 500)
    assert count == len(want) > 0 and np.array_equal(rows, want)


def test_refusals():
    L = _native.lib()
    out = np.full(len(HAND), 99, np.uint8)
    refa = np.frombuffer(REF, np.uint8)
    for args in ((COUNTS.ctypes.data, refa.ctypes.data, len(HAND), 0, out.ctypes.data), (COUNTS.ctypes.data, refa.ctypes.data, -1, 1, out.ctypes.data),
                 (None, refa.ctypes.data, 2, 1, out.ctypes.data), (COUNTS.ctypes.data, None, 2, 1, out.ctypes.data),
                 (COUNTS.ctypes.data, refa.ctypes.data, 2, 1, None)):
        assert L.wfa_hip_calls_host(*args) == _native.EINVAL and (out == 99).all(), args
    for md, pm, cap in ((0, 500, 4), (1, 0, 4), (1, 1001, 4), (1, 500, -1)):
        rc, count, rows = sites_raw(COUNTS, REF, 0, 0, md, pm, max(cap, 4)) if cap >= 0 else (None, -1, np.full((4, 8), -7))
        if cap < 0:
            cnt = ctypes.c_int64(-1)
            rc = L.wfa_hip_sites_host(COUNTS.ctypes.data, refa.ctypes.data, len(HAND), 0, 0, md, pm, cap, ctypes.byref(cnt), rows.ctypes.data)
            count = cnt.value
        assert rc == _native.EINVAL and count == -1 and (rows == -7).all(), (md, pm, cap)
    cnt = ctypes.c_int64(-1)
    assert L.wfa_hip_sites_host(COUNTS.ctypes.data, refa.ctypes.data, len(HAND), 0, 0, 1, 500, 3, ctypes.byref(cnt), None) == _native.EINVAL
    assert L.wfa_hip_sites_host(COUNTS.ctypes.data, refa.ctypes.data, len(HAND), 0, 0, 1, 500, 0, None, None) == _native.EINVAL
    assert cnt.value == -1
    with pytest.raises(ValueError, match="min_depth = 0"):
        _native.calls_host(COUNTS, REF, 0)
    with pytest.raises(ValueError, match="min_permille = 1001"):
        _native.sites_host(COUNTS, REF, 0, 0, 1, 1001)
    with pytest.raises(ValueError, match="one byte per row"):
        _native.calls_host(COUNTS, REF[:-1], 1)


def test_surface_constants():
    assert _native.SITE_COLS == 8 and Pileup.SITE_COLUMNS == ("j", "pos", "ref", "alt", "depth", "ref_count", "alt_count", "ins_count")
    assert Pileup.CALL_CODES == ("A", "C", "G", "T", "other", "del", "no call")


def test_corpus_holds_what_it_is_for():
    """From the oracle-derived expectation alone: the kinds of sites, ties either way, no-calls, insertion flags, and the planted
    homozygous events recovered at min_frac 0.5 where at least 8 reads cover the base."""
    e = expectation()
    refs, tables, cover, planted = e["refs"], e["tables"], e["cover"], e["planted"]
    assert [len(r) for r in refs][4:] == [41, 0] and len(refs[4]) < 64 and (np.asarray(e["o"]["status"]) == 0).all()
    assert 15 <= np.concatenate(cover).mean() <= 25
    rows = expected_sites(1, 500)
    assert ((rows[:, 3] >= 0) & (rows[:, 3] < 4)).any() and (rows[:, 3] == 5).any() and (rows[:, 3] == -1).any() and (rows[:, 2] == 4).any()
    order = rows[:, 0].astype(np.int64) * 2**32 + rows[:, 1]
    assert (np.diff(order) > 0).all()
    calls = np.concatenate(expected_calls(1))
    assert ((calls & 7) == 6).any() and (calls & 8).any() and ((calls & 7) == 5).any()
    assert ((expected_calls(1)[1][2100:2300] & 7) == 6).all()          # the stretch no read covers
    assert len(expected_sites(2**31 - 1, 500)) == 0 and all(((c & 15) == 6).all() for c in expected_calls(2**31 - 1))
    tie_ref = tie_other = 0
    for t, r in zip(tables, refs):
        c = t[:, :6]
        top = c.max(axis=1, keepdims=True) if len(c) else c[:, :1]
        tied = (c == top) & (c.sum(axis=1, keepdims=True) > 0)
        for g in np.flatnonzero(tied.sum(axis=1) > 1):
            if tied[g, REF_COL.get(ord(r[g]), 4)]:
                tie_ref += 1
            else:
                tie_other += 1
    assert tie_ref >= 1 and tie_other >= 1, (tie_ref, tie_other)
    at = {(int(r[0]), int(r[1])): r for r in expected_sites(8, 500)}
    checked = dict(snv=0, dele=0, ins=0)
    for r, p, alt in planted["snv"]:
        if cover[r][p] >= 8:
            assert (r, p) in at and at[(r, p)][3] == alt, ("snv", r, p)
            checked["snv"] += 1
    for r, p, n in planted["dele"]:
        for q in range(p, p + n):
            if cover[r][q] >= 8:
                assert (r, q) in at and at[(r, q)][3] == 5, ("deletion", r, q)
                checked["dele"] += 1
    for r, p, n in planted["ins"]:
        if cover[r][p] >= 8:
            assert (r, p) in at and 2 * at[(r, p)][7] >= at[(r, p)][4], ("insertion", r, p)
            checked["ins"] += 1
    assert all(v >= 1 for v in checked.values()), checked
    assert any((r, p) in {(int(x[0]), int(x[1])) for x in rows} for r, p, _ in planted["under_n"])
