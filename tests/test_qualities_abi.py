"""Base qualities without a GPU (wfa_hip_ops_pileup_quals, wfa_hip_genotypes_quals_host): the C++ statements of the rule must equal
the NumPy restatement (qual_common) on the corpus, on the edge list and on hand-made op strings; their refusals; the checks Python
makes before anything is uploaded; the new entries in the header, the library, the binding and the shim."""
import ctypes
import os

import numpy as np
import pytest

from qual_common import (COLS, EDGES, GENO_PARAMS, MAX_Q, PARAMS, corpus_case, edge_case, edge_ops, fastq, py_costs, py_genotypes_quals,
                         py_pileup_quals, window_quals)
from pywfa_amd import _native
from pywfa_amd.align import _quality_blob

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FILL = -7


def both(ops, pattern, quals, tlen, mbq, cap):
    """(rows, qrows) of the C++ rule and of the NumPy rule for one pair."""
    got = _native.ops_pileup_quals(ops, pattern, tlen, quals, mbq, cap)
    want = np.zeros((tlen, 8), np.int32), np.zeros((tlen, 8), np.int32)
    py_pileup_quals(ops, pattern, quals, mbq, cap, *want)
    return got, want


@pytest.mark.parametrize("mbq,cap", PARAMS)
@pytest.mark.parametrize("case", [corpus_case, edge_case])
def test_host_rule_equals_the_numpy_rule(case, mbq, cap):
    c = case()
    n = len(c.W["i"])
    step = 1 if n < 100 else 7          # (every seventh pair of the corpus: some 340 op strings of 100 - 200 ops)
    seen = 0
    for q in range(0, n, step):
        assert c.o["status"][q] == 0 or case is corpus_case
        if c.o["status"][q] != 0:
            continue
        (rows, qrows), (wr, wq) = both(c.o["cigars"][q], c.pats[q].encode(), window_quals(c.quals, c.W, q), int(c.W["t_len"][q]), mbq, cap)
        assert rows.dtype == qrows.dtype == np.int32 and np.array_equal(rows, wr) and np.array_equal(qrows, wq), (q, mbq, cap)
        if mbq == 0:
            assert np.array_equal(rows, _native.ops_pileup(c.o["cigars"][q], c.pats[q].encode(), int(c.W["t_len"][q]))), q
        seen += int(wq.sum() > 0)
    assert seen > 0 or mbq == MAX_Q


def test_the_quality_arrays_sit_on_the_edges():
    for case in (corpus_case, edge_case):
        allq = np.concatenate(case().quals)
        assert allq.max() <= MAX_Q and all((allq == e).sum() > 0 for e in EDGES)
        for mbq, cap in PARAMS:
            for v in (mbq, mbq - 1, cap, cap + 1):
                assert v < 0 or v > MAX_Q or (allq == v).any(), (mbq, cap, v)


def test_the_edge_list_is_what_it_says():
    c = edge_case()
    assert (np.asarray(c.o["status"]) == 0).all() and len(c.o["status"]) == 48
    want = [b"M" * n for n in (1, 2, 63, 64, 65, 127, 128, 129, 200)] + [b"M" * 62 + b"DDD" + b"M" * 60, b"M" * 64 + b"I" + b"M" * 60]
    for k, w in enumerate(want):
        assert edge_ops(c, k) == [w] * 4, k
    assert all(o[30:31] == b"X" and b"N" in c.pats[44 + k].encode() for k, o in enumerate(edge_ops(c, 11)))
    assert c.W["reverse"].tolist() == [0, 0, 1, 1] * 12 and c.W["p_start"].tolist() == [0, 7] * 24
    assert all(len(c.reads[q]) == c.W["p_len"][q] + (12 if c.W["p_start"][q] else 0) for q in range(48))


HAND = [
    # (ops, pattern, qualities, tlen, note)
    (b"MIMM", b"ACG", [30, 10, 50], 4, "an I directly after the core's first M: min(Qc(0), Qc(1))"),
    (b"MMDDM", b"ACGTA", [30, 31, 7, 90, 33], 3, "a D run as the last op before the last M: the quality of its FIRST base"),
    (b"XXMIID", b"ACGT", [40, 41, 12, 9], 5, "a pair whose only M is one base: nothing else is in the core"),
    (b"DMXIMD", b"TACGA", [1, 13, 12, 93, 2], 4, "ops in front of and behind the core add nothing"),
    (b"MIIIM", b"AC", [93, 0], 5, "an I run: every I takes the same two neighbours"),
    (b"MDIM", b"ACG", [20, 45, 39], 3, "a D run and an I side by side"),
    (b"MXM", b"ANG", [13, 12, 14], 3, "a letter outside ACGT under column 4"),
    (b"", b"", [], 0, "nothing"),
    (b"XDI", b"AC", [5, 5], 2, "no M: no core"),
]


@pytest.mark.parametrize("mbq,cap", PARAMS + [(40, 13), (14, 39)])
def test_hand_made_op_strings(mbq, cap):
    for ops, pattern, quals, tlen, note in HAND:
        quals = np.array(quals, np.uint8)
        (rows, qrows), (wr, wq) = both(ops, pattern, quals, tlen, mbq, cap)
        assert np.array_equal(rows, wr) and np.array_equal(qrows, wq), (note, mbq, cap, rows, wr, qrows, wq)
        if mbq == 0:
            assert np.array_equal(rows, _native.ops_pileup(ops, pattern, tlen)), note


def test_the_figures_of_the_hand_made_cases():
    """Worked out here from the header, not taken from either implementation."""
    rows, qrows = _native.ops_pileup_quals(b"MIMM", b"ACG", 4, np.array([30, 10, 50], np.uint8), 13, 40)
    assert rows.tolist() == [[1, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1, 0, 0], [0] * 8, [0, 0, 1, 0, 0, 0, 0, 0]]      # C (Q 10) is filtered
    assert qrows[0, 0] == 30 and qrows[1, 5] == 10 and qrows[3, 2] == 40 and qrows.sum() == 80
    rows, qrows = _native.ops_pileup_quals(b"MMDDM", b"ACGTA", 3, np.array([30, 31, 7, 90, 33], np.uint8), 0, 40)
    assert rows[2].tolist() == [1, 0, 0, 0, 0, 0, 1, 0] and qrows[2].tolist() == [33, 0, 0, 0, 0, 0, 7, 0]
    rows, qrows = _native.ops_pileup_quals(b"XXMIID", b"ACGT", 5, np.array([40, 41, 12, 9], np.uint8), 0, 93)
    assert rows.sum() == 1 and rows[2, 2] == 1 and qrows[2, 2] == 12
    rows, qrows = _native.ops_pileup_quals(b"MXM", b"ANG", 3, np.array([13, 12, 14], np.uint8), 13, 1)
    assert rows[:, 4].sum() == 0 and rows[:, 7].sum() == 0 and qrows.sum() == 2                                         # the X (Q 12) adds nothing at all
    with pytest.raises(ValueError):
        _native.ops_pileup_quals(b"MM", b"AC", 1, np.array([1, 1], np.uint8))                                           # outruns its text


def raw_ops(ops, pattern, plen, tlen, quals, mbq, cap, rows, qrows, ops_len=None):
    p = lambda a: None if a is None else a.ctypes.data
    return _native.lib().wfa_hip_ops_pileup_quals(p(ops), len(ops) if ops_len is None else ops_len, p(pattern), plen, tlen, p(quals), mbq, cap,
                                                  p(rows), p(qrows))


def test_ops_refusals_add_nothing():
    ops, pattern = np.frombuffer(b"MXIMDM", np.uint8), np.frombuffer(b"ACGTA", np.uint8)
    quals = np.array([20, 30, 40, 50, 60], np.uint8)
    rows, qrows = np.full((5, 8), FILL, np.int32), np.full((5, 8), FILL, np.int32)
    ok = dict(ops=ops, pattern=pattern, plen=5, tlen=5, quals=quals, mbq=13, cap=40, rows=rows, qrows=qrows, ops_len=None)
    over = quals.copy()
    over[3] = 94
    bad = [dict(mbq=-1), dict(mbq=94), dict(cap=0), dict(cap=94), dict(quals=over), dict(quals=None), dict(pattern=None), dict(ops=None, ops_len=6),
           dict(rows=None), dict(qrows=None), dict(plen=4), dict(tlen=3), dict(plen=-1), dict(tlen=-1), dict(ops_len=-1)]
    for b in bad:
        kw = dict(ok, **b)
        ops_arg = kw["ops"] if kw["ops"] is not None else ops
        rc = _native.lib().wfa_hip_ops_pileup_quals(None if kw["ops"] is None else ops_arg.ctypes.data, 6 if kw["ops_len"] is None else kw["ops_len"],
                                                    None if kw["pattern"] is None else kw["pattern"].ctypes.data, kw["plen"], kw["tlen"],
                                                    None if kw["quals"] is None else kw["quals"].ctypes.data, kw["mbq"], kw["cap"],
                                                    None if kw["rows"] is None else kw["rows"].ctypes.data,
                                                    None if kw["qrows"] is None else kw["qrows"].ctypes.data)
        assert rc == _native.EINVAL and (rows == FILL).all() and (qrows == FILL).all(), b
    assert raw_ops(ops, pattern, 5, 5, quals, 13, 40, rows, qrows) == _native.OK and (rows != FILL).any()
    for kw in (dict(min_base_quality=94), dict(quality_cap=0)):
        with pytest.raises(ValueError, match="wfa_hip_ops_pileup_quals: invalid arguments"):
            _native.ops_pileup_quals(b"M", b"A", 1, np.array([1], np.uint8), **kw)
    with pytest.raises(ValueError, match="one value per pattern base"):
        _native.ops_pileup_quals(b"M", b"A", 1, np.array([1, 2], np.uint8))


# ---- genotypes --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("params", GENO_PARAMS)
def test_genotypes_host_equals_the_numpy_rule_on_the_corpus(params):
    c = corpus_case()
    total = 0
    for mbq, cap in PARAMS[:2]:
        counts, qsums, fwd = c.tables(mbq, cap)
        for j, t in enumerate(counts):
            ref = c.refs[j].encode()
            want = py_genotypes_quals(t, qsums[j], fwd[j], ref, j, 0, *params)
            count, rows = _native.genotypes_quals_host(t, qsums[j], ref, fwd[j], j, 0, *params)
            assert rows.dtype == np.int32 and rows.shape == (count, COLS) and np.array_equal(rows, want), (j, params, mbq, cap)
            # the selection, the filter and every column but the four genotype ones are those of the plain genotypes
            _, plain = _native.genotypes_host(t, ref, fwd[j], j, 0, *params)
            assert np.array_equal(rows[:, :8], plain[:, :8]) and np.array_equal(rows[:, 12:], plain[:, 12:])
            total += int((rows[:, 8:12] != plain[:, 8:12]).any(axis=1).sum())
            count, rows = _native.genotypes_quals_host(t[100:900], qsums[j][100:900], ref[100:900], fwd[j][100:900], j, 100, *params)
            assert np.array_equal(rows, want[(want[:, 1] >= 100) & (want[:, 1] < 900)]), (j, params)
            if params[3] == 0:
                count, rows = _native.genotypes_quals_host(t, qsums[j], ref, None, j, 0, *params)
                assert np.array_equal(rows, py_genotypes_quals(t, qsums[j], None, ref, j, 0, *params)) and (rows[:, 12:] == -1).all()
    if params == GENO_PARAMS[1]:
        assert total > 0      # among the many rows of these parameters the qualities change some genotype or its confidence


def row8(a=0, c=0, g=0, t=0, other=0, dele=0, ins=0, mm=0):
    return [a, c, g, t, other, dele, ins, mm]


def test_genotype_costs_by_hand():
    """L0 = qsum[alt], L1 = 3 (R + A), L2 = qsum[r]; the insertion keeps err_q * R for the reads that do not insert."""
    assert py_costs([30, 60, 600]) == (0, 30) and py_costs([60, 60, 340]) == (0, 0) and py_costs([340, 60, 60]) == (1, 0)
    counts = np.array([row8(a=17, c=3), row8(a=3, c=17), row8(c=9), row8(a=4, ins=9), row8(a=10, dele=10)], np.int32)
    qsums = np.array([row8(a=600, c=30), row8(a=6, c=600), row8(c=300), row8(a=100, ins=5), row8(a=61, dele=400)], np.int32)
    count, rows = _native.genotypes_quals_host(counts, qsums, b"AAAAA", None, 0, 0, 1, 100, 20, 0)
    assert count == 5
    # 30 | 60 | 600;  600 | 60 | 6;  300 | 27 | 0;  insertion: 5 | 3 * 9 | 20 * 0;  deletion as alt: 400 | 60 | 61
    assert rows[:, 8:12].tolist() == [[0, 30, -1, -1], [2, 54, -1, -1], [2, 27, -1, -1], [-1, -1, 2, 5], [1, 1, -1, -1]]
    big = 2**31 - 1
    counts = np.array([row8(a=big, c=big)], np.int32)
    qsums = np.array([row8(a=big, c=big - 50)], np.int32)
    count, rows = _native.genotypes_quals_host(counts, qsums, b"A", None, 0, 0, 1, 1, 60, 0)
    assert rows[0, 8:10].tolist() == [0, 50]          # 3 * (R + A) needs 64 bits


def test_genotypes_refusals_write_nothing():
    c = corpus_case()
    counts, qsums, fwd = (np.ascontiguousarray(x[0]) for x in c.tables(0, 40))
    ref = np.frombuffer(c.refs[0].encode(), np.uint8)
    rows = np.full((4, COLS), FILL, np.int32)
    count = ctypes.c_int64(-1)
    p = lambda a: None if a is None else a.ctypes.data
    ok = dict(counts=counts, qsums=qsums, fwd=fwd, ref=ref, n=len(counts), params=(1, 500, 20, 0), cap=4, count=ctypes.byref(count), rows=rows)
    bad = [dict(params=(0, 500, 20, 0)), dict(params=(1, 0, 20, 0)), dict(params=(1, 1001, 20, 0)), dict(params=(1, 500, 0, 0)),
           dict(params=(1, 500, 61, 0)), dict(params=(1, 500, 20, -1)), dict(params=(1, 500, 20, 1), fwd=None), dict(n=-1), dict(cap=-1),
           dict(counts=None), dict(qsums=None), dict(ref=None), dict(count=None), dict(rows=None)]
    call = lambda kw: _native.lib().wfa_hip_genotypes_quals_host(p(kw["counts"]), p(kw["qsums"]), p(kw["fwd"]), p(kw["ref"]), kw["n"], 0, 0,
                                                                 *kw["params"], kw["cap"], kw["count"], p(kw["rows"]))
    for b in bad:
        assert call(dict(ok, **b)) == _native.EINVAL and (rows == FILL).all() and count.value == -1, b
    assert call(ok) == _native.OK and count.value > 4 and (rows != FILL).all()
    with pytest.raises(ValueError, match="qsums"):
        _native.genotypes_quals_host(counts, qsums[:-1], ref)
    with pytest.raises(ValueError, match="wfa_hip_genotypes_quals_host: invalid arguments"):
        _native.genotypes_quals_host(counts, qsums, ref, err_q=0)


# ---- Python's own checks, the declarations ----------------------------------------------------------------------------------------

def test_quality_lists_are_checked_before_anything_is_uploaded():
    q = [np.array([0, 40, 93], np.uint8), np.array([7], np.uint8)]
    blob, off, length = _quality_blob([fastq(q[0]), fastq(q[1]).encode()], [3, 1], 33)
    assert blob.tolist() == [0, 40, 93, 7] and off.tolist() == [0, 3] and length.tolist() == [3, 1] and blob.dtype == np.uint8
    assert _quality_blob(q, [3, 1], 64)[0].tolist() == [0, 40, 93, 7]            # raw arrays: the offset plays no part
    assert _quality_blob(["@hI"], [3], 64)[0].tolist() == [0, 40, 9]
    for quals, lengths, offset, pattern in (
            ([fastq(q[0])], [3, 1], 33, "qualities has 1 entries, the reads are 2"),
            ([fastq(q[0]), "II"], [3, 1], 33, r"qualities\[1\] has 2 values, read 1 has 1 bases"),
            (["!\x7f!", "I"], [3, 1], 33, r"qualities\[0\]\[1\] = 94 is out of range \(phred 0 .. 93\)"),
            (["! !", "I"], [3, 1], 33, r"qualities\[0\]\[1\] = -1 is out of range"),
            ([np.array([1, 2, 94], np.uint8), q[1]], [3, 1], 33, r"qualities\[0\]\[2\] = 94 is out of range"),
            ([[1, 2, 3], q[1]], [3, 1], 33, r"qualities\[0\] must be a str, bytes or a one-dimensional uint8 array, got list"),
            ([np.array([1, 2, 3], np.int64), q[1]], [3, 1], 33, r"qualities\[0\] must be a str, bytes or a one-dimensional uint8 array"),
            ("III", [3], 33, "qualities must be a list"),
            ([fastq(q[0]), "I"], [3, 1], 163, "offset = 163 is out of range"),
            ([fastq(q[0]), "I"], [3, 1], 33.0, "offset = 33.0 is out of range")):
        with pytest.raises(ValueError, match=pattern):
            _quality_blob(quals, lengths, offset)


def test_header_binding_and_shim_declare_the_entries():
    raw_h = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    pxd = open(os.path.join(ROOT, "pywfa_amd", "cython_shim", "wfa_hip.pxd")).read()
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in ("wfa_hip_qualset_create", "wfa_hip_qualset_destroy", "wfa_hip_pileup_track_qualities", "wfa_hip_pileup_add_quals",
                 "wfa_hip_pileup_read_quality", "wfa_hip_pileup_genotypes_quals", "wfa_hip_ops_pileup_quals", "wfa_hip_genotypes_quals_host"):
        assert name + "(" in raw_h and name in _native.SYMBOLS and hasattr(L, name) and name + "(" in pxd, name
    assert "#define WFA_HIP_MAX_QUALITY 93" in raw_h and "base qualities" in raw_h and _native.MAX_QUALITY == 93
    assert "Out of scope: quality values" not in raw_h and "multi-base events" in raw_h
    import pywfa_amd
    from pywfa_amd.align import Pileup, WavefrontAligner
    assert pywfa_amd.QualitySet is not None and hasattr(WavefrontAligner, "quality_set") and hasattr(Pileup, "quality_sums")
    for method in ("track_qualities", "add_quals", "read_quality"):
        assert hasattr(_native.Pileup, method)
