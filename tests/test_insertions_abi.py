"""The insertion log of a pileup, without a GPU: the host statements wfa_hip_ops_insertions / wfa_hip_insertions_host against the Python
restatement of the rule (insertions_common), over the corpus and over random op strings, with capacities below, at and above the
counts; their refusals; the new entries in the header, the library, the binding and the shim; and the conditions on the corpus
itself that the GPU tests rely on, from the oracle-derived expectation alone."""
import ctypes
import os
import re

import numpy as np
import pytest

from insertions_common import ASCII, STAGE, expectation, expected_insertions, py_insertions, py_ops_insertions
from pywfa_amd import _native
from pywfa_amd.align import Pileup, WavefrontAligner

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRIES = ("wfa_hip_pileup_track_insertions", "wfa_hip_pileup_insertion_stats", "wfa_hip_pileup_insertions", "wfa_hip_ops_insertions",
           "wfa_hip_insertions_host")
FILL = -7


def ops_raw(ops, pattern, tlen, cap, cols_cap):
    """wfa_hip_ops_insertions on prefilled arrays: (rc, count, recs, cols_count, cols)."""
    o, p = np.frombuffer(bytes(ops), np.uint8), np.frombuffer(bytes(pattern), np.uint8)
    recs, cols = np.full((cap, 3), FILL, np.int32), np.full(cols_cap, 99, np.uint8)
    count, ncols = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = _native.lib().wfa_hip_ops_insertions(o.ctypes.data if o.size else None, o.size, p.ctypes.data if p.size else None, p.size, tlen, cap,
                                              ctypes.byref(count), recs.ctypes.data if cap else None, cols_cap, ctypes.byref(ncols),
                                              cols.ctypes.data if cols_cap else None)
    return rc, count.value, recs, ncols.value, cols


def flat(recs):
    """[(h, n, columns)] as the arrays the host statement writes: recs (n x 3) and the column bytes."""
    rows, cols = [], []
    for h, n, c in recs:
        rows.append((h, n, len(cols)))
        cols += c
    return np.array(rows, np.int32).reshape(-1, 3), np.array(cols, np.uint8)


def check_ops(ops, pattern, tlen):
    want_recs, want_cols = flat(py_ops_insertions(ops, pattern))
    n, nc = len(want_recs), len(want_cols)
    recs, cols = _native.ops_insertions(ops, pattern, tlen)
    assert np.array_equal(recs, want_recs) and np.array_equal(cols, want_cols), (ops, pattern)
    for cap in {0, max(n - 1, 0), n, n + 3}:
        for cols_cap in {0, max(nc - 1, 0), nc, nc + 5}:
            rc, count, recs, ncols, cols = ops_raw(ops, pattern, tlen, cap, cols_cap)
            k = min(cap, n)
            assert rc == _native.OK and count == n and ncols == nc, (cap, cols_cap)
            assert np.array_equal(recs[:k], want_recs[:k]) and (recs[k:] == FILL).all(), (cap, cols_cap)
            fit = 0   # the column bytes of the written records that fit whole
            for h, m, off in want_recs[:k]:
                if off + m <= cols_cap:
                    assert np.array_equal(cols[off:off + m], want_cols[off:off + m]), (cap, cols_cap)
                    fit = off + m
            assert (cols[fit:] == 99).all(), (cap, cols_cap)
    return n


def random_ops(rng):
    """An op string with D runs before, inside and behind its core, and a pattern / text length that fit it (sometimes with room)."""
    parts = []
    for _ in range(int(rng.integers(0, 12))):
        parts.append("MXID"[int(rng.choice(4, p=[0.45, 0.1, 0.15, 0.3]))] * int(rng.integers(1, 5 if rng.random() < 0.9 else 80)))
    ops = "".join(parts).encode()
    plen = sum(1 for c in ops if c in b"MXD") + int(rng.integers(0, 3))
    tlen = sum(1 for c in ops if c in b"MXI") + int(rng.integers(0, 3))
    pattern = "".join(rng.choice(list("ACGTNacgt-"), plen, p=[0.22] * 4 + [0.04, 0.02, 0.02, 0.02, 0.01, 0.01])).encode()
    return ops, pattern, tlen


def test_ops_insertions_on_random_op_strings():
    rng = np.random.default_rng(31)
    seen = sum(check_ops(*random_ops(rng)) for _ in range(1500))
    assert seen > 500          # (the generator does produce runs inside cores)
    # by hand: the D run in front of the first M and the one behind the last M are no records; an X may stand beside a run
    assert py_ops_insertions(b"DDMXDDDIMDMDD", b"ttACGTNaCCgg") == [(2, 3, (2, 3, 4)), (4, 1, (1,))]
    assert check_ops(b"DDMXDDDIMDMDD", b"ttACGTNaCCgg", 5) == 2
    assert check_ops(b"", b"", 0) == 0 and check_ops(b"DDD", b"ACG", 0) == 0 and check_ops(b"IIXDX", b"ACG", 4) == 0


def test_ops_insertions_on_the_corpus():
    e = expectation()
    for q, ops in enumerate(e["o"]["cigars"]):
        recs, cols = _native.ops_insertions(ops, e["pats"][q].encode(), int(e["W"]["t_len"][q]))
        want_recs, want_cols = flat(py_ops_insertions(ops, e["pats"][q].encode()))
        assert np.array_equal(recs, want_recs) and np.array_equal(cols, want_cols), q
    for q in range(0, len(e["pats"]), 97):
        check_ops(e["o"]["cigars"][q], e["pats"][q].encode(), int(e["W"]["t_len"][q]))


def record_arrays(records, lo=0, hi=None, rng=None):
    """The records of the rows [lo, hi) of one reference as the arrays wfa_hip_insertions_host takes, rows relative to lo; shuffled
    when `rng` is given (the rule does not depend on the order)."""
    items = [(g - lo, n, cols) for g, recs in records.items() if g >= lo and (hi is None or g < hi) for n, cols in recs]
    if rng is not None:
        items = [items[k] for k in rng.permutation(len(items))]
    cols = [c for _, _, cs in items for c in cs]
    offs = np.cumsum([0] + [n for _, n, _ in items])[:-1]
    return (np.array([g for g, _, _ in items], np.int64), np.array([n for _, n, _ in items], np.int32), np.array(offs, np.int64),
            np.array(cols, np.uint8))


def letters_of(seqs):
    return np.frombuffer("".join(seqs).encode(), np.uint8)


@pytest.mark.parametrize("min_depth,permille", [(1, 0), (1, 1), (1, 200), (8, 500), (1, 1000), (8, 0)])
def test_insertions_host_on_the_corpus(min_depth, permille):
    e = expectation()
    rng = np.random.default_rng(5)
    for j, t in enumerate(e["tables"]):
        want_rows, want_seqs = py_insertions(t, e["records"][j], j, 0, min_depth, permille)
        for shuffle in (None, rng):
            count, rows, nbases, bases = _native.insertions_host(t, *record_arrays(e["records"][j], rng=shuffle), seq=j, min_depth=min_depth,
                                                                 min_permille=permille)
            assert count == len(want_rows) and rows.dtype == np.int32 and np.array_equal(rows, want_rows), (j, count, len(want_rows))
            assert nbases == sum(map(len, want_seqs)) and np.array_equal(bases, letters_of(want_seqs)), j
    # a range of the stage, numbered from its start; records outside the range are skipped
    t, recs = e["tables"][STAGE], e["records"][STAGE]
    want_rows, want_seqs = py_insertions(t[550:1300], {g - 550: v for g, v in recs.items()}, STAGE, 550, min_depth, permille)
    got = _native.insertions_host(t[550:1300], *record_arrays(recs, 550), seq=STAGE, start=550, min_depth=min_depth, min_permille=permille)
    assert got[0] == len(want_rows) >= 3 and np.array_equal(got[1], want_rows) and np.array_equal(got[3], letters_of(want_seqs))


def test_insertions_host_capacities_and_overflow(monkeypatch):
    e = expectation()
    t, recs = e["tables"][STAGE], record_arrays(e["records"][STAGE])
    want_rows, want_seqs = py_insertions(t, e["records"][STAGE], STAGE, 0, 1, 500)
    n, nb = len(want_rows), sum(map(len, want_seqs))
    assert n >= 6 and nb > 70
    ends = np.cumsum(want_rows[:, 5])
    for cap in (0, 1, n - 1, n, n + 4):
        for bases_cap in (0, 1, int(ends[2]) - 1, int(ends[2]), nb - 1, nb, nb + 9):
            rows, bases = np.full((cap, 8), FILL, np.int32), np.full(bases_cap, 99, np.uint8)
            count, nbases = ctypes.c_int64(-1), ctypes.c_int64(-1)
            rc = _native.lib().wfa_hip_insertions_host(t.ctypes.data, len(t), STAGE, 0, 1, 500, len(recs[0]), *[a.ctypes.data for a in recs],
                                                       len(recs[3]), cap, ctypes.byref(count), rows.ctypes.data if cap else None, bases_cap,
                                                       ctypes.byref(nbases), bases.ctypes.data if bases_cap else None)
            k = min(cap, n)
            fit = max([int(x) for x in ends[:k] if x <= bases_cap], default=0)
            assert rc == _native.OK and count.value == n and nbases.value == nb, (cap, bases_cap)
            assert np.array_equal(rows[:k], want_rows[:k]) and (rows[k:] == FILL).all(), (cap, bases_cap)
            assert np.array_equal(bases[:fit], letters_of(want_seqs)[:fit]) and (bases[fit:] == 99).all(), (cap, bases_cap)
    # the limit, read per call: the rows above it report overflow and zeros, the others are unchanged
    monkeypatch.setenv("WFA_HIP_INS_MAX_READS", "8")
    low_rows, low_seqs = py_insertions(t, e["records"][STAGE], STAGE, 0, 1, 500, max_reads=8)
    assert 0 < low_rows[:, 7].sum() < len(low_rows) and (low_rows[low_rows[:, 7] == 1][:, 4:7] == 0).all()
    count, rows, nbases, bases = _native.insertions_host(t, *recs, seq=STAGE)
    assert np.array_equal(rows, low_rows) and np.array_equal(bases, letters_of(low_seqs))
    monkeypatch.setenv("WFA_HIP_INS_MAX_READS", "0")        # (at least 1)
    assert (_native.insertions_host(t, *recs, seq=STAGE)[1][:, 7] == 1).all()


def test_refusals():
    L = _native.lib()
    assert ops_raw(b"MDM", b"ACG", 2, 4, 4)[0] == _native.OK
    for bad in ((b"MDM", b"AC", 2, 4, 4), (b"MDM", b"ACG", 1, 4, 4), (b"MDM", b"ACG", 2, -1, 4), (b"MDM", b"ACG", 2, 4, -1)):
        rc, count, recs, ncols, cols = ops_raw(*bad[:3], max(bad[3], 0), max(bad[4], 0)) if min(bad[3:]) >= 0 else (None, -1, None, -1, None)
        if rc is None:   # a negative capacity: through the raw entry, with room behind the pointers
            recs, cols = np.full((4, 3), FILL, np.int32), np.full(4, 99, np.uint8)
            c1, c2 = ctypes.c_int64(-1), ctypes.c_int64(-1)
            o, p = np.frombuffer(bad[0], np.uint8), np.frombuffer(bad[1], np.uint8)
            rc = L.wfa_hip_ops_insertions(o.ctypes.data, 3, p.ctypes.data, 3, bad[2], bad[3], ctypes.byref(c1), recs.ctypes.data, bad[4],
                                          ctypes.byref(c2), cols.ctypes.data)
            count, ncols = c1.value, c2.value
        assert rc == _native.EINVAL and count == -1 and ncols == -1 and (recs == FILL).all() and (cols == 99).all(), bad
    o, p = np.frombuffer(b"MDM", np.uint8), np.frombuffer(b"ACG", np.uint8)
    c1, c2 = ctypes.c_int64(-1), ctypes.c_int64(-1)
    recs, cols = np.full((4, 3), FILL, np.int32), np.full(4, 99, np.uint8)
    for args in ((None, 3, p.ctypes.data, 3, 2, 4, ctypes.byref(c1), recs.ctypes.data, 4, ctypes.byref(c2), cols.ctypes.data),
                 (o.ctypes.data, 3, None, 3, 2, 4, ctypes.byref(c1), recs.ctypes.data, 4, ctypes.byref(c2), cols.ctypes.data),
                 (o.ctypes.data, -1, p.ctypes.data, 3, 2, 4, ctypes.byref(c1), recs.ctypes.data, 4, ctypes.byref(c2), cols.ctypes.data),
                 (o.ctypes.data, 3, p.ctypes.data, 3, 2, 4, None, recs.ctypes.data, 4, ctypes.byref(c2), cols.ctypes.data),
                 (o.ctypes.data, 3, p.ctypes.data, 3, 2, 4, ctypes.byref(c1), recs.ctypes.data, 4, None, cols.ctypes.data),
                 (o.ctypes.data, 3, p.ctypes.data, 3, 2, 4, ctypes.byref(c1), None, 4, ctypes.byref(c2), cols.ctypes.data),
                 (o.ctypes.data, 3, p.ctypes.data, 3, 2, 4, ctypes.byref(c1), recs.ctypes.data, 4, ctypes.byref(c2), None)):
        assert L.wfa_hip_ops_insertions(*args) == _native.EINVAL, args
    assert c1.value == -1 and c2.value == -1 and (recs == FILL).all() and (cols == 99).all()
    with pytest.raises(ValueError, match="outruns its pair"):
        _native.ops_insertions(b"MDM", b"AC", 2)

    counts = np.zeros((3, 8), np.int32)
    counts[1] = [4, 0, 0, 0, 0, 0, 3, 0]
    good = dict(rec_row=[1, 1, 1], rec_n=[2, 2, 1], rec_off=[0, 2, 4], cols=[0, 1, 0, 1, 3])
    count, rows, nbases, bases = _native.insertions_host(counts, **good)
    assert count == 1 and rows.tolist() == [[0, 1, 4, 3, 2, 2, 2, 0]] and bases.tobytes() == b"AC"
    for change in (dict(min_depth=0), dict(min_permille=-1), dict(min_permille=1001), dict(cap=-1), dict(bases_cap=-1), dict(rec_n=[2, 2, -1]),
                   dict(rec_off=[0, 2, 5]), dict(rec_off=[-1, 2, 4])):
        with pytest.raises(ValueError, match="wfa_hip_insertions_host: invalid arguments"):
            _native.insertions_host(counts, **{**good, **change})
    rows, bases = np.full((2, 8), FILL, np.int32), np.full(4, 99, np.uint8)
    arrays = [np.array(good["rec_row"], np.int64), np.array(good["rec_n"], np.int32), np.array(good["rec_off"], np.int64), np.array(good["cols"], np.uint8)]
    ptrs = [a.ctypes.data for a in arrays]

    def host(counts_p=counts.ctypes.data, recs=ptrs, count_p=ctypes.byref(c1), rows_p=rows.ctypes.data, nb_p=ctypes.byref(c2), bases_p=bases.ctypes.data):
        return L.wfa_hip_insertions_host(counts_p, 3, 0, 0, 1, 500, 3, *recs, 5, 2, count_p, rows_p, 4, nb_p, bases_p)

    assert host(counts_p=None) == host(recs=[None] + ptrs[1:]) == host(recs=ptrs[:3] + [None]) == host(count_p=None) == host(rows_p=None) == _native.EINVAL
    assert host(nb_p=None) == host(bases_p=None) == _native.EINVAL
    assert c1.value == -1 and c2.value == -1 and (rows == FILL).all() and (bases == 99).all()
    assert host() == _native.OK and c1.value == 1 and c2.value == 2 and bases[:2].tobytes() == b"AC" and (bases[2:] == 99).all()


def test_header_binding_and_shim_declare_the_entries():
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    pxd = open(os.path.join(ROOT, "pywfa_amd", "cython_shim", "wfa_hip.pxd")).read()
    L = _native.lib()
    for name in ENTRIES:
        assert name + "(" in txt and name in _native.SYMBOLS and hasattr(L, name) and name + "(" in pxd, name
    assert "#define WFA_HIP_INSERTION_COLS 8 " in txt and "#define WFA_HIP_INS_MAX_READS 4096 " in txt
    assert raw.index("---- calls and sites:") < raw.index("---- insertions:") < raw.index("---- placement:")
    assert "does not record WHICH" not in raw and "ABOUT 24 BYTES PER RECORD AND 1 BYTE PER INSERTED" in raw
    assert _native.INSERTION_COLS == 8 and _native.INS_MAX_READS == 4096 and L.wfa_hip_abi_version() == _native.ABI_VERSION
    assert Pileup.INSERTION_COLUMNS == ("j", "pos", "depth", "ins_count", "allele_count", "allele_len", "alleles", "overflow")
    for name in ("track_insertions", "insertion_stats", "insertions"):
        assert hasattr(_native.Pileup, name), name
    assert os.path.exists(os.path.join(ROOT, "pywfa_amd", "csrc", "wfa_insertions.hpp")) and os.path.exists(os.path.join(ROOT, "pywfa_amd", "csrc", "k_insertions.hip"))
    assert "does not record which" not in Pileup.consensus.__doc__ and "with CIGARs" not in Pileup.sites.__doc__
    import inspect
    assert inspect.signature(WavefrontAligner.pileup).parameters["insertions"].default is False
    assert inspect.signature(Pileup.consensus).parameters["insertions"].default is False


def test_corpus_holds_what_it_is_for():
    """On the oracle alone: the conditions the GPU tests rely on."""
    e = expectation()
    refs, W, planted, tables = e["refs"], e["W"], e["planted"], e["tables"]
    assert (np.asarray(e["o"]["status"]) == 0).all() and len(e["reads"]) <= 2500 and sum(map(len, refs)) < 20000
    assert [len(r) for r in refs][4:] == [41, 0] and 15 <= np.concatenate(e["cover"][:3]).mean() <= 25
    # the invariant: the records at a row are its column 6
    for j, t in enumerate(tables):
        at = np.zeros(len(t), np.int64)
        for g, recs in e["records"][j].items():
            at[g] = len(recs)
        assert np.array_equal(at, t[:, 6]), j
    assert max(int(t[:, 6].max()) for t in tables if len(t)) < 64
    # a D run of at least 65 ops; runs that start at op indices 60..63 and end past 64, and at 124..127 past 128; one that ends at 63
    runs = []
    for q, ops in enumerate(e["o"]["cigars"]):
        if W["j"][q] == STAGE:
            runs += [(m.start(), m.end()) for m in re.finditer(rb"D+", ops)]
    assert any(b - a >= 65 for a, b in runs)
    for start in (60, 61, 62, 63):
        assert any(a == start and b > 64 for a, b in runs) and any(a == start + 64 and b > 128 for a, b in runs), start
    assert any(b == 64 for a, b in runs) and any(a == 64 for a, b in runs) and any(a == 128 for a, b in runs)
    # a window at t_start > 0 of a text that is not the first; reverse-strand reads that carry a record; a flagged pair with an N record
    assert all(W["t_start"][q] > 0 for q in range(len(e["pats"])) if W["j"][q] == STAGE)
    assert any(W["reverse"][q] and e["per_pair"][q] for q in range(len(e["pats"])))
    assert any(4 in cols for q in range(len(e["pats"])) if "N" in e["pats"][q] for _, _, cols in e["per_pair"][q])
    # every planted allele is what the rule recovers at min_depth 8, min_frac 0.5
    rows, seqs = expected_insertions(8, 500)
    got = {(int(r[0]), int(r[1])): (r, s) for r, s in zip(rows, seqs)}
    for name, (j, p, allele) in planted.items():
        if e["cover"][j][p] >= 8:
            assert (j, p) in got and got[(j, p)][1] == allele, (name, got.get((j, p)))
    assert sum(1 for j, p, _ in planted.values() if e["cover"][j][p] >= 8) >= len(planted) - 2
    assert "N" in got[planted["f"][:2]][1] and len(got[planted["d"][:2]][1]) == 70 and got[planted["d"][:2]][0][6] == 2
    b = got[planted["b"][:2]][0]
    assert (b[3], b[4], b[6]) == (9, 5, 2)                                # two alleles of different length, 5 against 4
    # the ties are exact, and the order decides: the shorter, the smaller letters
    for name in ("c_len", "c_let"):
        j, p, allele = planted[name]
        counts = sorted(__import__("collections").Counter(e["records"][j][p]).items(), key=lambda kv: kv[0])
        assert [c for _, c in counts] == [4, 4] and got[(j, p)][0][4] == 4 and got[(j, p)][0][6] == 2, name
        assert "".join(ASCII[x] for x in counts[0][0][1]) == allele == got[(j, p)][1], name
    (na, _), (nb, _) = [k for k, _ in sorted(__import__("collections").Counter(e["records"][STAGE][planted["c_len"][1]]).items())]
    assert na < nb
    (na, ca), (nb, cb) = [k for k, _ in sorted(__import__("collections").Counter(e["records"][STAGE][planted["c_let"][1]]).items())]
    assert na == nb and ca < cb
    # rows under the majority rule are exactly the insertion flags of the calls, and there are rows with several alleles
    all_rows, _ = expected_insertions(1, 0)
    assert len(all_rows) > len(planted) and (all_rows[:, 6] > 1).any() and (rows[:, 7] == 0).all()
