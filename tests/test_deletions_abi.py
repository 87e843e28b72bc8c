"""The deletion log of a pileup, without a GPU: the host statements wfa_hip_ops_deletions / wfa_hip_deletions_host against the Python
restatement of the rule (deletions_common), over the corpus and over random and hand-made op strings, with every parameter, ranges and
capacities below, at and above the counts; their refusals; the new entries in the header, the library, the binding and the shim; and
the conditions on the corpus itself that the GPU tests rely on, from the oracle-derived expectation alone."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from deletions_common import ADJACENT, STAGE, all_rows, expectation, expected_deletions, in_range, py_deletions, py_ops_deletions
from pywfa_amd import _native
from pywfa_amd.align import Pileup, WavefrontAligner
from reduce_common import core_of

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRIES = ("wfa_hip_pileup_track_deletions", "wfa_hip_pileup_deletion_stats", "wfa_hip_pileup_read_deletion_starts", "wfa_hip_pileup_deletions",
           "wfa_hip_ops_deletions", "wfa_hip_deletions_host")
FILL = -7


def lengths(ops):
    ops = bytes(ops)
    return sum(1 for c in ops if c in b"MXD"), sum(1 for c in ops if c in b"MXI")


def ops_raw(ops, plen, tlen, cap):
    """wfa_hip_ops_deletions on a prefilled array: (rc, count, recs)."""
    o = np.frombuffer(bytes(ops), np.uint8)
    recs = np.full((cap, 2), FILL, np.int32)
    count = ctypes.c_int64(-1)
    rc = _native.lib().wfa_hip_ops_deletions(o.ctypes.data if o.size else None, o.size, plen, tlen, cap, ctypes.byref(count),
                                             recs.ctypes.data if cap else None)
    return rc, count.value, recs


def check_ops(ops, plen=None, tlen=None):
    nv, nh = lengths(ops)
    plen, tlen = nv if plen is None else plen, nh if tlen is None else tlen
    want = np.array(py_ops_deletions(ops), np.int32).reshape(-1, 2)
    n = len(want)
    assert np.array_equal(_native.ops_deletions(ops, plen, tlen), want), ops
    for cap in {0, max(n - 1, 0), n, n + 3}:
        rc, count, recs = ops_raw(ops, plen, tlen, cap)
        k = min(cap, n)
        assert rc == _native.OK and count == n and np.array_equal(recs[:k], want[:k]) and (recs[k:] == FILL).all(), (ops, cap)
    return n


def random_ops(rng):
    """An op string with I runs before, inside and behind its core, some beside D runs, some longer than 64."""
    parts = []
    for _ in range(int(rng.integers(0, 12))):
        parts.append("MXDI"[int(rng.choice(4, p=[0.45, 0.1, 0.15, 0.3]))] * int(rng.integers(1, 5 if rng.random() < 0.9 else 150)))
    return "".join(parts).encode()


def test_ops_deletions_on_random_and_hand_made_op_strings():
    rng = np.random.default_rng(37)
    seen = 0
    for _ in range(1500):
        ops = random_ops(rng)
        nv, nh = lengths(ops)
        seen += check_ops(ops, nv + int(rng.integers(0, 3)), nh + int(rng.integers(0, 3)))
    assert seen > 500          # (the generator does produce runs inside cores)
    # by hand: the I run in front of the first M and the one behind the last M are no records; an X may stand beside a run
    assert py_ops_deletions(b"IIMXIIIDMIMII") == [(4, 3), (8, 1)] and check_ops(b"IIMXIIIDMIMII") == 2
    assert check_ops(b"") == 0 and check_ops(b"III") == 0 and check_ops(b"DDXIX") == 0 and check_ops(b"M") == 0
    # (h) a D run beside an I run neither breaks nor joins it
    want = {ADJACENT[0]: [(3, 3)], ADJACENT[1]: [(2, 3), (7, 1)], ADJACENT[2]: [(1, 1), (2, 1), (3, 1)], ADJACENT[3]: [(4, 2), (7, 2)]}
    for ops in ADJACENT:
        assert py_ops_deletions(ops) == want[ops] and check_ops(ops) == len(want[ops]), ops
    # runs longer than one 64-op round, and ones that end or start at op 64 and 128
    for left in (1, 59, 63, 64, 65, 127, 128):
        for n in (1, 5, 64, 70, 129):
            assert py_ops_deletions(b"M" * left + b"I" * n + b"MM") == [(left, n)] and check_ops(b"M" * left + b"I" * n + b"MM") == 1


def test_ops_deletions_on_the_corpus():
    e = expectation()
    for q, ops in enumerate(e["o"]["cigars"]):
        got = _native.ops_deletions(ops, len(e["pats"][q]), int(e["W"]["t_len"][q]))
        assert np.array_equal(got, np.array(py_ops_deletions(ops), np.int32).reshape(-1, 2)), q
    for q in range(0, len(e["pats"]), 97):
        check_ops(e["o"]["cigars"][q], len(e["pats"][q]), int(e["W"]["t_len"][q]))


def record_arrays(records, lo=0, hi=None, rng=None):
    """The records that start in the rows [lo, hi) of one reference as the arrays wfa_hip_deletions_host takes, rows relative to lo;
    shuffled when `rng` is given (the rule does not depend on the order)."""
    items = [(g - lo, n) for g, lens in records.items() if g >= lo and (hi is None or g < hi) for n in lens]
    if rng is not None:
        items = [items[k] for k in rng.permutation(len(items))]
    return np.array([g for g, _ in items], np.int64), np.array([n for _, n in items], np.int32)


@pytest.mark.parametrize("min_depth", [1, 8])
@pytest.mark.parametrize("permille", [0, 1, 200, 500, 1000])
def test_deletions_host_on_the_corpus(min_depth, permille):
    e = expectation()
    rng = np.random.default_rng(5)
    for j, t in enumerate(e["tables"]):
        want = py_deletions(t, e["starts"][j], e["records"][j], j, 0, min_depth, permille)
        for shuffle in (None, rng):
            count, rows = _native.deletions_host(t, e["starts"][j], *record_arrays(e["records"][j], rng=shuffle), seq=j, min_depth=min_depth,
                                                 min_permille=permille)
            assert count == len(want) and rows.dtype == np.int32 and np.array_equal(rows, want), (j, count, len(want))
    # ranges of the stage, numbered from their start: one that starts and one that ends inside the 70-base deletion; records that start
    # outside the range are skipped, a row's deleted bases may reach past it
    t, s, recs = e["tables"][STAGE], e["starts"][STAGE], e["records"][STAGE]
    d = e["planted"]["d"][1]
    for lo, hi in ((250, 1500), (d + 10, 1500), (250, d + 10), (d, d + 1), (d + 1, d + 70)):
        want = py_deletions(t[lo:hi], s[lo:hi], {g - lo: v for g, v in recs.items()}, STAGE, lo, min_depth, permille)
        got = _native.deletions_host(t[lo:hi], s[lo:hi], *record_arrays(recs, lo), seq=STAGE, start=lo, min_depth=min_depth, min_permille=permille)
        assert got[0] == len(want) and np.array_equal(got[1], want), (lo, hi)
        assert np.array_equal(want, in_range(expected_deletions(min_depth, permille), STAGE, lo, hi - lo)), (lo, hi)


def test_deletions_host_capacities_and_overflow(monkeypatch):
    monkeypatch.delenv("WFA_HIP_DEL_MAX_READS", raising=False)
    e = expectation()
    t, s, recs = e["tables"][STAGE], e["starts"][STAGE], record_arrays(e["records"][STAGE])
    want = py_deletions(t, s, e["records"][STAGE], STAGE, 0, 1, 200)
    n = len(want)
    assert n >= 7
    for cap in (0, 1, n - 1, n, n + 4):
        rows = np.full((cap, 8), FILL, np.int32)
        count = ctypes.c_int64(-1)
        rc = _native.lib().wfa_hip_deletions_host(t.ctypes.data, s.ctypes.data, len(t), STAGE, 0, 1, 200, len(recs[0]), *[a.ctypes.data for a in recs],
                                                  cap, ctypes.byref(count), rows.ctypes.data if cap else None)
        k = min(cap, n)
        assert rc == _native.OK and count.value == n and np.array_equal(rows[:k], want[:k]) and (rows[k:] == FILL).all(), cap
    # the limit, read per call: the rows above it report overflow and zeros, the others are unchanged
    monkeypatch.setenv("WFA_HIP_DEL_MAX_READS", "8")
    low = py_deletions(t, s, e["records"][STAGE], STAGE, 0, 1, 200, max_reads=8)
    assert 0 < low[:, 7].sum() < len(low) and (low[low[:, 7] == 1][:, 4:7] == 0).all() and np.array_equal(low[low[:, 7] == 0], want[low[:, 7] == 0])
    assert np.array_equal(_native.deletions_host(t, s, *recs, seq=STAGE, min_permille=200)[1], low)
    monkeypatch.setenv("WFA_HIP_DEL_MAX_READS", "0")        # (at least 1)
    assert np.array_equal(_native.deletions_host(t, s, *recs, seq=STAGE, min_permille=200)[1], py_deletions(t, s, e["records"][STAGE], STAGE, 0, 1, 200, 1))


def test_refusals():
    L = _native.lib()
    assert ops_raw(b"MIM", 2, 3, 4)[0] == _native.OK
    for ops, plen, tlen in ((b"MIM", 1, 3), (b"MIM", 2, 2), (b"MDM", 2, 2), (b"MIM", -1, 3), (b"MIM", 2, -3)):
        rc, count, recs = ops_raw(ops, plen, tlen, 4)
        assert rc == _native.EINVAL and count == -1 and (recs == FILL).all(), (ops, plen, tlen)
    o = np.frombuffer(b"MIM", np.uint8)
    c1 = ctypes.c_int64(-1)
    recs = np.full((4, 2), FILL, np.int32)
    for args in ((None, 3, 2, 3, 4, ctypes.byref(c1), recs.ctypes.data), (o.ctypes.data, -1, 2, 3, 4, ctypes.byref(c1), recs.ctypes.data),
                 (o.ctypes.data, 3, 2, 3, -1, ctypes.byref(c1), recs.ctypes.data), (o.ctypes.data, 3, 2, 3, 4, None, recs.ctypes.data),
                 (o.ctypes.data, 3, 2, 3, 4, ctypes.byref(c1), None)):
        assert L.wfa_hip_ops_deletions(*args) == _native.EINVAL, args
    assert c1.value == -1 and (recs == FILL).all()
    with pytest.raises(ValueError, match="outruns its pair"):
        _native.ops_deletions(b"MIM", 2, 2)

    counts = np.zeros((4, 8), np.int32)
    counts[1] = [1, 0, 0, 0, 0, 3, 0, 0]
    starts = np.array([0, 3, 0, 0], np.int32)
    good = dict(rec_row=[1, 1, 1], rec_n=[2, 3, 3])
    count, rows = _native.deletions_host(counts, starts, **good)
    assert count == 1 and rows.tolist() == [[0, 1, 4, 3, 2, 3, 2, 0]]
    for change in (dict(min_depth=0), dict(min_permille=-1), dict(min_permille=1001), dict(cap=-1), dict(rec_n=[2, 3, 0]), dict(rec_n=[2, -3, 3])):
        with pytest.raises(ValueError, match="wfa_hip_deletions_host: invalid arguments"):
            _native.deletions_host(counts, starts, **{**good, **change})
    with pytest.raises(ValueError, match="one value per row"):
        _native.deletions_host(counts, starts[:3], **good)
    rows = np.full((2, 8), FILL, np.int32)
    arrays = [np.array(good["rec_row"], np.int64), np.array(good["rec_n"], np.int32)]
    ptrs = [a.ctypes.data for a in arrays]

    def host(counts_p=counts.ctypes.data, starts_p=starts.ctypes.data, recs=ptrs, count_p=ctypes.byref(c1), rows_p=rows.ctypes.data):
        return L.wfa_hip_deletions_host(counts_p, starts_p, 4, 0, 0, 1, 500, 3, *recs, 2, count_p, rows_p)

    assert host(counts_p=None) == host(starts_p=None) == host(recs=[None, ptrs[1]]) == host(recs=[ptrs[0], None]) == _native.EINVAL
    assert host(count_p=None) == host(rows_p=None) == _native.EINVAL
    assert c1.value == -1 and (rows == FILL).all()
    assert host() == _native.OK and c1.value == 1 and rows[0].tolist() == [0, 1, 4, 3, 2, 3, 2, 0] and (rows[1] == FILL).all()


def test_header_binding_and_shim_declare_the_entries():
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    pxd = open(os.path.join(ROOT, "pywfa_amd", "cython_shim", "wfa_hip.pxd")).read()
    L = _native.lib()
    for name in ENTRIES:
        assert name + "(" in txt and name in _native.SYMBOLS and hasattr(L, name) and name + "(" in pxd, name
    assert "#define WFA_HIP_DELETION_COLS 8 " in txt and "#define WFA_HIP_DEL_MAX_READS 4096 " in txt
    assert raw.index("---- insertions:") < raw.index("---- deletions:") < raw.index("---- strands and genotypes:")
    assert "Out of scope: multi-base events" not in raw and "16 BYTES PER RECORD" in raw and "4 MORE BYTES PER TEXT" in raw
    assert "VCF anchors a deletion one base earlier" in raw
    assert _native.DELETION_COLS == 8 and _native.DEL_MAX_READS == 4096 and L.wfa_hip_abi_version() == _native.ABI_VERSION
    assert Pileup.DELETION_COLUMNS == ("j", "pos", "depth", "del_count", "allele_count", "allele_len", "alleles", "overflow")
    for name in ("track_deletions", "deletion_stats", "deletion_starts", "deletions"):
        assert hasattr(_native.Pileup, name), name
    assert hasattr(_native, "ops_deletions") and hasattr(_native, "deletions_host")
    for name in ("wfa_deletions.hpp", "k_deletions.hip"):
        assert os.path.exists(os.path.join(ROOT, "pywfa_amd", "csrc", name)), name
    assert os.path.exists(os.path.join(ROOT, "tools", "deletions_host_check.cpp"))
    assert inspect.signature(WavefrontAligner.pileup).parameters["deletions"].default is False
    assert inspect.signature(Pileup.deletions).parameters["min_frac"].default == 0.5
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "multi-base events" not in readme and readme.index("What the reads insert") < readme.index("What the reads delete")


def test_corpus_holds_what_it_is_for():
    """On the oracle alone: the invariants of the rule, and the conditions the GPU tests rely on."""
    e = expectation()
    refs, W, planted, tables, starts = e["refs"], e["W"], e["planted"], e["tables"], e["starts"]
    assert (np.asarray(e["o"]["status"]) == 0).all() and len(e["reads"]) <= 2500 and sum(map(len, refs)) < 20000
    assert [len(r) for r in refs][4:] == [41, 0] and 15 <= np.concatenate(e["cover"][:3]).mean() <= 25 and "N" * 16 in refs[2]
    assert all(2500 <= len(r) <= 3500 for r in refs[:4]) and W["reverse"][1::2].all() and not W["reverse"][0::2].any()
    # the invariants: the records that cover a row are its column 5; the records that start at a row are at most that
    for j, t in enumerate(tables):
        cover = np.zeros(len(t) + 1, np.int64)
        for g, lens in e["records"][j].items():
            for n in lens:
                cover[g] += 1
                cover[g + n] -= 1
        assert np.array_equal(np.cumsum(cover)[:-1], t[:, 5]) and (starts[j] <= t[:, 5]).all(), j
    assert max(int(s.max()) for s in starts if len(s)) < 64
    assert sum(len(r) for r in e["per_pair"]) > 500 and any(n > 1 for r in e["per_pair"] for _, n in r)
    # no I run beside a D run inside a core under these penalties: case (h) goes to the host statement alone
    for ops in e["o"]["cigars"]:
        a, b = core_of(ops)
        assert not re.search(rb"ID|DI", bytes(ops)[a:b + 1])
    # an I run of at least 65 ops, one that fills a whole round; runs that start at op indices 60..63 and end past 64, and at 124..127
    # past 128; ones that end at 63 / 127 and start at 64 / 128
    runs = []
    for q, ops in enumerate(e["o"]["cigars"]):
        if W["j"][q] == STAGE:
            runs += [(m.start(), m.end()) for m in re.finditer(rb"I+", ops)]
    assert any(b - a >= 65 for a, b in runs) and any(a <= 64 and b >= 128 for a, b in runs)
    for start in (60, 61, 62, 63):
        assert any(a == start and b > 64 for a, b in runs) and any(a == start + 64 and b > 128 for a, b in runs), start
    assert any(b == 64 for a, b in runs) and any(a == 64 for a, b in runs) and any(b == 128 for a, b in runs) and any(a == 128 for a, b in runs)
    # windows at t_start > 0 of a text that is not the first; reverse-strand reads that carry a record; a flagged pair with a record
    assert all(W["t_start"][q] > 0 for q in range(len(e["pats"])) if W["j"][q] == STAGE)
    assert any(W["reverse"][q] and e["per_pair"][q] for q in range(len(e["pats"])))
    assert sum(1 for q in range(len(e["pats"])) if "N" in e["pats"][q] and W["j"][q] == STAGE and e["per_pair"][q]) >= 3
    # every planted site is what the rule recovers at min_depth 8, min_frac 0.5 (expectation() asserts it too)
    rows = expected_deletions(8, 500)
    got = {(int(r[0]), int(r[1])): r for r in rows}
    for name, (j, p, n) in planted.items():
        if name != "g_in":
            assert (j, p) in got and got[(j, p)][5] == n and e["cover"][j][p] >= 8, (name, got.get((j, p)))
    b = got[planted["b"][:2]]
    assert (b[3], b[4], b[5], b[6]) == (9, 5, 2, 2)                       # two lengths, 5 against 4
    c = got[planted["c"][:2]]
    assert (c[3], c[4], c[5], c[6]) == (8, 4, 2, 2)                       # an exact tie: the shorter
    assert sorted(__import__("collections").Counter(e["records"][STAGE][planted["c"][1]]).items()) == [(2, 4), (3, 4)]
    d = got[planted["d"][:2]]
    assert (d[3], d[4], d[5], d[6]) == (10, 9, 70, 2) and sorted(set(e["records"][STAGE][planted["d"][1]])) == [69, 70]
    # (g) the nested deletion is a row of its own under a lower min_frac, and is covered by the longer one's reads
    low = {(int(r[0]), int(r[1])): r for r in expected_deletions(8, 200)}
    g, g_in = low[planted["g"][:2]], low[planted["g_in"][:2]]
    assert (g[3], g[5]) == (6, 12) and (g_in[2], g_in[3], g_in[5]) == (11, 5, 3) and planted["g_in"][:2] not in got
    assert planted["g"][1] < planted["g_in"][1] and planted["g_in"][1] + 3 < planted["g"][1] + 12
    # rows with several lengths; no overflow at the default limit
    assert (expected_deletions(1, 1)[:, 6] > 1).sum() >= 3 and (expected_deletions(1, 1)[:, 7] == 0).all()
    assert np.array_equal(all_rows(tables, starts, e["records"], 8, 500), rows)
