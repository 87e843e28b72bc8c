"""The deletion log of a pileup on the GPU (wfa_hip_pileup_track_deletions / _deletion_stats / _read_deletion_starts / _deletions,
pileup(deletions=True), Pileup.deletions, Pileup.deletion_starts): the device must equal the Python restatement of the rule
(deletions_common) applied to the records, planes and tables built from the ORACLE's op strings — never to the device's own output —
exactly: through the C ABI over parameters, ranges, capacities and chunk sizes, with the list added in pieces and in reversed order,
after a clear, with a keep mask, with the limit lowered, beside the insertion, strand and quality tracks, with tracking off, on
recycled memory filled with a poison byte; and from Python with handles and with lists, left-aligned."""
import ctypes

import numpy as np
import pytest

from common import configs_pair
from deletions_common import KW, STAGE, all_rows, expectation, expected_deletions, in_range, py_deletions, py_ops_deletions, records_of, starts_of
from leftalign_common import py_left_align
from oracle import loader
from pywfa_amd import WavefrontAligner, _native, datagen
from reduce_common import expected_tables
from test_windows_gpu import as_list, materialise, native_set, native_windows

FILL = -7


def ranges():
    """Rows of the first text, around the N run, the stage whole, ranges that start and that end inside the 70-base deletion, its first
    base alone, the short text in part and whole, empty ranges at the end of a text and of the empty text."""
    d = expectation()["planted"]["d"][1]
    return [(0, 13, 1000), (2, 1001, 1999), (STAGE, 250, 2400), (STAGE, d + 10, 600), (STAGE, 250, d + 10 - 250), (STAGE, d, 1), (STAGE, d + 1, 69),
            (1, 1960, 500), (4, 5, 30), (4, 0, 41), (1, 3500, 0), (3, 0, 0), (5, 0, 0)]


class Rig:
    """An aligner, the two sets and a pileup of the corpus at the C ABI binding; `order`: the pieces of the list (of `parts`) in the
    order they are added; `track`: whether the pileup tracks deletions; `keep`: a mask over the list; `also`: the insertion, strand and
    quality tracks beside it (qualities seeded, nothing filtered)."""

    def __init__(self, parts=1, order=None, track=True, keep=None, also=False):
        e = expectation()
        self.e = e
        _, nc = configs_pair(**KW)
        self.al = _native.Aligner(nc)
        self.ps, self.ts = native_set(self.al, e["reads"]), native_set(self.al, e["refs"])
        self.pile = self.al.pileup(self.ts)
        if track:
            self.pile.track_deletions(True)
        self.qs = None
        if also:
            self.pile.track_insertions(True)
            self.pile.track_strands(True)
            self.pile.track_qualities(True)
            rng = np.random.default_rng(3)
            length = np.array([len(r) for r in e["reads"]], np.int32)
            off = np.concatenate([[0], np.cumsum(length)[:-1]]).astype(np.int64)
            self.qs = self.al.qualset(self.ps, rng.integers(2, 42, int(length.sum())).astype(np.uint8), off, length)
        n = len(e["W"]["i"])
        cuts = [n * k // parts for k in range(parts + 1)]
        self.batches = []
        for k in (range(parts) if order is None else order):
            part = {key: v[cuts[k]:cuts[k + 1]] for key, v in e["W"].items()}
            rb = native_windows(self.al, self.ps, self.ts, part)
            rb.run()
            self.batches.append((rb, part, None if keep is None else keep[cuts[k]:cuts[k + 1]]))
            self.add(len(self.batches) - 1)

    def add(self, k):
        rb, part, keep = self.batches[k]
        if self.qs is not None:
            self.pile.add_quals(rb, part["j"], self.qs, part["i"], part["t_start"], keep, part["reverse"], part["p_start"], 0, 40)
        else:
            self.pile.add(rb, part["j"], part["t_start"], keep)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.al.close()
        return False

    def raw(self, seq, start, length, md, pm, cap, count, rows, ts=None):
        ts = self.ts if ts is None else ts
        return _native.lib().wfa_hip_pileup_deletions(self.pile._h, ts._h, seq, start, length, md, pm, cap, count, rows)

    def dels(self, seq=-1, start=0, length=-1, md=1, pm=500, cap=None):
        """wfa_hip_pileup_deletions on an array prefilled with FILL: (count, rows); a capacity of None: the counting call first."""
        count = ctypes.c_int64(-1)
        if cap is None:
            assert self.raw(seq, start, length, md, pm, 0, ctypes.byref(count), None) == _native.OK, self.al.error()
            cap = count.value
        rows = np.full((cap, 8), FILL, np.int32)
        rc = self.raw(seq, start, length, md, pm, cap, ctypes.byref(count), rows.ctypes.data if cap else None)
        assert rc == _native.OK, self.al.error()
        return count.value, rows

    def check(self, want, ctx, **kw):
        count, got = self.dels(**kw)
        assert count == len(want) and np.array_equal(got, want), (ctx, count, len(want))
        return got

    def check_planes(self, starts, total, ctx):
        for j, s in enumerate(starts):
            assert np.array_equal(self.pile.deletion_starts(j), s), (ctx, j)
        assert self.pile.deletion_stats() == total, ctx


def totals(per_pair, keep=None):
    recs = [r for q, rs in enumerate(per_pair) if keep is None or keep[q] for r in rs]
    return len(recs), sum(n for _, n in recs)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", ["64", None])
def test_c_abi_over_parameters_ranges_and_capacities(gpu, monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("WFA_HIP_CALLS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("WFA_HIP_CALLS_CHUNK", chunk)
    monkeypatch.delenv("WFA_HIP_DEL_MAX_READS", raising=False)
    with Rig() as rig:
        e = rig.e
        for j, t in enumerate(e["tables"]):
            assert np.array_equal(rig.pile.read(j), t), j
        rig.check_planes(e["starts"], totals(e["per_pair"]), "whole list")
        d = e["planted"]["d"][1]
        assert np.array_equal(rig.pile.deletion_starts(STAGE, d - 3, 9), e["starts"][STAGE][d - 3:d + 6]) and e["starts"][STAGE][d] == 10
        assert len(rig.pile.deletion_starts(5)) == 0 and len(rig.pile.deletion_starts(1, 3500, 0)) == 0
        for md in (1, 8):
            for pm in (0, 1, 200, 500, 1000):
                got = rig.check(expected_deletions(md, pm), (md, pm), md=md, pm=pm)
                assert rig.dels(md=md, pm=pm)[1].tobytes() == got.tobytes()          # two calls, identical bytes
        want = expected_deletions(1, 200)
        for seq, start, length in ranges():
            rig.check(in_range(want, seq, start, length), (seq, start, length), seq=seq, start=start, length=length, pm=200)
        assert len(in_range(want, STAGE, d, 1)) == 1 and len(in_range(want, STAGE, d + 1, 69)) == 0
        n = len(want)
        assert n > 12
        for cap in (0, 1, n - 1, n, n + 1, n + 5):
            count, got = rig.dels(pm=200, cap=cap)
            k = min(cap, n)
            assert count == n and np.array_equal(got[:k], want[:k]) and (got[k:] == FILL).all(), cap
        w = in_range(want, STAGE, 250, 2400)
        count, got = rig.dels(STAGE, 250, 2400, pm=200, cap=3)
        assert count == len(w) >= 7 and np.array_equal(got, w[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("parts,order", [(3, None), (3, (2, 1, 0))])
def test_pieces_orders_stats_and_a_clear(gpu, monkeypatch, parts, order):
    monkeypatch.setenv("WFA_HIP_CALLS_CHUNK", "192")
    monkeypatch.delenv("WFA_HIP_DEL_MAX_READS", raising=False)
    with Rig(parts, order) as rig:
        e = rig.e
        total = totals(e["per_pair"])
        assert total[0] > 500
        rig.check_planes(e["starts"], total, (parts, order))
        for md, pm in ((1, 500), (8, 0), (1, 1)):
            rig.check(expected_deletions(md, pm), (parts, order, md, pm), md=md, pm=pm)
        if order is not None:
            return
        # cleared: the log is dropped, the plane zeroed, the setting kept; the last third added twice and the first once
        rig.pile.clear()
        assert rig.pile.deletion_stats() == (0, 0) and not rig.pile.deletion_starts(STAGE).any() and rig.dels(cap=4)[0] == 0
        for k in (2, 0, 2):
            rig.add(k)
        n = len(e["pats"])
        q = np.arange(n)
        first, third = q < n // 3, q >= 2 * n // 3
        lens = [len(r) for r in e["refs"]]
        args = (e["o"], e["pats"], e["W"]["j"], e["W"]["t_start"], e["W"]["t_len"])
        tables = [a + 2 * b for a, b in zip(expected_tables(lens, *args, first)[0], expected_tables(lens, *args, third)[0])]
        one, two = records_of(e["per_pair"], e["W"], len(lens), first), records_of(e["per_pair"], e["W"], len(lens), third)
        records = [{g: one[j].get(g, []) + 2 * two[j].get(g, []) for g in set(one[j]) | set(two[j])} for j in range(len(lens))]
        starts = starts_of(records, e["refs"])
        t1, t3 = totals(e["per_pair"], first), totals(e["per_pair"], third)
        rig.check_planes(starts, (t1[0] + 2 * t3[0], t1[1] + 2 * t3[1]), "re-added")
        rows = all_rows(tables, starts, records, 8, 200)
        rig.check(rows, "re-added", md=8, pm=200)
        assert len(rows) >= 4 and not np.array_equal(rows, expected_deletions(8, 200))
        # ... and cleared again, the whole list once: as at first
        rig.pile.clear()
        for k in range(parts):
            rig.add(k)
        rig.check(expected_deletions(1, 500), "after a clear and a re-add")
        rig.check_planes(e["starts"], total, "after a clear and a re-add")


@pytest.mark.gpu
def test_keep_mask_and_the_limit_lowered(gpu, monkeypatch):
    monkeypatch.delenv("WFA_HIP_DEL_MAX_READS", raising=False)
    e = expectation()
    keep = (np.arange(len(e["pats"])) % 3 != 1).astype(np.uint8)
    lens = [len(r) for r in e["refs"]]
    tables, _ = expected_tables(lens, e["o"], e["pats"], e["W"]["j"], e["W"]["t_start"], e["W"]["t_len"], keep)
    records = records_of(e["per_pair"], e["W"], len(lens), keep)
    starts = starts_of(records, e["refs"])
    with Rig(2, keep=keep) as rig:
        rig.check_planes(starts, totals(e["per_pair"], keep), "keep")
        assert totals(e["per_pair"], keep)[0] < totals(e["per_pair"])[0]
        for md, pm in ((1, 500), (1, 1), (8, 0)):
            rig.check(all_rows(tables, starts, records, md, pm), ("keep", md, pm), md=md, pm=pm)
    with Rig() as rig:
        full, low = expected_deletions(1, 1), expected_deletions(1, 1, 3)
        over = low[:, 7] == 1
        assert over.sum() >= 8 and (~over).sum() >= 100 and (low[over][:, 4:7] == 0).all() and (low[over][:, 3] > 3).all()
        assert np.array_equal(low[~over], full[~over])
        monkeypatch.setenv("WFA_HIP_DEL_MAX_READS", "3")
        rig.check(low, "limit 3", pm=1)
        monkeypatch.setenv("WFA_HIP_DEL_MAX_READS", "0")       # (at least 1)
        rig.check(expected_deletions(1, 1, 1), "limit 1", pm=1)
        monkeypatch.delenv("WFA_HIP_DEL_MAX_READS")
        rig.check(full, "limit back at its default", pm=1)


@pytest.mark.gpu
def test_beside_the_insertion_strand_and_quality_tracks(gpu, monkeypatch):
    """With every other track on: the deletion rows are the rule's, and the tables, the insertion rows and the genotypes are byte for
    byte what the same pileup gives without deletion tracking."""
    monkeypatch.delenv("WFA_HIP_DEL_MAX_READS", raising=False)
    with Rig(2, also=True) as rig, Rig(2, also=True, track=False) as plain:
        e = rig.e
        rig.check_planes(e["starts"], totals(e["per_pair"]), "every track")
        for md, pm in ((1, 500), (8, 200), (1, 0)):
            rig.check(expected_deletions(md, pm), ("every track", md, pm), md=md, pm=pm)
        for j in range(len(e["refs"])):
            assert np.array_equal(rig.pile.read(j), e["tables"][j]), j
            for a, b in ((rig.pile.read(j), plain.pile.read(j)), (rig.pile.read(j, strand=0), plain.pile.read(j, strand=0)),
                         (rig.pile.read_quality(j), plain.pile.read_quality(j))):
                assert a.tobytes() == b.tobytes(), j
        assert rig.pile.insertion_stats() == plain.pile.insertion_stats() and rig.pile.insertion_stats()[0] > 100
        a, b = rig.pile.insertions(rig.ts, min_permille=1), plain.pile.insertions(plain.ts, min_permille=1)
        assert a[0] == b[0] > 100 and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[3].tobytes() == b[3].tobytes()
        for quals in (False, True):
            a = rig.pile.genotypes(rig.ts, min_permille=1, min_alt_strand=1, qualities=quals)
            b = plain.pile.genotypes(plain.ts, min_permille=1, min_alt_strand=1, qualities=quals)
            assert a[0] == b[0] > 100 and a[1].tobytes() == b[1].tobytes(), quals
        # a stranded pileup without qualities takes the log too
        rig.pile.clear()
        rig.pile.track_qualities(False)
        rig.qs = None
        for rb, part, _ in rig.batches:
            rig.pile.add(rb, part["j"], part["t_start"], None, part["reverse"])
        rig.check_planes(e["starts"], totals(e["per_pair"]), "strands and insertions")
        rig.check(expected_deletions(1, 500), "strands and insertions")


@pytest.mark.gpu
def test_tracking_off_and_the_refusals(gpu):
    with Rig() as rig, Rig(track=False) as plain:
        for j in range(len(rig.e["refs"])):
            assert np.array_equal(rig.pile.read(j), plain.pile.read(j)) and np.array_equal(plain.pile.read(j), rig.e["tables"][j]), j
        rows = np.full((4, 8), FILL, np.int32)
        count = ctypes.c_int64(-1)

        def refused(r, rc, pattern):
            assert rc == _native.EINVAL and pattern in r.al.error(), (rc, r.al.error())
            assert (rows == FILL).all() and count.value == -1

        def call(r, seq=-1, start=0, length=-1, md=1, pm=500, cap=4, cnt=ctypes.byref(count), rowp=rows.ctypes.data, ts=None):
            return r.raw(seq, start, length, md, pm, cap, cnt, rowp, ts)

        L = _native.lib()
        out = np.full(8, FILL, np.int32)
        refused(plain, call(plain), "was not made to track deletions")
        assert L.wfa_hip_pileup_deletion_stats(plain.pile._h, None, None) == _native.EINVAL and "was not made to track deletions" in plain.al.error()
        assert L.wfa_hip_pileup_read_deletion_starts(plain.pile._h, 0, 0, 8, out.ctypes.data) == _native.EINVAL and (out == FILL).all()
        assert "was not made to track deletions" in plain.al.error()
        assert L.wfa_hip_pileup_read_deletion_starts(rig.pile._h, 0, 2495, 8, out.ctypes.data) == _native.EINVAL and (out == FILL).all()
        assert "rows [2495, 2495 + 8) of sequence 0 are out of range" in rig.al.error()
        assert L.wfa_hip_pileup_read_deletion_starts(rig.pile._h, 0, 0, 8, None) == _native.EINVAL and "null output" in rig.al.error()
        assert L.wfa_hip_pileup_deletion_stats(rig.pile._h, None, None) == _native.OK
        for r in (rig, plain):       # after an add the setting stays
            for on in (0, 1):
                assert L.wfa_hip_pileup_track_deletions(r.pile._h, on) == _native.EINVAL and "while the pileup is empty" in r.al.error()
        refused(plain, call(plain), "was not made to track deletions")
        refused(rig, call(rig, cap=-1), "cap = -1 is negative")
        refused(rig, call(rig, md=0), "min_depth = 0 is out of range")
        refused(rig, call(rig, pm=-1), "min_permille = -1 is out of range (0 .. 1000)")
        refused(rig, call(rig, pm=1001), "min_permille = 1001 is out of range (0 .. 1000)")
        refused(rig, call(rig, start=5), "seq = -1 (every sequence) goes with start = 0 and len = -1")
        refused(rig, call(rig, seq=0, start=2490, length=11), "rows [2490, 2490 + 11) of sequence 0 are out of range")
        refused(rig, call(rig, seq=6, start=0, length=1), "out of range")
        refused(rig, call(rig, ts=rig.ps), "the set holds")
        refused(rig, call(rig, ts=plain.ts), "sequence set of another aligner")
        refused(rig, call(rig, cnt=None), "null count")
        refused(rig, call(rig, rowp=None), "null rows")
        # a cleared pileup takes the setting again: off, the list added, as the plain one; on again after another clear
        rig.pile.clear()
        rig.pile.track_deletions(False)
        rig.add(0)
        refused(rig, call(rig), "was not made to track deletions")
        assert np.array_equal(rig.pile.read(STAGE), plain.pile.read(STAGE))
        rig.pile.clear()
        rig.pile.track_deletions(True)
        rig.add(0)
        rig.check(expected_deletions(1, 500), "tracking on again")
        rig.check_planes(rig.e["starts"], totals(rig.e["per_pair"]), "tracking on again")


@pytest.mark.gpu
@pytest.mark.parametrize("poison", ["127", "255"])
def test_on_recycled_memory_filled_with_a_poison_byte(gpu, monkeypatch, poison):
    """WFA_HIP_POISON (read when the aligner is created) fills whatever the library hands out: the plane, the log's grown tail, every
    scratch block.  The list in three pieces, so that the log grows over its own contents; the reductions twice."""
    monkeypatch.setenv("WFA_HIP_POISON", poison)
    monkeypatch.setenv("WFA_HIP_CALLS_CHUNK", "128")
    monkeypatch.delenv("WFA_HIP_DEL_MAX_READS", raising=False)
    with Rig(3, (1, 2, 0)) as rig:
        e = rig.e
        for rnd in range(2):
            rig.check_planes(e["starts"], totals(e["per_pair"]), (poison, rnd))
            for md, pm in ((1, 500), (8, 200), (1, 1), (1, 0)):
                rig.check(expected_deletions(md, pm), (poison, rnd, md, pm), md=md, pm=pm)
            rig.check(in_range(expected_deletions(1, 200), STAGE, 250, 2400), (poison, rnd, "range"), seq=STAGE, start=250, length=2400, pm=200)
        for j, t in enumerate(e["tables"]):
            assert np.array_equal(rig.pile.read(j), t), j


def window_kw(W):
    return dict(i=W["i"], j=W["j"], pattern_start=W["p_start"], pattern_len=W["p_len"], text_start=W["t_start"], text_len=W["t_len"], reverse=W["reverse"])


def stacked(d, columns):
    return np.stack([d[k] for k in columns], axis=1)


@pytest.mark.gpu
def test_python_handles_and_lists(gpu, monkeypatch):
    monkeypatch.delenv("WFA_HIP_DEL_MAX_READS", raising=False)
    e = expectation()
    refs, W = e["refs"], e["W"]
    wa = WavefrontAligner(**KW)
    rows = expected_deletions(1, 500)
    with wa.sequence_set(refs) as G:
        p = wa.pileup(e["reads"], G, deletions=True, **window_kw(W))
        plain = wa.pileup(e["reads"], G, **window_kw(W))
        both = wa.pileup(e["reads"], G, deletions=True, insertions=True, strands=True, min_score=-60, **window_kw(W))
        for texts in (G, refs):
            s = p.deletions(texts)
            assert tuple(s) == p.DELETION_COLUMNS and all(s[k].dtype == np.int32 for k in p.DELETION_COLUMNS)
            assert np.array_equal(stacked(s, p.DELETION_COLUMNS), rows)
            s = p.deletions(texts, STAGE, 250, 2650, min_depth=8, min_frac=0.2)
            w = in_range(expected_deletions(8, 200), STAGE, 250, 2400)
            assert len(w) >= 7 and np.array_equal(stacked(s, p.DELETION_COLUMNS), w)
            assert np.array_equal(stacked(p.deletions(texts, min_frac=0), p.DELETION_COLUMNS), expected_deletions(1, 0))     # the majority rule
            assert len(p.deletions(texts, 5)["pos"]) == 0
            # the deleted letters are the reference's
            j, pos, n = e["planted"]["d"]
            k = [(int(a), int(b)) for a, b in zip(s["j"], s["pos"])].index((j, pos))
            assert s["allele_len"][k] == n == 70 and len(refs[j][pos:pos + s["allele_len"][k]]) == 70
        for j in range(len(refs)):
            assert np.array_equal(p.deletion_starts(j), e["starts"][j]) and np.array_equal(p.counts(j), plain.counts(j)), j
        assert np.array_equal(p.deletion_starts(STAGE, 900, 920), e["starts"][STAGE][900:920])
        # with a score bar, beside insertions and strands
        keep = np.asarray(e["o"]["score"]) >= -60
        assert 20 <= (~keep).sum() <= len(keep) - 500
        lens = [len(r) for r in refs]
        tables, _ = expected_tables(lens, e["o"], e["pats"], W["j"], W["t_start"], W["t_len"], keep)
        records = records_of(e["per_pair"], W, len(lens), keep)
        assert np.array_equal(stacked(both.deletions(G, min_frac=0.2), p.DELETION_COLUMNS), all_rows(tables, starts_of(records, refs), records, 1, 200))
        for call in (lambda: plain.deletions(refs), lambda: plain.deletion_starts(0), lambda: plain.deletions(G, 0)):
            with pytest.raises(ValueError, match="was not made to track deletions"):
                call()
        both.close()
    for bad, pattern in ((dict(j=6), "j = 6 is out of range for 6 text sequences"), (dict(j=0, start=5, stop=2501), r"rows \[5, 2501\) are out of range"),
                         (dict(j=0, min_depth=0), "min_depth = 0 is out of range"), (dict(min_frac=-0.1), "min_frac"), (dict(min_frac=1.2), "min_frac"),
                         (dict(start=3), "start and stop go with one text")):
        with pytest.raises(ValueError, match=pattern):
            p.deletions(refs, **bad)
    p.close()
    plain.close()
    with pytest.raises(ValueError, match="pileup is closed"):
        p.deletions(refs)
    with pytest.raises(ValueError, match="pileup is closed"):
        p.deletion_starts(0)


LEFT = "TGCATCGATTCGAGCTAGCTTGACCGTATCGGATCCGTAGCTTGCAAGTCCGTTAGCGTC"     # 60 bases, no A at its end
RIGHT = "CTGGATCCTAGGCTTAGCGATCGTAGGCTAACGTTAGCGTTCAGGCTTAACGGATTCGCT"   # 60 bases, no A at its start


@pytest.mark.gpu
def test_left_aligned_a_homopolymer_deletion_is_one_row(gpu, monkeypatch):
    """Twelve reads over a two-base deletion in A9 at [60, 69): seven plain ones, three with a substitution inside the run, two that end
    inside it (their gap lies behind their last M: no record).  WFA's own strings put every gap at the right end of the run, base 67;
    left-aligned, the plain reads give the one row a caller expects, at base 60, and a read with a substitution stops at it, a row of
    its own under a low min_frac.  The expected rows come from left_align_ops's rule applied to the oracle's strings."""
    monkeypatch.delenv("WFA_HIP_DEL_MAX_READS", raising=False)
    ref = LEFT + "A" * 9 + RIGHT
    reads, rows = [], []

    def add(read, t0, t_len):
        rows.append((len(reads), 0, 0, len(read), t0, t_len, 0))
        reads.append(read)

    for k in range(7):
        add(LEFT[3 * k:] + "A" * 7 + RIGHT[:30 + 4 * k], 3 * k, 60 - 3 * k + 9 + 30 + 4 * k)
    for k, mid in enumerate(("AATAAAA", "AAAACAA", "AAAAAGA")):
        add(LEFT[5 + k:] + mid + RIGHT[:40 + k], 5 + k, 60 - 5 - k + 9 + 40 + k)
    for k, n in enumerate((3, 5)):                     # n As of the read against n + 2 of the run: the window ends inside the run
        add(LEFT[10 + k:] + "A" * n, 10 + k, 60 - 10 - k + n + 2)
    W = as_list(rows)
    pats, txts = materialise(reads, [ref], W)
    kw = dict(span="end-to-end")
    o = loader.run(loader.oracle(), loader.make_config(**kw), datagen.from_strings(pats, txts, upper=True))
    assert (o["status"] == 0).all()
    moved = dict(cigars=[py_left_align(ops, p.encode(), t.encode())[0] for ops, p, t in zip(o["cigars"], pats, txts)], status=o["status"])
    want = {}
    for name, res in (("left", moved), ("wfa", o)):
        tables, _ = expected_tables([len(ref)], res, pats, W["j"], W["t_start"], W["t_len"])
        records = records_of([py_ops_deletions(ops) for ops in res["cigars"]], W, 1)
        starts = starts_of(records, [ref])
        want[name] = tables[0], starts[0], {pm: all_rows(tables, starts, records, 1, pm) for pm in (1, 500)}
    left, wfa = want["left"][2], want["wfa"][2]
    assert left[500].tolist() == [[0, 60, 12, 7, 7, 2, 1, 0]] and wfa[500].tolist() == [[0, 67, 10, 10, 10, 2, 1, 0]] == wfa[1].tolist()
    assert [int(r[1]) for r in left[1]] == [60, 63, 65, 66] and want["left"][1].sum() == 10 == want["wfa"][1].sum()
    wa = WavefrontAligner(**kw)
    try:
        with wa.sequence_set([ref]) as G:
            for texts in (G, [ref]):
                with wa.pileup(reads, texts, deletions=True, left_align=True, **window_kw(W)) as p, wa.pileup(reads, texts, deletions=True, **window_kw(W)) as q:
                    for pile, (table, starts, by_pm) in ((p, want["left"]), (q, want["wfa"])):
                        assert np.array_equal(pile.counts(0), table) and np.array_equal(pile.deletion_starts(0), starts)
                        for pm, w in by_pm.items():
                            assert np.array_equal(stacked(pile.deletions(texts, min_frac=pm / 1000), pile.DELETION_COLUMNS), w), pm
    finally:
        wa.close()
