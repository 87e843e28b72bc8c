"""The per-strand pileup and the genotyped sites on the GPU (wfa_hip_pileup_track_strands / _add_strands / _read_strand / _genotypes,
pileup(strands=True), Pileup.counts(strand=), Pileup.genotypes): the device must equal, exactly, the tables built from the ORACLE's op
strings (the forward ones from the pairs with reverse == 0) and the Python restatement of the rule (genotype_common) applied to THOSE
tables — never to the device's own counts."""
import ctypes

import numpy as np
import pytest

from calls_common import KW, expectation
from common import configs_pair
from genotype_common import COLS, PARAMS, expected_genotypes, forward_tables, in_range, left_aligned, py_genotypes_all, tables_of
from pywfa_amd import WavefrontAligner, _native
from test_calls_gpu import RANGES
from test_windows_gpu import native_set, native_windows

FILL = -7


class Rig:
    """An aligner, the two sets and a pileup of the corpus at the C ABI binding.  `parts`: the list added in that many pieces;
    `strands` / `insertions`: what the pileup tracks; `keep`: a mask over the list; `reverse`: False passes NULL (every pair forward)."""

    def __init__(self, parts=1, strands=True, insertions=False, keep=None, reverse=True):
        e = expectation()
        self.e = e
        _, nc = configs_pair(**KW)
        self.al = _native.Aligner(nc)
        self.ps, self.ts = native_set(self.al, e["reads"]), native_set(self.al, e["refs"])
        self.pile = self.al.pileup(self.ts)
        if insertions:
            self.pile.track_insertions(True)
        if strands:
            self.pile.track_strands(True)
        self.strands = strands
        n = len(e["W"]["i"])
        cuts = [n * k // parts for k in range(parts + 1)]
        self.batches = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = {k: v[lo:hi] for k, v in e["W"].items()}
            rb = native_windows(self.al, self.ps, self.ts, part)
            rb.run()
            self.batches.append((rb, part, None if keep is None else keep[lo:hi]))
        self.add_all(reverse)

    def add_all(self, reverse=True, pile=None):
        pile = self.pile if pile is None else pile
        for rb, part, keep in self.batches:
            if pile.strands:
                pile.add(rb, part["j"], part["t_start"], keep, part["reverse"] if reverse else None)
            else:
                pile.add(rb, part["j"], part["t_start"], keep)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.al.close()
        return False

    def check_tables(self, total, fwd, ctx):
        """Every sequence whole, through wfa_hip_pileup_read and _read_strand."""
        for j in range(len(self.e["refs"])):
            got = self.pile.read(j)
            assert np.array_equal(got, total[j]), (ctx, j, np.argwhere(got != total[j])[:5])
            plus, minus = self.pile.read(j, strand=0), self.pile.read(j, strand=1)
            assert plus.dtype == np.int32 and plus.shape == got.shape
            assert np.array_equal(plus, fwd[j]), (ctx, "+", j, np.argwhere(plus != fwd[j])[:5])
            assert np.array_equal(plus + minus, got) and (minus >= 0).all(), (ctx, "-", j)

    def geno(self, params, seq=-1, start=0, length=-1, cap=None, ts=None):
        """wfa_hip_pileup_genotypes on rows prefilled with FILL: (count, rows); cap None: the counting call first."""
        ts = self.ts if ts is None else ts
        count = ctypes.c_int64(-1)
        L = _native.lib()
        if cap is None:
            assert L.wfa_hip_pileup_genotypes(self.pile._h, ts._h, seq, start, length, *params, 0, ctypes.byref(count), None) == _native.OK, self.al.error()
            cap = count.value
        rows = np.full((cap, COLS), FILL, np.int32)
        rc = L.wfa_hip_pileup_genotypes(self.pile._h, ts._h, seq, start, length, *params, cap, ctypes.byref(count), rows.ctypes.data if cap else None)
        assert rc == _native.OK, self.al.error()
        return count.value, rows


# ---- tables and strand reads --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("parts", [1, 3])
def test_strand_tables_in_pieces_ranges_and_after_a_clear(gpu, parts):
    """Reads of 100-200 ops cross the 64-op round of the walk; every second read is reverse."""
    with Rig(parts=parts) as rig:
        e, fwd = rig.e, forward_tables()
        assert sum(int(f.sum()) for f in fwd) > 0 and any(not np.array_equal(f, t) for f, t in zip(fwd, e["tables"]))
        rig.check_tables(e["tables"], fwd, "first")
        for seq, start, length in RANGES:
            for strand in (0, 1):
                got = rig.pile.read(seq, start, length, strand=strand)
                f, t = fwd[seq][start:start + length], e["tables"][seq][start:start + length]
                assert got.shape == (length, 8) and np.array_equal(got, f if strand == 0 else t - f), (seq, start, length, strand)
        # clear keeps the setting and zeroes both tables
        rig.pile.clear()
        zero = [np.zeros_like(t) for t in e["tables"]]
        rig.check_tables(zero, zero, "cleared")
        rig.add_all()
        rig.check_tables(e["tables"], fwd, "again")
        # integer adds: the list a second time doubles both
        rig.add_all()
        rig.check_tables([2 * t for t in e["tables"]], [2 * f for f in fwd], "twice")


@pytest.mark.gpu
def test_keep_and_all_forward(gpu):
    e = expectation()
    score = np.asarray(e["o"]["score"])
    ok = np.asarray(e["o"]["status"]) == 0
    keep = score >= int(np.median(score[ok]))            # what pileup(min_score=) passes
    assert 0 < keep[ok].sum() < ok.sum()
    with Rig(parts=2, keep=keep) as rig:
        total, fwd = tables_of(e["o"], keep, e["W"]["reverse"])
        assert not np.array_equal(total[0], e["tables"][0])
        rig.check_tables(total, fwd, "keep")
        # reverse = NULL: every pair is forward, forward equals total
        rig.pile.clear()
        rig.add_all(reverse=False)
        rig.check_tables(total, total, "all forward")


@pytest.mark.gpu
def test_with_insertions_and_left_aligned(gpu):
    """Both kinds of tracking on: the tables hold, and the insertion rows are those of a pileup that tracks insertions only."""
    with Rig(insertions=True) as rig:
        e = rig.e
        rig.check_tables(e["tables"], forward_tables(), "tracked")
        plain = rig.al.pileup(rig.ts)
        plain.track_insertions(True)
        rig.add_all(pile=plain)
        assert rig.pile.insertion_stats() == plain.insertion_stats() and plain.insertion_stats()[0] > 0
        for md, pm in ((1, 500), (8, 200), (1, 0)):
            a, b = rig.pile.insertions(rig.ts, min_depth=md, min_permille=pm), plain.insertions(rig.ts, min_depth=md, min_permille=pm)
            assert a[0] == b[0] > 0 and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[3].tobytes() == b[3].tobytes(), (md, pm)
        # the op strings left-aligned on the device, then piled up: the oracle's strings left-aligned by the Python rule
        o, total, fwd = left_aligned()
        assert any(not np.array_equal(t, u) for t, u in zip(total, e["tables"]))
        for rb, _, _ in rig.batches:
            rb.left_align()
        rig.pile.clear()
        rig.add_all()
        rig.check_tables(total, fwd, "left-aligned")


@pytest.mark.gpu
def test_a_pileup_without_strands_is_as_before(gpu):
    with Rig(strands=False) as rig:
        e = rig.e
        for j, t in enumerate(e["tables"]):
            assert np.array_equal(rig.pile.read(j), t), j
        out = np.full((4, 8), FILL, np.int32)
        rc = _native.lib().wfa_hip_pileup_read_strand(rig.pile._h, 0, 0, 4, 0, out.ctypes.data)
        assert rc == _native.EINVAL and "was not made to track strands" in rig.al.error() and (out == FILL).all()
        # genotypes without strands: the last four columns are -1, the rest as on a tracking pileup
        for params in (PARAMS[0], PARAMS[1], PARAMS[3]):
            want = expected_genotypes(params, False)
            count, rows = rig.geno(params)
            assert count == len(want) and np.array_equal(rows, want), params
            assert (rows[:, 12:] == -1).all() and np.array_equal(rows[:, :12], expected_genotypes(params)[:, :12])


# ---- genotypes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("chunk", ["64", "192", None])
def test_genotypes_over_chunks_parameters_ranges_and_capacities(gpu, monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("WFA_HIP_CALLS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("WFA_HIP_CALLS_CHUNK", chunk)
    with Rig() as rig:
        e = rig.e
        for params in PARAMS:
            want = expected_genotypes(params)
            count, rows = rig.geno(params)
            assert count == len(want) and np.array_equal(rows, want), (params, count, len(want), np.argwhere(rows != want)[:5] if count == len(want) else None)
            again = rig.geno(params)
            assert again[0] == count and again[1].tobytes() == rows.tobytes()                # two calls, identical bytes
            for seq, start, length in RANGES:
                count, rows = rig.geno(params, seq, start, length)
                w = in_range(want, seq, start, length)
                assert count == len(w) and np.array_equal(rows, w), (params, seq, start, length, count, len(w))
            n = len(want)
            for cap in (0, n - 1, n, n + 5) if n else (0, 5):
                count, rows = rig.geno(params, cap=cap)
                k = min(cap, n)
                assert count == n and np.array_equal(rows[:k], want[:k]) and (rows[k:] == FILL).all(), (params, cap)
            if params[3] == 0:                                                                # the site rows of the same process
                sc, srows = rig.pile.sites(rig.ts, min_depth=params[0], min_permille=params[1])
                assert sc == len(want) and np.ascontiguousarray(want[:, :8]).tobytes() == srows.tobytes(), params
        assert len(expected_genotypes(PARAMS[2])) < len(expected_genotypes(PARAMS[1]))        # the strand filter bites
        # the set closed, and opened again from the same sequences
        rig.ts.close()
        reopened = native_set(rig.al, e["refs"])
        for params in (PARAMS[1], PARAMS[2]):
            want = expected_genotypes(params)
            count, rows = rig.geno(params, ts=reopened)
            assert count == len(want) and np.array_equal(rows, want), params
        # cleared: nothing is covered, nothing is written
        rig.pile.clear()
        count, rows = rig.geno(PARAMS[0], ts=reopened, cap=4)
        assert count == 0 and (rows == FILL).all()


@pytest.mark.gpu
def test_genotypes_after_keep_and_two_adds(gpu):
    """Tables that differ from the corpus': a keep mask, the list added twice — the rule on the oracle's tables of exactly that."""
    e = expectation()
    keep = np.arange(len(e["W"]["i"])) % 3 != 0
    with Rig(parts=2, keep=keep) as rig:
        rig.add_all()
        total, fwd = tables_of(e["o"], keep, e["W"]["reverse"])
        total, fwd = [2 * t for t in total], [2 * f for f in fwd]
        for params in (PARAMS[1], PARAMS[2]):
            want = py_genotypes_all(total, fwd, e["refs"], params)
            count, rows = rig.geno(params)
            assert count == len(want) > 0 and np.array_equal(rows, want), params
            assert not np.array_equal(want, expected_genotypes(params))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals_launch_and_write_nothing(gpu):
    with Rig() as rig:
        e, L, pile, ts = rig.e, _native.lib(), rig.pile, rig.ts
        rb, part, _ = rig.batches[0]
        rows = np.full((4, COLS), FILL, np.int32)
        out = np.full((4, 8), FILL, np.int32)
        count = ctypes.c_int64(-1)
        j, t0 = np.ascontiguousarray(part["j"], np.int32), np.ascontiguousarray(part["t_start"], np.int32)
        rev = np.ascontiguousarray(part["reverse"], np.uint8)

        def untouched():
            return (rows == FILL).all() and (out == FILL).all() and count.value == -1

        def refused(rc, pattern, al=rig.al):
            assert rc == _native.EINVAL and pattern in al.error(), (rc, al.error())
            assert untouched()

        def geno(tset, seq, start, length, md, pm, eq, mas, cap, cnt=ctypes.byref(count), rowp=rows.ctypes.data, p=pile):
            return L.wfa_hip_pileup_genotypes(p._h, tset._h, seq, start, length, md, pm, eq, mas, cap, cnt, rowp)

        before = [pile.read(k) for k in range(len(e["refs"]))]
        # the tracking state
        refused(L.wfa_hip_pileup_track_strands(pile._h, 0), "strand tracking is chosen while the pileup is empty")
        refused(L.wfa_hip_pileup_track_strands(pile._h, 1), "this one has been added to")
        refused(L.wfa_hip_pileup_add(pile._h, rb._h, j.ctypes.data, t0.ctypes.data, None), "wfa_hip_pileup_add_strands")
        plain = rig.al.pileup(ts)
        refused(L.wfa_hip_pileup_add_strands(plain._h, rb._h, j.ctypes.data, t0.ctypes.data, None, rev.ctypes.data), "was not made to track strands")
        assert (plain.read(0) == 0).all()
        refused(geno(ts, -1, 0, -1, 1, 500, 20, 1, 4, p=plain), "min_alt_strand = 1 needs a pileup made to track strands")
        refused(L.wfa_hip_pileup_read_strand(plain._h, 0, 0, 4, 0, out.ctypes.data), "was not made to track strands")
        # what wfa_hip_pileup_add refuses, in its words
        bad = j.copy()
        bad[5] = 6
        refused(L.wfa_hip_pileup_add_strands(pile._h, rb._h, bad.ctypes.data, t0.ctypes.data, None, rev.ctypes.data),
                "text index out of range at position 5 of the pair list: j = 6 over a set of 6 sequences")
        far = t0.copy()
        far[7] = 100000
        refused(L.wfa_hip_pileup_add_strands(pile._h, rb._h, j.ctypes.data, far.ctypes.data, None, rev.ctypes.data), "text window out of range at position 7")
        refused(L.wfa_hip_pileup_add_strands(pile._h, rb._h, None, t0.ctypes.data, None, rev.ctypes.data), "the text indices are missing")
        # the strand and the rows of a strand read
        for strand in (-1, 2):
            refused(L.wfa_hip_pileup_read_strand(pile._h, 0, 0, 4, strand, out.ctypes.data), f"strand = {strand} is out of range (0 forward, 1 reverse)")
        refused(L.wfa_hip_pileup_read_strand(pile._h, 0, 2990, 11, 0, out.ctypes.data), "rows [2990, 2990 + 11) of sequence 0 are out of range")
        refused(L.wfa_hip_pileup_read_strand(pile._h, 6, 0, 1, 1, out.ctypes.data), "of sequence 6 are out of range")
        refused(L.wfa_hip_pileup_read_strand(pile._h, 0, 0, 4, 0, None), "null output")
        # the parameters of the genotypes
        for eq in (0, 61, -5):
            refused(geno(ts, -1, 0, -1, 1, 500, eq, 0, 4), f"err_q = {eq} is out of range (1 .. 60)")
        refused(geno(ts, -1, 0, -1, 1, 500, 20, -1, 4), "min_alt_strand = -1 is negative")
        # whatever the sites refuse
        _, nc = configs_pair(**KW)
        al2 = _native.Aligner(nc)
        try:
            refused(geno(native_set(al2, e["refs"]), -1, 0, -1, 1, 500, 20, 0, 4), "sequence set of another aligner")
        finally:
            al2.close()
        changed = list(e["refs"])
        changed[2] = changed[2][:-1]
        refused(geno(native_set(rig.al, changed), -1, 0, -1, 1, 500, 20, 0, 4), "sequence 2 of the set has 5999 bases, the pileup was made over 6000")
        refused(geno(native_set(rig.al, e["refs"][:5]), -1, 0, -1, 1, 500, 20, 0, 4), "the set holds 5 sequences, the pileup was made over 6")
        refused(geno(ts, 0, 2990, 11, 1, 500, 20, 0, 4), "rows [2990, 2990 + 11) of sequence 0 are out of range (6 sequences; sequence length 3000)")
        refused(geno(ts, -1, 5, -1, 1, 500, 20, 0, 4), "seq = -1 (every sequence) goes with start = 0 and len = -1, got start = 5, len = -1")
        refused(geno(ts, -2, 0, -1, 1, 500, 20, 0, 4), "out of range")
        refused(geno(ts, -1, 0, -1, 0, 500, 20, 0, 4), "min_depth = 0 is out of range")
        refused(geno(ts, -1, 0, -1, 1, 0, 20, 0, 4), "min_permille = 0 is out of range (1 .. 1000)")
        refused(geno(ts, -1, 0, -1, 1, 1001, 20, 0, 4), "min_permille = 1001 is out of range (1 .. 1000)")
        refused(geno(ts, -1, 0, -1, 1, 500, 20, 0, -1), "cap = -1 is negative")
        refused(geno(ts, -1, 0, -1, 1, 500, 20, 0, 4, None), "null count")
        refused(geno(ts, -1, 0, -1, 1, 500, 20, 0, 4, ctypes.byref(count), None), "null rows")
        # nothing was added by any of it, and the pileup is usable afterwards
        for k, t in enumerate(before):
            assert np.array_equal(pile.read(k), t) and np.array_equal(t, e["tables"][k])
        assert geno(ts, -1, 0, -1, 8, 200, 20, 2, 4) == _native.OK and count.value == len(expected_genotypes(PARAMS[2]))
        assert np.array_equal(rows, expected_genotypes(PARAMS[2])[:4])
        # tracking may be changed again once the pileup is empty; turning it off makes it a plain pileup
        pile.clear()
        pile.track_strands(False)
        pile.add(rb, part["j"], part["t_start"])
        assert L.wfa_hip_pileup_read_strand(pile._h, 0, 0, 4, 0, out.ctypes.data) == _native.EINVAL and (out == FILL).all()


# ---- from Python --------------------------------------------------------------------------------------------------------------------

def stacked(d, names):
    return np.stack([d[k] for k in names], axis=1)


@pytest.mark.gpu
def test_python_handles_and_lists(gpu):
    e = expectation()
    refs, W, fwd = e["refs"], e["W"], forward_tables()
    kw = dict(i=W["i"], j=W["j"], pattern_start=W["p_start"], pattern_len=W["p_len"], text_start=W["t_start"], text_len=W["t_len"], reverse=W["reverse"])
    wa = WavefrontAligner(**KW)
    with wa.sequence_set(refs) as G:
        p = wa.pileup(e["reads"], G, strands=True, **kw)
        for j, t in enumerate(e["tables"]):
            assert np.array_equal(p.counts(j), t), j
            plus, minus = p.counts(j, strand="+"), p.counts(j, strand="-")
            assert np.array_equal(plus, fwd[j]) and np.array_equal(plus + minus, t), j
            assert np.array_equal(p.depth(j, strand="+"), fwd[j][:, :6].sum(axis=1)) and p.depth(j, strand="-").dtype == np.int32
        assert np.array_equal(p.counts(2, 1001, 3334, strand="-"), (e["tables"][2] - fwd[2])[1001:3334])
        for texts in (G, refs):
            g = p.genotypes(texts)
            assert tuple(g) == p.GENOTYPE_COLUMNS == _native.GENOTYPE_COLUMNS and all(v.dtype == np.int32 and v.flags.c_contiguous for v in g.values())
            assert np.array_equal(stacked(g, p.GENOTYPE_COLUMNS), expected_genotypes((8, 200, 20, 0)))            # the defaults
            g = p.genotypes(texts, min_depth=8, min_frac=0.2, err_q=20, min_alt_strand=2)
            assert np.array_equal(stacked(g, p.GENOTYPE_COLUMNS), expected_genotypes(PARAMS[2]))
            g = p.genotypes(texts, 2, 1001, 3334, min_depth=4, min_frac=1.0, err_q=60, min_alt_strand=1)
            assert np.array_equal(stacked(g, p.GENOTYPE_COLUMNS), in_range(expected_genotypes(PARAMS[4]), 2, 1001, 2333))
            g = p.genotypes(texts, 0, min_depth=1, min_frac=0.5)
            w = in_range(expected_genotypes(PARAMS[0]), 0, 0, 3000)
            assert len(w) > 0 and np.array_equal(stacked(g, p.GENOTYPE_COLUMNS), w)
            assert len(p.genotypes(texts, 5)["gt"]) == 0
            s = p.sites(texts, min_depth=8, min_frac=0.2)
            g = p.genotypes(texts)
            assert all(np.array_equal(s[k], g[k]) for k in p.SITE_COLUMNS)
        # reverse=None: every read counts as forward
        q = wa.pileup(e["reads"], G, strands=True, **dict(kw, reverse=None))
        assert np.array_equal(q.counts(4, strand="+"), q.counts(4)) and (q.counts(4, strand="-") == 0).all()
        q.close()
        # without the keyword: as before, and the strand forms say what is missing
        plain = wa.pileup(e["reads"], G, **kw)
        assert np.array_equal(plain.counts(0), e["tables"][0])
        for call in (lambda: plain.counts(0, strand="+"), lambda: plain.depth(0, strand="-")):
            with pytest.raises(ValueError, match="was not made to track strands"):
                call()
        with pytest.raises(ValueError, match="min_alt_strand > 0 needs a pileup made to track strands"):
            plain.genotypes(G, min_alt_strand=1)
        g = plain.genotypes(G)
        assert np.array_equal(stacked(g, plain.GENOTYPE_COLUMNS), expected_genotypes((8, 200, 20, 0), False))
        plain.close()
    for bad, pattern in ((dict(err_q=0), "err_q = 0 is out of range"), (dict(err_q=61), "err_q = 61"), (dict(err_q=2.5), "err_q"),
                         (dict(min_alt_strand=-1), "min_alt_strand = -1 is out of range"), (dict(min_frac=0), "min_frac"),
                         (dict(min_depth=0), "min_depth = 0 is out of range"), (dict(j=6), "j = 6 is out of range for 6 text sequences"),
                         (dict(start=3), "start and stop go with one text")):
        with pytest.raises(ValueError, match=pattern):
            p.genotypes(refs, **bad)
    with pytest.raises(ValueError, match="strand = 'x'"):
        p.counts(0, strand="x")
    p.close()
    with pytest.raises(ValueError, match="pileup is closed"):
        p.genotypes(refs)
    with pytest.raises(ValueError, match="pileup is closed"):
        p.counts(0, strand="+")
