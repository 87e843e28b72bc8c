"""Base qualities in the pileup on the GPU (wfa_hip_qualset_create, wfa_hip_pileup_track_qualities / _add_quals / _read_quality /
_genotypes_quals, pileup(qualities=), Pileup.quality_sums, Pileup.genotypes(qualities=True)): the device must equal, exactly, the
tables built from the ORACLE's op strings and the NumPy rule of qual_common — never the device's own counts — on the corpus of
calls_common and on a list of small pairs made for the rounds of the walk."""
import ctypes
import json
import os

import numpy as np
import pytest

from common import configs_pair
from genotype_common import in_range, left_aligned
from qual_common import (COLS, GENO_PARAMS, PARAMS, corpus_case, edge_case, fastq, py_genotypes_quals_all, tables_q)
from pywfa_amd import QualitySet, WavefrontAligner, _native
from test_windows_gpu import native_set, native_windows

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILL = -7


def native_quals(al, reads_set, quals):
    length = np.array([len(q) for q in quals], np.int32)
    off = np.zeros(len(quals), np.int64)
    off[1:] = np.cumsum(length[:-1])
    return al.qualset(reads_set, np.concatenate(quals) if quals else np.zeros(0, np.uint8), off, length)


class Rig:
    """An aligner, the sets, the quality set and a pileup of one list (qual_common.Case) at the C ABI binding.  `parts`: the list is
    added in that many pieces; `strands` / `insertions` / `qualities`: what the pileup tracks; `keep`: a mask over the list."""

    def __init__(self, case, parts=1, strands=False, insertions=False, qualities=True, keep=None):
        self.case = case
        _, nc = configs_pair(**case.kw)
        self.al = _native.Aligner(nc)
        self.ps, self.ts = native_set(self.al, case.reads), native_set(self.al, case.refs)
        self.qs = native_quals(self.al, self.ps, case.quals)
        self.pile = self.make(strands, insertions, qualities)
        n = len(case.W["i"])
        cuts = [n * k // parts for k in range(parts + 1)]
        self.batches = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = {k: v[lo:hi] for k, v in case.W.items()}
            rb = native_windows(self.al, self.ps, self.ts, part)
            rb.run()
            self.batches.append((rb, part, None if keep is None else keep[lo:hi]))

    def make(self, strands, insertions, qualities):
        pile = self.al.pileup(self.ts)
        if insertions:
            pile.track_insertions(True)
        if strands:
            pile.track_strands(True)
        if qualities:
            pile.track_qualities(True)
        return pile

    def add_all(self, mbq=0, cap=40, pile=None):
        pile = self.pile if pile is None else pile
        for rb, part, keep in self.batches:
            if pile.qualities:
                pile.add_quals(rb, part["j"], self.qs, part["i"], part["t_start"], keep, part["reverse"], part["p_start"], mbq, cap)
            elif pile.strands:
                pile.add(rb, part["j"], part["t_start"], keep, part["reverse"])
            else:
                pile.add(rb, part["j"], part["t_start"], keep)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.al.close()
        return False

    def check(self, want, ctx, pile=None):
        """Every sequence whole: counts, quality sums and, on a pileup with strands, the forward counts."""
        pile = self.pile if pile is None else pile
        counts, qsums, fwd = want
        for j in range(len(self.case.refs)):
            got = pile.read(j)
            assert got.dtype == np.int32 and np.array_equal(got, counts[j]), (ctx, "counts", j, np.argwhere(got != counts[j])[:5])
            got = pile.read_quality(j)
            assert got.dtype == np.int32 and got.shape == counts[j].shape
            assert np.array_equal(got, qsums[j]), (ctx, "quality sums", j, np.argwhere(got != qsums[j])[:5])
            if pile.strands:
                got = pile.read(j, strand=0)
                assert np.array_equal(got, fwd[j]), (ctx, "forward", j, np.argwhere(got != fwd[j])[:5])

    def bytes_of(self, pile=None):
        pile = self.pile if pile is None else pile
        return b"".join(pile.read(j).tobytes() + pile.read_quality(j).tobytes() for j in range(len(self.case.refs)))


# ---- tables -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("case", [corpus_case, edge_case])
def test_tables_under_every_parameter_pair_in_pieces_and_after_a_clear(gpu, case, parts):
    c = case()
    if case is edge_case:
        assert (np.asarray(c.o["status"]) == 0).all()          # no pair of the added list drops out
    with Rig(c, parts) as rig:
        plain = rig.make(False, False, False)
        rig.add_all(pile=plain)
        for mbq, cap in PARAMS:
            want = c.tables(mbq, cap)
            assert sum(int(t.sum()) for t in want[1]) > 0 or mbq == 93
            rig.pile.clear()
            rig.add_all(mbq, cap)
            rig.check(want, (mbq, cap))
            first = rig.bytes_of()
            if mbq == 0:                                                               # byte for byte the plain pileup's table
                assert all(rig.pile.read(j).tobytes() == plain.read(j).tobytes() for j in range(len(c.refs)))
            else:
                assert any(rig.pile.read(j).tobytes() != plain.read(j).tobytes() for j in range(len(c.refs)))
            rig.pile.clear()
            zero = [np.zeros_like(t) for t in want[0]]
            rig.check((zero, zero, zero), "cleared")
            rig.add_all(mbq, cap)
            assert rig.bytes_of() == first, (mbq, cap)
        start, length = (1001, 1333) if case is corpus_case else (37, 1000)
        got = rig.pile.read_quality(0, start, length)
        assert got.shape == (length, 8) and np.array_equal(got, c.tables(*PARAMS[-1])[1][0][start:start + length])


@pytest.mark.gpu
def test_keep_mask(gpu):
    c = corpus_case()
    score, ok = np.asarray(c.o["score"]), np.asarray(c.o["status"]) == 0
    keep = score >= int(np.median(score[ok]))            # what pileup(min_score=) passes
    assert 0 < keep[ok].sum() < ok.sum()
    with Rig(c, 2, strands=True, keep=keep) as rig:
        rig.add_all(13, 40)
        want = tables_q(c.lens, c.o, c.pats, c.W, c.quals, 13, 40, keep)
        assert not np.array_equal(want[1][0], c.tables(13, 40)[1][0])
        rig.check(want, "keep")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [corpus_case, edge_case])
@pytest.mark.parametrize("strands,insertions", [(True, False), (False, True), (True, True)])
def test_with_strands_and_insertions(gpu, case, strands, insertions):
    """The forward table (the filter included) and the insertion log; at min_base_quality 0 both are those of the same pileup
    without qualities."""
    c = case()
    with Rig(c, 2, strands, insertions) as rig:
        rig.add_all(13, 40)
        rig.check(c.tables(13, 40), "13, 40")
        rig.pile.clear()
        rig.add_all(0, 93)
        rig.check(c.tables(0, 93), "0, 93")
        plain = rig.make(strands, insertions, False)
        rig.add_all(pile=plain)
        for j in range(len(c.refs)):
            assert rig.pile.read(j).tobytes() == plain.read(j).tobytes()
            if strands:
                assert rig.pile.read(j, strand=0).tobytes() == plain.read(j, strand=0).tobytes()
        if insertions:
            assert rig.pile.insertion_stats() == plain.insertion_stats() and plain.insertion_stats()[0] > 0
            for md, pm in ((1, 500), (1, 0)):
                a, b = rig.pile.insertions(rig.ts, min_depth=md, min_permille=pm), plain.insertions(rig.ts, min_depth=md, min_permille=pm)
                assert a[0] == b[0] > 0 and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[3].tobytes() == b[3].tobytes(), (md, pm)
            # the log does not depend on the qualities: a filter that removes every M and X leaves it as it is
            rig.pile.clear()
            rig.add_all(93, 93)
            assert rig.pile.insertion_stats() == plain.insertion_stats()


@pytest.mark.gpu
def test_left_aligned(gpu):
    """The op strings left-aligned on the device, then piled up with everything tracked: the oracle's strings left-aligned by the
    Python rule (leftalign_common), under the NumPy rule."""
    c = corpus_case()
    o = left_aligned()[0]
    want = tables_q(c.lens, o, c.pats, c.W, c.quals, 13, 40)
    assert any(not np.array_equal(t, u) for t, u in zip(want[1], c.tables(13, 40)[1]))
    with Rig(c, 1, True, True) as rig:
        for rb, _, _ in rig.batches:
            rb.left_align()
        rig.add_all(13, 40)
        rig.check(want, "left-aligned")


# ---- genotypes ----------------------------------------------------------------------------------------------------------------------

def geno(rig, params, seq=-1, start=0, length=-1, cap=None, pile=None):
    pile = rig.pile if pile is None else pile
    count = ctypes.c_int64(-1)
    L = _native.lib()
    if cap is None:
        assert L.wfa_hip_pileup_genotypes_quals(pile._h, rig.ts._h, seq, start, length, *params, 0, ctypes.byref(count), None) == _native.OK, rig.al.error()
        cap = count.value
    rows = np.full((cap, COLS), FILL, np.int32)
    rc = L.wfa_hip_pileup_genotypes_quals(pile._h, rig.ts._h, seq, start, length, *params, cap, ctypes.byref(count), rows.ctypes.data if cap else None)
    assert rc == _native.OK, rig.al.error()
    return count.value, rows


@pytest.mark.gpu
@pytest.mark.parametrize("strands", [True, False])
def test_genotypes_quals(gpu, strands):
    c = corpus_case()
    with Rig(c, 1, strands) as rig:
        for mbq, cap in PARAMS[:2]:
            rig.pile.clear()
            rig.add_all(mbq, cap)
            counts, qsums, fwd = c.tables(mbq, cap)
            differ = 0
            for params in GENO_PARAMS:
                if params[3] > 0 and not strands:
                    continue
                want = py_genotypes_quals_all(counts, qsums, fwd if strands else None, c.refs, params)
                count, rows = geno(rig, params)
                assert count == len(want) and np.array_equal(rows, want), (params, mbq, cap, count, len(want))
                n = len(want)
                for k in (0, n - 1, n + 5) if n else (0, 5):
                    count, rows = geno(rig, params, cap=k)
                    m = min(k, n)
                    assert count == n and np.array_equal(rows[:m], want[:m]) and (rows[m:] == FILL).all(), (params, k)
                count, rows = geno(rig, params, 2, 1001, 2333)
                w = in_range(want, 2, 1001, 2333)
                assert count == len(w) and np.array_equal(rows, w), params
                # the plain genotypes of the same tables: the same rows, other costs
                pc, prows = rig.pile.genotypes(rig.ts, -1, 0, -1, *params)
                assert pc == n and np.array_equal(prows[:, :8], want[:, :8]) and np.array_equal(prows[:, 12:], want[:, 12:])
                differ += int((prows[:, 8:12] != want[:, 8:12]).any())
            assert differ > 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals_launch_and_write_nothing(gpu):
    """tests/golden/quality_refusals.json, "device": the code and wfa_hip_last_error of every refused call; no table changes."""
    with open(os.path.join(GOLD, "quality_refusals.json")) as f:
        golden = json.load(f)["device"]
    c = corpus_case()
    with Rig(c, 2, strands=True) as rig:
        rig.add_all(13, 40)
        L, al, pile, ts, qs = _native.lib(), rig.al, rig.pile, rig.ts, rig.qs
        rb, part, _ = rig.batches[0]
        part = {k: np.array(v, np.uint8 if k == "reverse" else np.int32) for k, v in part.items()}
        before = rig.bytes_of()
        plain = rig.make(False, False, False)
        _, nc = configs_pair(**c.kw)
        al2 = _native.Aligner(nc)
        ps2 = native_set(al2, c.reads[:2])
        qs2 = native_quals(al2, ps2, c.quals[:2])
        rows = np.full((4, COLS), FILL, np.int32)
        out = np.full((11, 8), FILL, np.int32)
        count = ctypes.c_int64(-1)
        p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data
        length = np.array([len(q) for q in c.quals], np.int32)
        off = np.zeros(len(length), np.int64)
        off[1:] = np.cumsum(length[:-1])
        blob = np.concatenate(c.quals)
        longer = length.copy()
        longer[3] += 1
        over = blob.copy()
        over[off[1] + 2] = 94
        keepalive = []

        def create(al_, set_, q, o, n):
            h = L.wfa_hip_qualset_create(al_._h, set_._h, p(q), p(o), p(n))
            assert not h
            return _native.EINVAL

        def add(pl=pile, batch=rb, quals=qs, mbq=13, cap=40, **changed):
            a = {k: np.array(v, np.uint8 if k == "reverse" else np.int32) for k, v in part.items()}   # (what the binding would pass)
            for k, (pos, v) in changed.items():
                if pos is None:
                    a[k] = None
                else:
                    a[k][pos] = v
            keepalive.append(a)
            return L.wfa_hip_pileup_add_quals(pl._h, batch._h, p(a["j"]), p(a["t_start"]), None, p(a["reverse"]), None if quals is None else quals._h,
                                              p(a["i"]), p(a["p_start"]), mbq, cap)

        calls = {
            "qualset: a set of another aligner": lambda: create(al, ps2, blob, off, length),
            "qualset: missing qualities": lambda: create(al, rig.ps, None, off, length),
            "qualset: missing lengths": lambda: create(al, rig.ps, blob, off, None),
            "qualset: entry 3 one value longer": lambda: create(al, rig.ps, blob, off, longer),
            "qualset: 94 at position 2 of entry 1": lambda: create(al, rig.ps, over, off, length),
            "track: after an add": lambda: L.wfa_hip_pileup_track_qualities(pile._h, 0),
            "add_quals: a pileup that does not track": lambda: add(pl=plain),
            "add_quals: a quality set of another aligner": lambda: add(quals=qs2),
            "add_quals: no quality set": lambda: add(quals=None),
            "add_quals: i missing": lambda: add(i=(None, 0)),
            "add_quals: i[5] = 2400": lambda: add(i=(5, 2400)),
            "add_quals: i[5] = -1": lambda: add(i=(5, -1)),
            "add_quals: p_start[4] = -1": lambda: add(p_start=(4, -1)),
            "add_quals: p_start[7] = 3": lambda: add(p_start=(7, 3)),
            "add_quals: min_base_quality = 94": lambda: add(mbq=94),
            "add_quals: min_base_quality = -1": lambda: add(mbq=-1),
            "add_quals: quality_cap = 0": lambda: add(cap=0),
            "add_quals: quality_cap = 94": lambda: add(cap=94),
            "add_quals: j[5] = 6": lambda: add(j=(5, 6)),
            "add_quals: j missing": lambda: add(j=(None, 0)),
            "add: a pileup that tracks qualities": lambda: L.wfa_hip_pileup_add(pile._h, rb._h, p(part["j"]), p(part["t_start"]), None),
            "add_strands: a pileup that tracks qualities":
                lambda: L.wfa_hip_pileup_add_strands(pile._h, rb._h, p(part["j"]), p(part["t_start"]), None, p(part["reverse"])),
            "read_quality: a pileup that does not track": lambda: L.wfa_hip_pileup_read_quality(plain._h, 0, 0, 4, out.ctypes.data),
            "read_quality: rows behind the end": lambda: L.wfa_hip_pileup_read_quality(pile._h, 0, 2990, 11, out.ctypes.data),
            "read_quality: null output": lambda: L.wfa_hip_pileup_read_quality(pile._h, 0, 0, 4, None),
            "genotypes_quals: a pileup that does not track":
                lambda: L.wfa_hip_pileup_genotypes_quals(plain._h, ts._h, -1, 0, -1, 1, 500, 20, 0, 4, ctypes.byref(count), rows.ctypes.data),
            "genotypes_quals: err_q = 0":
                lambda: L.wfa_hip_pileup_genotypes_quals(pile._h, ts._h, -1, 0, -1, 1, 500, 0, 0, 4, ctypes.byref(count), rows.ctypes.data),
        }
        try:
            assert [g["case"] for g in golden] == list(calls)
            for g in golden:
                assert calls[g["case"]]() == _native.EINVAL, g
                assert al.error() == g["last_error"], (g, al.error())
                assert (rows == FILL).all() and (out == FILL).all() and count.value == -1, g
            assert rig.bytes_of() == before and all((plain.read(j) == 0).all() for j in range(len(c.refs)))
            # the pileup is usable afterwards, and tracking may change once it is empty
            assert add() == _native.OK
            pile.clear()
            pile.track_qualities(False)
            pile.add(rb, part["j"], part["t_start"], None, part["reverse"])
            assert L.wfa_hip_pileup_read_quality(pile._h, 0, 0, 4, out.ctypes.data) == _native.EINVAL and (out == FILL).all()
        finally:
            al2.close()


# ---- from Python --------------------------------------------------------------------------------------------------------------------

def stacked(d, names):
    return np.stack([d[k] for k in names], axis=1)


@pytest.mark.gpu
def test_python_lists_handles_and_messages(gpu):
    with open(os.path.join(GOLD, "quality_refusals.json")) as f:
        golden = {g["case"]: g["message"] for g in json.load(f)["python"]}
    c = corpus_case()
    W = c.W
    kw = dict(i=W["i"], j=W["j"], pattern_start=W["p_start"], pattern_len=W["p_len"], text_start=W["t_start"], text_len=W["t_len"], reverse=W["reverse"])
    strings = [fastq(q) for q in c.quals]
    wa = WavefrontAligner(**c.kw)
    counts, qsums, fwd = c.tables(13, 40)
    with wa.sequence_set(c.reads) as P, wa.sequence_set(c.refs) as G:
        with wa.quality_set(P, strings) as Q:
            assert isinstance(Q, QualitySet) and len(Q) == len(c.reads)
            for qualities, patterns, extra in ((strings, c.reads, {}), (Q, P, dict(strands=True, insertions=True)), (list(c.quals), P, {})):
                with wa.pileup(patterns, G, qualities=qualities, min_base_quality=13, quality_cap=40, **extra, **kw) as p:
                    for j in range(len(c.refs)):
                        assert np.array_equal(p.counts(j), counts[j]), j
                        s = p.quality_sums(j)
                        assert s.dtype == np.int32 and s.shape == (len(c.refs[j]), 8) and np.array_equal(s, qsums[j]), j
                    assert np.array_equal(p.quality_sums(2, 1001, 3334), qsums[2][1001:3334])
                    g = p.genotypes(G, qualities=True)
                    assert tuple(g) == p.GENOTYPE_COLUMNS and all(v.dtype == np.int32 and v.flags.c_contiguous for v in g.values())
                    want = py_genotypes_quals_all(counts, qsums, fwd if extra else None, c.refs, (8, 200, 20, 0))
                    assert np.array_equal(stacked(g, p.GENOTYPE_COLUMNS), want)
            # the defaults: no filter, a cap of 40; offset 64 through quality_set
            with wa.quality_set(c.reads, [(q.astype(np.int32) + 64).astype(np.uint8).tobytes() for q in c.quals], offset=64) as Q64:
                with wa.pileup(P, G, qualities=Q64, **kw) as p:
                    assert np.array_equal(p.quality_sums(1), c.tables(0, 40)[1][1]) and np.array_equal(p.counts(1), c.tables(0, 40)[0][1])
            with wa.pileup(P, G, **kw) as plain, wa.quality_set(c.reads[:2], strings[:2]) as other:
                closed = wa.quality_set(P, strings)
                closed.close()
                calls = {
                    "min_base_quality without qualities": lambda: wa.pileup(P, G, min_base_quality=13, **kw),
                    "quality_cap without qualities": lambda: wa.pileup(P, G, quality_cap=30, **kw),
                    "min_base_quality = 94": lambda: wa.pileup(P, G, qualities=Q, min_base_quality=94, **kw),
                    "min_base_quality = 2.5": lambda: wa.pileup(P, G, qualities=Q, min_base_quality=2.5, **kw),
                    "quality_cap = 0": lambda: wa.pileup(P, G, qualities=Q, quality_cap=0, **kw),
                    "one entry for 2400 reads": lambda: wa.pileup(P, G, qualities=strings[:1], **kw),
                    "entry 3 one value longer": lambda: wa.pileup(P, G, qualities=strings[:3] + [strings[3] + "I"] + strings[4:], **kw),
                    "a space in entry 1": lambda: wa.pileup(P, G, qualities=strings[:1] + [strings[1][:2] + " " + strings[1][3:]] + strings[2:], **kw),
                    "a quality set of other reads": lambda: wa.pileup(P, G, qualities=other, **kw),
                    "a closed quality set": lambda: wa.pileup(P, G, qualities=closed, **kw),
                    "genotypes(qualities=True) without qualities": lambda: plain.genotypes(G, qualities=True),
                    "quality_sums without qualities": lambda: plain.quality_sums(0),
                }
                assert list(calls) == list(golden)
                for case, call in calls.items():
                    with pytest.raises(ValueError) as info:
                        call()
                    assert str(info.value) == golden[case], case
