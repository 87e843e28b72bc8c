"""Duplicate marking on the GPU (wfa_hip_placer_duplicates, place_pairs / place_windows(duplicates=True)): the device's rows equal the
host statement wfa_hip_duplicates_host byte for byte — on random cases in which every clause of the rule occurs, on buckets of the
sizes round the cap, on a text set whose plane needs the second round of the scan's top kernel, under WFA_HIP_POISON in a fresh child
process — and place_pairs(duplicates=True) marks exactly the copies a corpus was built with."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":   # (the poison child: the paths conftest.py sets up)
    sys.path[:0] = [os.path.join(HERE, ".."), HERE]

from common import configs_pair
from dup_common import MAX_BUCKET, as_arrays, random_dup_case, sized_dup_case
from pair_common import INT32_MIN, PAIR_COLUMNS
from place_common import COLUMNS
from pywfa_amd import WavefrontAligner, _native
from test_windows_gpu import LETTERS, as_list, revcomp

KW = dict(span="ends-free", text_begin_free=20, text_end_free=20)
PAR = dict(min_score=INT32_MIN, full_gap=24, min_insert=0, max_insert=1000, unpaired=0)
DUP_KEYS = ("dup", "dup_rep", "dup_size", "dup_overflow")


def seqset(al, lengths):
    """A resident set of sequences of the given lengths (the rule reads the lengths and the base offsets alone)."""
    lengths = np.asarray(lengths, np.int32)
    off = np.zeros(len(lengths), np.int64)
    off[1:] = np.cumsum(lengths[:-1])
    return al.seqset(np.full(max(int(lengths.sum()), 1), ord("A"), np.uint8), off, lengths)


def host(nreads, a, mates, par, text_len):
    return _native.duplicates_host(nreads, *a, mates, text_len, **par)


class Device:
    """A placer holding the first `upto` hits of one case (added in two adds) and the set of its text lengths."""

    def __init__(self, al, nreads, a, text_len, upto=None):
        self.texts = seqset(al, text_len)
        self.pl = al.placer(nreads)
        self.a = a
        n = len(a[0]) if upto is None else upto
        for lo, hi in ((0, n // 3), (n // 3, n)):
            self.add(lo, hi)

    def add(self, lo, hi):
        self.pl.add_hits(*[None if x is None else x[lo:hi] for x in self.a])

    def duplicates(self, mates, par):
        return self.pl.duplicates(self.texts, mates, **par)

    def close(self):
        self.pl.close()
        self.texts.close()


def same_rows(got, want, ctx):
    for g, w, what in zip(got, want, ("read rows", "pair rows")):
        assert g.dtype == np.int32 and g.shape == w.shape, (ctx, what, g.shape, w.shape)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0 and g.tobytes() == w.tobytes(), (ctx, what, int(bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist(), bad.size)


# reads per sized case: round a wave, round a workgroup of 256 slots and up to 2 000, never a multiple of 256
SIZED = [1, 2, 3, 63, 65, 255, 257, 511, 513, 777, 1023, 1025, 1791, 1999, 2000]


def random_cases(al):
    """About 200 cases on one aligner, so that its pool blocks are recycled from case to case: 150 small ones in which every clause
    occurs and 45 sized ones (up to 2 000 reads, text sets up to 64 kb, few places or many).  Returns the number of duplicates seen."""
    rng = np.random.default_rng(2028)
    dups = 0
    cases = [random_dup_case(rng) for _ in range(150)]
    for k, nreads in enumerate(SIZED * 3):
        text_len = [[1000, 700], [30000, 34000], [65536]][k % 3]
        hits, mates = sized_dup_case(rng, nreads, text_len, spread=(None, 7, 40)[k // len(SIZED)])
        cases.append((nreads, hits, mates, PAR, text_len))
    for k, (nreads, hits, mates, par, text_len) in enumerate(cases):
        a = as_arrays(hits)
        want = host(nreads, a, mates, par, text_len)
        d = Device(al, nreads, a, text_len)
        try:
            got = d.duplicates(mates, par)
            same_rows(got, want, ("random", k, nreads))
            again = d.duplicates(mates, par)                                            # two calls: identical bytes
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), k
        finally:
            d.close()
        dups += int(want[0][:, 2].sum())
    return dups


@pytest.mark.gpu
def test_duplicates_equal_the_host_statement_on_random_cases(gpu):
    al = _native.Aligner(configs_pair(**KW)[1])
    try:
        assert random_cases(al) >= 2000
    finally:
        al.close()


@pytest.mark.gpu
def test_duplicates_between_the_placers_other_runs_and_adds(gpu):
    """One call after run_pairs, one after a further add (the grouping is redone, the plane reused), one on a larger text set (the
    plane regrown), one in the single-end form; a pair run behind them gives what one in front gave."""
    al = _native.Aligner(configs_pair(**KW)[1])
    try:
        rng = np.random.default_rng(5)
        nreads, text_len = 999, [3000, 2000]
        hits, mates = sized_dup_case(rng, nreads, text_len, spread=9)
        a = as_arrays(hits)
        n = len(a[0])
        part = [None if x is None else x[:n // 2] for x in a]
        d = Device(al, nreads, a, text_len, upto=n // 2)
        try:
            before = d.pl.run_pairs(mates, **PAR)
            same_rows(d.duplicates(mates, PAR), host(nreads, part, mates, PAR, text_len), "after run_pairs")
            assert d.pl.kernel_ms() > 0.0
            after = d.pl.run_pairs(mates, **PAR)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
            d.add(n // 2, n)
            same_rows(d.duplicates(mates, PAR), host(nreads, a, mates, PAR, text_len), "after a further add")
            same_rows(d.duplicates(0, PAR), host(nreads, a, 0, PAR, text_len), "single-end")
            other = dict(PAR, min_score=-1, max_insert=200, unpaired=5)
            same_rows(d.duplicates(mates, other), host(nreads, a, mates, other, text_len), "other parameters")
            longer = seqset(al, [3000, 2000, 50000])
            same_rows(d.pl.duplicates(longer, mates, **PAR), host(nreads, a, mates, PAR, [3000, 2000, 50000]), "a larger text set")
            shorter = seqset(al, [3000, 2000])
            same_rows(d.pl.duplicates(shorter, mates, **PAR), host(nreads, a, mates, PAR, text_len), "the smaller one again")
            longer.close()
            shorter.close()
        finally:
            d.close()
    finally:
        al.close()


@pytest.mark.gpu
def test_bucket_sizes_round_the_cap_in_one_case(gpu):
    """Buckets of 1, 2, 64, 65, 4 096 and 4 097 units, each a mix of forward and reverse read units (two groups); only the last is
    not resolved."""
    al = _native.Aligner(configs_pair(**KW)[1])
    try:
        rng = np.random.default_rng(6)
        sizes = [1, 2, 64, 65, MAX_BUCKET, MAX_BUCKET + 1]
        rows = []
        for k, size in enumerate(sizes):
            b = 100 + 10 * k
            for _ in range(size):
                rv = int(rng.integers(0, 2))
                ln = int(rng.choice([30, 50]))
                ts, te = (b + 1 - ln, b + 1) if rv else (b, b + ln)
                rows.append((len(rows), 0, rv, -int(rng.integers(0, 4)), 0, ts, te))
        nreads = len(rows)
        rows = [rows[q] for q in rng.permutation(nreads)]
        a = as_arrays(dict(zip(("i", "j", "reverse", "score", "status", "text_start", "text_end"), zip(*rows))))
        want = host(nreads, a, 0, PAR, [1000])
        over = want[0][:, 3] == 1
        assert over.sum() == MAX_BUCKET + 1 and (want[0][over, 1] == 1).all() and sorted(set(want[0][~over, 1].tolist()))[-1] > MAX_BUCKET // 3
        d = Device(al, nreads, a, [1000])
        try:
            same_rows(d.duplicates(0, PAR), want, "bucket sizes")
        finally:
            d.close()
    finally:
        al.close()


@pytest.mark.gpu
def test_a_text_set_above_2_to_the_20_bases(gpu):
    """1 061 869 bases: the plane's 260 scan chunks reach the second round of the top scan kernel.  Units in the first bucket, in the
    last bucket of the last text, on both sides of a 4 096-counter chunk edge and of the edge between the top kernel's rounds."""
    al = _native.Aligner(configs_pair(**KW)[1])
    try:
        text_len = [3 * 4096 + 5, 1 << 20, 1000]
        off = [0, text_len[0], text_len[0] + text_len[1]]
        assert sum(text_len) + 1 > 256 * 4096
        places = [(0, 0), (2, 999), (0, 4095), (0, 4096), (1, 256 * 4096 - 1 - off[1]), (1, 256 * 4096 - off[1]), (1, 257 * 4096 - off[1]),
                  (1, text_len[1] - 1), (2, 0), (1, 0)]
        rng = np.random.default_rng(8)
        rows = []
        for j, b in places:      # three forward reads (one group), and a fragment and its copy, where there is room for them
            for _ in range(3):
                rows.append((len(rows), j, 0, -int(rng.integers(0, 3)), 0, b, b + int(rng.integers(1, 40))))
        nsingle = len(rows)
        nfrag = 0
        for j, b in places:
            if b + 300 > text_len[j]:
                continue
            for s in (-2, 0):
                r = nsingle + 2 * nfrag
                rows += [(r, j, 0, s, 0, b, b + 50), (r + 1, j, 1, -1, 0, b + 200, b + 250)]
                nfrag += 1
        nreads = len(rows)
        mates = np.arange(nsingle, nreads).reshape(-1, 2)
        rows = [rows[q] for q in rng.permutation(nreads)]
        a = as_arrays(dict(zip(("i", "j", "reverse", "score", "status", "text_start", "text_end"), zip(*rows))))
        want = host(nreads, a, mates, PAR, text_len)
        assert (want[0][:nsingle, 1] == 3).all() and (want[1][:, 1] == 2).all() and want[1][:, 2].sum() == nfrag // 2 and nfrag >= 12
        d = Device(al, nreads, a, text_len)
        try:
            same_rows(d.duplicates(mates, PAR), want, "large text set")
        finally:
            d.close()
    finally:
        al.close()


@pytest.mark.gpu
def test_random_cases_under_poison_in_a_fresh_process(gpu):
    """The random cases once more with every recycled pool block filled with 0x7f, then 0xff (WFA_HIP_POISON is read when an aligner is
    created): no row depends on a byte that nothing wrote.  A fresh process, so that its pool starts empty."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(HERE, ".."), HERE] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "poison 127 ok" in out.stdout and "poison 255 ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


@pytest.mark.gpu
def test_refusals_launch_nothing(gpu):
    nc = configs_pair(**KW)[1]
    al, other = _native.Aligner(nc), _native.Aligner(nc)
    try:
        a = as_arrays(dict(i=[0, 2], j=[0, 1], reverse=[0, 0], score=[-4, -4], status=[0, 0], text_start=[1000, 5], text_end=[1150, 100]))
        d = Device(al, 4, a, [5000, 300])
        T = d.texts
        one_text, foreign = seqset(al, [5000]), seqset(other, [5000, 300])
        for args, kw, msg in (((one_text, 2), {}, r"duplicates: text index out of range at position 1 of the hit list: j = 1 over 1 texts"),
                              ((foreign, 2), {}, r"sequence set of another aligner"), ((T, 2), dict(full_gap=0), r"full_gap = 0 is out of range"),
                              ((T, 2), dict(min_insert=-1), r"min_insert = -1"), ((T, 2), dict(min_insert=1001), r"max_insert = 1000 are out of range"),
                              ((T, 2), dict(unpaired=-1), r"unpaired = -1 is out of range"), ((T, -1), {}, r"a negative number of fragments"),
                              ((T, 3), {}, r"3 interleaved fragments need 6 reads, there are 4"),
                              ((T, [[0, 4]]), {}, r"mate out of range at fragment 0: mate2 = 4 over 4 reads"),
                              ((T, [[0, 1], [1, 2]]), {}, r"read 1 is named by two fragments")):
            with pytest.raises(ValueError, match=msg):
                d.pl.duplicates(*args, **dict(PAR, **kw))
        L = _native.lib()
        reads, pairs = np.full((4, 4), 7, np.int32), np.full((2, 4), 7, np.int32)
        m = np.array([0, 2], np.int32)
        head = (INT32_MIN, 24, 0, 1000, 0)
        assert L.wfa_hip_placer_duplicates(d.pl._h, T._h, *head, 2, None, None, None, pairs.ctypes.data) == _native.EINVAL and "missing array (read_rows)" in al.error()
        assert L.wfa_hip_placer_duplicates(d.pl._h, T._h, *head, 2, None, None, reads.ctypes.data, None) == _native.EINVAL and "missing array (pair_rows)" in al.error()
        assert L.wfa_hip_placer_duplicates(d.pl._h, None, *head, 2, None, None, reads.ctypes.data, pairs.ctypes.data) == _native.EINVAL and "missing sequence set" in al.error()
        assert L.wfa_hip_placer_duplicates(d.pl._h, T._h, *head, 2, m.ctypes.data, None, reads.ctypes.data, pairs.ctypes.data) == _native.EINVAL and "mate2 is missing" in al.error()
        assert L.wfa_hip_placer_duplicates(d.pl._h, one_text._h, *head, 2, None, None, reads.ctypes.data, pairs.ctypes.data) == _native.EINVAL
        assert (reads == 7).all() and (pairs == 7).all() and d.pl.kernel_ms() == 0.0 and len(d.pl) == 2       # no kernel has run, nothing was written
        # usable afterwards; NULL pair_rows is legal without fragments
        assert L.wfa_hip_placer_duplicates(d.pl._h, T._h, *head, 0, None, None, reads.ctypes.data, None) == _native.OK and d.pl.kernel_ms() > 0.0
        assert reads.tolist() == [[0, 1, 0, 0], [-1, 0, 0, 0], [2, 1, 0, 0], [-1, 0, 0, 0]] and (pairs == 7).all()
        same_rows(d.duplicates(2, PAR), host(4, a, 2, PAR, [5000, 300]), "after the refusals")
        d.pl.clear()                                                                                          # the text indices go with the hits
        assert d.pl.duplicates(one_text, 2, **PAR)[0].tolist() == [[-1, 0, 0, 0]] * 4
        empty = al.placer(0)
        assert [x.shape for x in empty.duplicates(T, 0, **PAR)] == [(0, 4), (0, 4)]
        empty.close()
        one_text.close()
        foreign.close()
        d.close()
    finally:
        al.close()
        other.close()


# ---- end to end: 2 references of 4 kb, 64 fragments of 2 x 100 bases, 16 of them copies of others ----

GAP, PAD, L, NF, NCOPY = 24, 16, 100, 64, 16
HOW = dict(min_score=-100, min_insert=100, max_insert=600)
HOSTPAR = dict(min_score=-100, full_gap=GAP, min_insert=100, max_insert=600, unpaired=GAP)


def corpus(seed=21):
    """refs, reads (fragment f = reads 2 f and 2 f + 1), the window list (a read's true place padded by PAD, shuffled) and, per copy, its
    source.  Fragments 0 .. 47 are cut from distinct places, every second one with mate 1 as the reverse mate; fragments 48 .. 63 copy
    fragments 0 .. 15 with two substitutions per mate at read positions 10 .. 89, so that the aligned cores keep their ends."""
    rng = np.random.default_rng(seed)
    refs = ["".join(LETTERS[rng.integers(0, 4, 4000)]) for _ in range(2)]
    lefts = rng.permutation(np.arange(PAD, 4000 - 400 - PAD))[:NF - NCOPY]
    frags = [(int(rng.integers(0, 2)), int(lefts[f]), int(rng.integers(220, 401)), f % 2 == 1) for f in range(NF - NCOPY)]
    frags += frags[:NCOPY]
    reads, rows = [], []
    for f, (r, left, outer, flip) in enumerate(frags):
        pos_l, pos_r = left, left + outer - L
        for k, (pos, right_hand) in enumerate(((pos_r, True), (pos_l, False)) if flip else ((pos_l, False), (pos_r, True))):
            s = list(refs[r][pos:pos + L])
            if f >= NF - NCOPY:
                for at in rng.permutation(np.arange(10, 90))[:2]:
                    s[at] = "ACGT"[("ACGT".index(s[at]) + 1 + int(rng.integers(0, 3))) % 4]
            s = "".join(s)
            reads.append(revcomp(s) if right_hand else s)
            rows.append((2 * f + k, r, 0, L, pos - PAD, L + 2 * PAD, int(right_hand)))
    rows = [rows[q] for q in rng.permutation(len(rows))]
    return refs, reads, as_list(rows), list(range(NCOPY)), frags


REFS, READS, W, SOURCE, FRAGS = corpus()


def window_kwargs(Wl):
    return dict(i=Wl["i"], j=Wl["j"], pattern_start=Wl["p_start"], pattern_len=Wl["p_len"], text_start=Wl["t_start"], text_len=Wl["t_len"],
                reverse=Wl["reverse"])


def hits_from(res, Wl):
    """The hit list of an align_windows(summary=True) result: the interval is the window's start plus columns 8 and 9 of the summary."""
    loc = res["summary"]["locations"]
    t0 = np.asarray(Wl["t_start"], np.int64)
    return as_arrays(dict(i=Wl["i"], j=Wl["j"], reverse=Wl["reverse"], score=res["score"], status=res["status"], text_start=t0 + loc[:, 2],
                          text_end=t0 + loc[:, 3]))


def same_columns(res, want, ctx):
    for part, rows in (("reads", want[0]), ("pairs", want[1])):
        if part in res:
            for name, c in zip(DUP_KEYS, (2, 0, 1, 3)):
                got = res[part][name]
                assert got.dtype == np.int32 and got.tobytes() == np.ascontiguousarray(rows[:, c]).tobytes(), (ctx, part, name, got.tolist(), rows[:, c].tolist())


@pytest.mark.gpu
def test_place_pairs_marks_exactly_the_designed_copies(gpu, monkeypatch):
    wa = WavefrontAligner(**KW)
    text_len = [len(r) for r in REFS]
    plain = wa.place_pairs(READS, REFS, full_gap=GAP, **HOW, **window_kwargs(W))
    # duplicates=False: exactly the keys of before
    assert tuple(plain) == ("score", "status", "flag", "reads", "pair_flag", "pairs")
    assert tuple(plain["reads"]) == COLUMNS and tuple(plain["pairs"]) == PAIR_COLUMNS and plain["pairs"]["proper"].all()
    res = wa.place_pairs(READS, REFS, full_gap=GAP, duplicates=True, **HOW, **window_kwargs(W))
    assert tuple(res) == tuple(plain) and tuple(res["reads"]) == COLUMNS + DUP_KEYS and tuple(res["pairs"]) == PAIR_COLUMNS + DUP_KEYS
    for part in ("reads", "pairs"):
        assert all(res[part][k].tobytes() == plain[part][k].tobytes() for k in plain[part]), part
    pairs, reads = res["pairs"], res["reads"]
    assert pairs["dup"].tolist() == [0] * (NF - NCOPY) + [1] * NCOPY
    assert pairs["dup_rep"].tolist() == list(range(NF - NCOPY)) + SOURCE
    assert pairs["dup_size"].tolist() == [2] * NCOPY + [1] * (NF - 2 * NCOPY) + [2] * NCOPY and not pairs["dup_overflow"].any()
    assert reads["dup"].tolist() == np.repeat(pairs["dup"], 2).tolist() and (reads["dup_rep"] == -1).all() and not reads["dup_size"].any()
    # ... and the host statement fed with the hits of align_windows(summary=True)
    a = hits_from(wa.align_windows(READS, REFS, summary=True, **window_kwargs(W)), W)
    want = host(len(READS), a, NF, HOSTPAR, text_len)
    same_columns(res, want, "one chunk")
    # a list cut into chunks; resident sets and mates as an array
    monkeypatch.setenv("WFA_HIP_PAIRS_BAND", "37")
    same_columns(wa.place_pairs(READS, REFS, full_gap=GAP, duplicates=True, **HOW, **window_kwargs(W)), want, "chunks of 37")
    monkeypatch.delenv("WFA_HIP_PAIRS_BAND")
    with wa.sequence_set(READS) as R, wa.sequence_set(REFS) as G:
        same_columns(wa.place_pairs(R, G, full_gap=GAP, duplicates=True, mates=np.arange(2 * NF).reshape(-1, 2), **HOW, **window_kwargs(W)), want, "sets")
    # place_windows on the same reads, unpaired: every read is a unit, the copies' reads are duplicates of their sources'
    single = wa.place_windows(READS, REFS, full_gap=GAP, min_score=-100, **window_kwargs(W))
    assert tuple(single) == ("score", "status", "flag", "reads") and tuple(single["reads"]) == COLUMNS
    single = wa.place_windows(READS, REFS, full_gap=GAP, min_score=-100, duplicates=True, **window_kwargs(W))
    assert tuple(single) == ("score", "status", "flag", "reads") and tuple(single["reads"]) == COLUMNS + DUP_KEYS
    same_columns(single, host(len(READS), a, 0, dict(HOSTPAR, min_insert=0, max_insert=1000, unpaired=0), text_len), "place_windows")
    assert single["reads"]["dup"].tolist() == [0] * (2 * (NF - NCOPY)) + [1] * (2 * NCOPY)
    assert single["reads"]["dup_rep"][2 * (NF - NCOPY):].tolist() == list(range(2 * NCOPY))
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="duplicates must be True or False"):
            wa.place_pairs(READS, REFS, duplicates=bad, **window_kwargs(W))
        with pytest.raises(ValueError, match="duplicates must be True or False"):
            wa.place_windows(READS, REFS, duplicates=bad, **window_kwargs(W))
    wa.close()


@pytest.mark.gpu
def test_duplicates_run_after_a_rescue(gpu):
    """A copied fragment far from the ends of its reference (its rescue window is not clipped) loses the window of its mate 2: without
    a rescue it is not proper and its copy is alone; with rescue=True the mate comes back at its place and the marking, which runs
    after the final pairing, groups the two."""
    f = next(f for f in range(NCOPY) if 800 <= FRAGS[f][1] <= 2800)
    keep = W["i"] != 2 * f + 1
    Wl = {k: v[keep] for k, v in W.items()}
    wa = WavefrontAligner(**KW)
    lost = wa.place_pairs(READS, REFS, full_gap=GAP, duplicates=True, **HOW, **window_kwargs(Wl))
    assert lost["pairs"]["proper"][f] == 0 and lost["pairs"]["dup_rep"][f] == -1 and lost["pairs"]["dup_size"][NF - NCOPY + f] == 1
    assert lost["pairs"]["dup"].sum() == NCOPY - 1 and lost["reads"]["dup_rep"][2 * f] == 2 * f and lost["reads"]["dup_rep"][2 * f + 1] == -1
    res = wa.place_pairs(READS, REFS, full_gap=GAP, duplicates=True, rescue=True, rescue_pad=PAD, **HOW, **window_kwargs(Wl))
    assert res["pairs"]["proper"][f] == 1 and res["pairs"]["rescued"][f] == 1
    assert res["pairs"]["dup"].tolist() == [0] * (NF - NCOPY) + [1] * NCOPY and res["pairs"]["dup_rep"][NF - NCOPY + f] == f
    # the host statement over the listed hits followed by the rescue hits, aligned with the free ends a rescue sets
    found = res["rescue"]
    Wr = dict(i=found["i"], j=found["j"], p_start=np.zeros(len(found["i"]), np.int32), p_len=np.full(len(found["i"]), L, np.int64),
              t_start=found["text_start"].astype(np.int64), t_len=found["text_len"], reverse=found["reverse"].astype(np.uint8))
    a0 = hits_from(wa.align_windows(READS, REFS, summary=True, **window_kwargs(Wl)), Wl)
    free = (600 - 100) + 2 * PAD
    wa.text_begin_free = free
    wa.text_end_free = free
    a1 = hits_from(wa.align_windows(READS, REFS, summary=True, **window_kwargs(Wr)), Wr)
    a = [np.concatenate([x, y]) for x, y in zip(a0, a1)]
    same_columns(res, host(len(READS), a, NF, HOSTPAR, [len(r) for r in REFS]), "after a rescue")
    wa.close()


if __name__ == "__main__":
    for poison in ("127", "255"):
        os.environ["WFA_HIP_POISON"] = poison   # (read when the aligner is created)
        aligner = _native.Aligner(configs_pair(**KW)[1])
        try:
            assert random_cases(aligner) >= 2000
        finally:
            aligner.close()
        print(f"poison {poison} ok", flush=True)
