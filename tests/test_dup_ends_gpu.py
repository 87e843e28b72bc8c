"""Clips on every hit, duplicates on unclipped ends and the representative by base quality, on the GPU: the record kernel's clip word
against the summary's locations and the SAM clips of the same pairs, on op strings whose first and last M sit round the 64-op rounds of
the walk; wfa_hip_placer_duplicates_ex against the host statement wfa_hip_duplicates_host_ex byte for byte under every flag
combination; the quality-sum kernel against wfa_hip_qsum_host for reads that start at every byte offset mod 16 with other reads'
bytes on either side, under WFA_HIP_POISON in a fresh child process; and place_pairs / place_windows(dup_ends=, dup_qualities=) on a
corpus whose copies carry a substitution at a 5' end."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":   # (the poison child: the paths conftest.py sets up)
    sys.path[:0] = [os.path.join(HERE, ".."), HERE]

from common import configs_pair
from dup_common import MAX_BUCKET, as_arrays, sized_dup_case
from dup_ends_common import BY_QUALITY, CLIP_MAX, UNCLIPPED, py_clips, random_ends_case, sized_ends_case
from pair_common import INT32_MIN
from pywfa_amd import WavefrontAligner, _native
from test_windows_gpu import LETTERS, as_list, oracle_windows, revcomp

KW = dict(span="ends-free", text_begin_free=20, text_end_free=20)
PAR = dict(min_score=INT32_MIN, full_gap=24, min_insert=0, max_insert=1000, unpaired=0)
DUP_KEYS = ("dup", "dup_rep", "dup_size", "dup_overflow")
HIT = ("i", "j", "reverse", "score", "status", "text_start", "text_end")


def window_kwargs(Wl):
    return dict(i=Wl["i"], j=Wl["j"], pattern_start=Wl["p_start"], pattern_len=Wl["p_len"], text_start=Wl["t_start"], text_len=Wl["t_len"],
                reverse=Wl["reverse"])


def other(c, k=1):
    return "ACGT"[("ACGT".index(c) + k) % 4]


# ---- the record kernel: first and last M round the 64-op rounds ------------------------------------------------------------------------

FREE = 140
KW_TEXT = dict(span="ends-free", text_begin_free=FREE, text_end_free=FREE)
KW_READ = dict(span="ends-free", pattern_begin_free=FREE, pattern_end_free=FREE, text_begin_free=4, text_end_free=4)
HEADS = (0, 1, 63, 64, 65, 70, 128, 130)


def record_lists(seed=41):
    """(refs, {name: (kw, reads, window list)}).  "text": a read of 40 .. 200 bases against its place with h free text bases in front and
    t behind, h and t from HEADS: h leading and t trailing I ops, the first M at op h; every third read has its first base substituted
    (an X in front of the first M), every fourth its last.  "read": a read of 40 .. 70 true bases with h junk bases in front and t
    behind (70 and 130: D heads and tails that cross one and two 64-op rounds) against its exact place.  Both lists on both strands,
    every window at least as long as the free ends the span allows.  "steps": the "text" list under a step limit, so that some pairs
    do not finish.  "edge", end to end: an empty pattern window, an empty text window, both empty, a pair without any M, and reads
    whose first and last base are substituted."""
    rng = np.random.default_rng(seed)
    ref = "".join(LETTERS[rng.integers(0, 4, 6000)])
    lists = {}
    reads, rows = [], []
    for k, (h, t) in enumerate([(h, t) for h in HEADS for t in HEADS]):
        L = int(rng.integers(max(40, FREE - h - t), 201))
        pos = 200 + int(rng.integers(0, 5000))
        s = list(ref[pos:pos + L])
        if k % 3 == 0:
            s[0] = other(s[0])
        if k % 4 == 0:
            s[-1] = other(s[-1])
        rev = k % 2
        reads.append(revcomp("".join(s)) if rev else "".join(s))
        rows.append((len(reads) - 1, 0, 0, L, pos - h, L + h + t, rev))
    lists["text"] = (KW_TEXT, reads, as_list(rows))
    lists["steps"] = (dict(KW_TEXT, max_steps=2), reads, as_list(rows))
    reads, rows = [], []
    for k, (h, t) in enumerate([(h, t) for h in HEADS for t in HEADS if 80 <= h + t <= 150]):
        L = int(rng.integers(max(40, FREE - h - t), min(70, 200 - h - t) + 1))
        pos = 200 + int(rng.integers(0, 5000))
        junk = lambda n: "".join(LETTERS[rng.integers(0, 4, n)])
        s = junk(h) + ref[pos:pos + L] + junk(t)
        rev = k % 2
        reads.append(revcomp(s) if rev else s)
        rows.append((len(reads) - 1, 0, 0, len(s), pos, L, rev))
    lists["read"] = (KW_READ, reads, as_list(rows))
    reads, rows = ["A" * 40], [(0, 0, 0, 0, 300, 60, 0), (0, 0, 0, 40, 300, 0, 0), (0, 0, 0, 0, 300, 0, 0), (0, 1, 5, 4, 0, 4, 0)]
    for k in range(12):
        L = int(rng.integers(40, 201))
        pos = 200 + int(rng.integers(0, 5000))
        s = list(ref[pos:pos + L])
        for at in ([0], [-1], [0, -1], [0, 1, -1])[k % 4]:
            s[at] = other(s[at])
        reads.append(revcomp("".join(s)) if k % 2 else "".join(s))
        rows.append((len(reads) - 1, 0, 0, L, pos, L, k % 2))
    lists["edge"] = (dict(span="end-to-end"), reads, as_list(rows))
    return [ref, "CCCCCCCC"], lists


RECORD_REFS, RECORD_LISTS = record_lists()
_oracle_cache = {}


def oracle_of(name):
    """The oracle's result for one record list, computed once."""
    if name not in _oracle_cache:
        kw, reads, Wl = RECORD_LISTS[name]
        _oracle_cache[name] = oracle_windows(kw, reads, RECORD_REFS, Wl)[0]
    return _oracle_cache[name]


def test_the_designed_pairs_hold_the_shapes():
    """On the CPU, from the oracle's op strings: the lists are what record_lists says they are."""
    first_m, last_m, lead, trail = set(), set(), set(), set()
    for name in ("text", "read"):
        o = oracle_of(name)
        kw, reads, Wl = RECORD_LISTS[name]
        assert set(Wl["reverse"].tolist()) == {0, 1}
        for q, ops in enumerate(o["cigars"]):
            if b"M" not in ops:
                continue
            assert o["status"][q] == 0
            first_m.add(ops.index(b"M"))
            last_m.add(len(ops) - 1 - ops.rindex(b"M"))
            l, t = py_clips(ops, int(Wl["p_len"][q]), int(Wl["t_len"][q]))
            lead.add(l)
            trail.add(t)
            if name == "read":
                assert set(ops[:ops.index(b"M")]) <= set(b"DI") and l in HEADS and t in HEADS, (q, ops)
    for have in (first_m, last_m):
        assert {0, 1, 63, 64, 65, 128} <= have and max(have) > 128, sorted(have)
    for have in (lead, trail):
        assert {0, 1, 63, 64, 65, 70, 128, 130} <= have, sorted(have)
    o = oracle_of("edge")
    assert [c for c in o["cigars"][:4]] == [b"I" * 60, b"D" * 40, b"", b"XXXX"]      # the empty windows, and no M at all
    assert sum(c[:1] == b"X" for c in o["cigars"]) >= 6 and sum(c[-1:] == b"X" for c in o["cigars"]) >= 6 and any(c[:2] == b"XX" for c in o["cigars"])
    assert all(40 <= len(r) <= 200 for name in RECORD_LISTS for r in RECORD_LISTS[name][1])
    assert sum(st != 0 for st in oracle_of("steps")["status"]) >= 5 and sum(st == 0 for st in oracle_of("steps")["status"]) >= 5


def place_and_clips(wa, reads, refs, Wl):
    """What place_windows runs — the windows aligned, every chunk added to a placer — and the placer's clips read back."""
    w = wa._windows(reads, refs, Wl["i"], Wl["j"], Wl["p_start"], Wl["p_len"], Wl["t_start"], Wl["t_len"], Wl["reverse"])
    with w:
        placer = w.attach(wa._native.placer(w.nreads))
        out = w.run(each=wa._hits_into(placer, w.arrays))
        return out, placer.clips()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["text", "read", "steps", "edge"])
def test_record_kernel_stores_the_clips(gpu, monkeypatch, name):
    kw, reads, Wl = RECORD_LISTS[name]
    o = oracle_of(name)
    plen, tlen = Wl["p_len"].astype(np.int64), Wl["t_len"].astype(np.int64)
    want = np.array([py_clips(c, int(plen[q]), int(tlen[q])) for q, c in enumerate(o["cigars"])], np.int32).reshape(-1, 2)
    wa = WavefrontAligner(**kw)
    try:
        for band in (None, "37"):   # one chunk, and a list cut into chunks: several adds
            if band:
                monkeypatch.setenv("WFA_HIP_PAIRS_BAND", band)
            out, (lead, trail) = place_and_clips(wa, reads, RECORD_REFS, Wl)
            assert np.array_equal(out["status"], o["status"]) and lead.dtype == trail.dtype == np.int32
            assert np.array_equal(lead, want[:, 0]) and np.array_equal(trail, want[:, 1]), (name, band, np.flatnonzero(lead != want[:, 0])[:5])
        monkeypatch.delenv("WFA_HIP_PAIRS_BAND")
        # ... the summary's locations of the same pairs: pattern_start and plen - pattern_end, where there is an M
        loc = wa.align_windows(reads, RECORD_REFS, summary=True, **window_kwargs(Wl))["summary"]["locations"]
        has_m = np.array([b"M" in c for c in o["cigars"]])
        assert has_m.sum() >= len(has_m) // 3 and (name != "edge" or (~has_m).sum() == 4)
        assert np.array_equal(lead[has_m], loc[has_m, 0]) and np.array_equal(trail[has_m], (plen - loc[:, 1])[has_m])
        assert not lead[~has_m].any() and not trail[~has_m].any()
        # ... and the SAM fields under clip_mismatches: us = pos - clip_left, ue = pos + ref_len + clip_right
        sam = wa.align_windows(reads, RECORD_REFS, sam=True, clip_mismatches=True, **window_kwargs(Wl))["sam"]
        mapped = sam["pos"] >= 0
        assert np.array_equal(mapped, has_m & (o["status"] == 0))
        ts, te = Wl["t_start"] + loc[:, 2], Wl["t_start"] + loc[:, 3]
        assert np.array_equal((ts - lead)[mapped], (sam["pos"].astype(np.int64) - sam["clip_left"])[mapped])
        assert np.array_equal((te + trail)[mapped], (sam["pos"].astype(np.int64) + sam["ref_len"] + sam["clip_right"])[mapped])
        # scope score: no clips
        ws = WavefrontAligner(**dict(kw, scope="score"))
        try:
            _, (l0, t0) = place_and_clips(ws, reads, RECORD_REFS, Wl)
            assert l0.shape == lead.shape and not l0.any() and not t0.any()
        finally:
            ws.close()
    finally:
        wa.close()


# ---- the device against the host statement ----------------------------------------------------------------------------------------------

def seqset(al, lengths):
    """A resident set of sequences of the given lengths (the rule reads the lengths and the base offsets alone)."""
    lengths = np.asarray(lengths, np.int32)
    off = np.zeros(len(lengths), np.int64)
    off[1:] = np.cumsum(lengths[:-1])
    return al.seqset(np.full(max(int(lengths.sum()), 1), ord("A"), np.uint8), off, lengths)


class Qualities:
    """A quality set over `nreads` reads made from the given uint8 arrays, and the host statement's sums of it."""

    def __init__(self, al, quals):
        self.quals = quals
        lengths = np.array([len(q) for q in quals], np.int32)
        off = np.zeros(len(quals), np.int64)
        off[1:] = np.cumsum(lengths[:-1])
        self.reads = seqset(al, lengths)
        self.set = al.qualset(self.reads, np.concatenate(quals + [np.zeros(0, np.uint8)]), off, lengths)
        self.off = off

    def sums(self, min_quality):
        return np.array([_native.qsum_host(q, min_quality) for q in self.quals], np.int32)

    def close(self):
        self.set.close()
        self.reads.close()


def same_rows(got, want, ctx):
    for g, w, what in zip(got, want, ("read rows", "pair rows")):
        assert g.dtype == np.int32 and g.shape == w.shape, (ctx, what, g.shape, w.shape)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0 and g.tobytes() == w.tobytes(), (ctx, what, int(bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist(), bad.size)


def run_case(al, nreads, hits, mates, par, text_len, lead, trail, flags, quals, min_quality, ctx):
    """One case on the device (two adds, two calls) against the host statement; returns the host's rows."""
    a = as_arrays(hits)
    Q = Qualities(al, quals) if flags & BY_QUALITY else None
    qsum = Q.sums(min_quality) if Q else None
    want = _native.duplicates_host(nreads, *a, mates, text_len, **par, lead=lead, trail=trail, flags=flags, qsum=qsum)
    texts, pl = seqset(al, text_len), al.placer(nreads)
    try:
        n = len(a[0])
        for lo, hi in ((0, n // 3), (n // 3, n)):
            pl.add_hits(*[None if x is None else x[lo:hi] for x in a], lead=lead[lo:hi], trail=trail[lo:hi])
        back = pl.clips()
        assert np.array_equal(back[0], np.minimum(lead, CLIP_MAX)) and np.array_equal(back[1], np.minimum(trail, CLIP_MAX)), ctx
        how = dict(par, unclipped=bool(flags & UNCLIPPED), qualities=Q.set if Q else None, min_quality=min_quality)
        got = pl.duplicates(texts, mates, **how)
        same_rows(got, want, ctx)
        again = pl.duplicates(texts, mates, **how)                                   # two calls: identical bytes
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), ctx
        if flags == 0:                                                                # flags 0 is wfa_hip_placer_duplicates
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, pl.duplicates(texts, mates, **par))), ctx
    finally:
        pl.close()
        texts.close()
        if Q:
            Q.close()
    return want


def random_quals(rng, nreads):
    """Per read one of three quality arrays (ties are frequent), of 0 .. 40 bases."""
    pool = [rng.integers(0, 94, int(rng.integers(0, 41))).astype(np.uint8) for _ in range(3)]
    return [pool[int(k)] for k in rng.integers(0, 3, nreads)]


SIZED = [1, 2, 3, 63, 65, 255, 257, 511, 513, 777, 1023, 1025, 1791, 1999, 2000]


def random_cases(al):
    """About 200 cases on one aligner: 150 small ones in which every new clause occurs and 45 sized ones (up to 2 000 reads, text sets
    up to 64 kb), the flag combinations 0 .. 3 in turn.  Returns the number of duplicates seen."""
    rng = np.random.default_rng(2032)
    dups = 0
    for k in range(150):
        nreads, hits, mates, par, text_len, lead, trail, flags, _ = random_ends_case(rng)
        want = run_case(al, nreads, hits, mates, par, text_len, lead, trail, flags, random_quals(rng, nreads), int(rng.choice([0, 15, 93])), ("small", k, flags))
        dups += int(want[0][:, 2].sum())
    for k, nreads in enumerate(SIZED * 3):
        text_len = [[1000, 700], [30000, 34000], [65536]][k % 3]
        hits, mates = sized_dup_case(rng, nreads, text_len, spread=(None, 7, 40)[k // len(SIZED)])
        hits, lead, trail = sized_ends_case(rng, hits)
        want = run_case(al, nreads, hits, mates, PAR, text_len, lead, trail, k % 4, random_quals(rng, nreads), 15, ("sized", k, nreads))
        dups += int(want[0][:, 2].sum())
    return dups


@pytest.mark.gpu
def test_duplicates_ex_equals_the_host_statement_on_random_cases(gpu):
    al = _native.Aligner(configs_pair(**KW)[1])
    try:
        assert random_cases(al) >= 1500
    finally:
        al.close()


@pytest.mark.gpu
def test_buckets_formed_by_clips_alone_and_the_edges_of_a_text(gpu):
    """Forward read units whose cores start at b, b + 1, b + 2 and b + 3 with leads 0 .. 3: by core four buckets, unclipped one — of
    4 096 units (one group) and of 4 097 (not resolved); units at b = -1, 0, tlen - 1 and tlen; clips of 65 535 and above."""
    rng = np.random.default_rng(7)
    tlen = 80000
    rows, lead, trail = [], [], []

    def unit(rv, ts, te, l, t):
        rows.append((len(rows), 0, rv, -int(rng.integers(0, 4)), 0, ts, te))
        lead.append(l)
        trail.append(t)

    for b, size in ((100, MAX_BUCKET), (300, MAX_BUCKET + 1)):
        for k in range(size):
            unit(0, b + k % 4, b + 50, k % 4, int(rng.integers(0, 3)))
    for l in (1, 0, 1):          # us = -1 (twice: alone all the same) and us = 0
        unit(0, 0, 40, l, 0)
    unit(0, 1, 40, 1, 0)         # us = 0
    for t in (1, 0, 1):          # p5 = tlen (twice) and tlen - 1
        unit(1, tlen - 40, tlen, 0, t)
    unit(1, tlen - 40, tlen - 1, 5, 1)
    for l in (CLIP_MAX, CLIP_MAX + 1, 1 << 20, CLIP_MAX - 1):
        unit(0, 70000, 70050, l, 0)
    nreads = len(rows)
    order = rng.permutation(nreads)
    hits = dict(zip(HIT, zip(*[rows[q] for q in order])))
    lead, trail = np.array(lead, np.int32)[order], np.array(trail, np.int32)[order]
    al = _native.Aligner(configs_pair(**KW)[1])
    try:
        for flags in (UNCLIPPED, 0, UNCLIPPED | BY_QUALITY):
            want = run_case(al, nreads, hits, 0, PAR, [tlen], lead, trail, flags, random_quals(rng, nreads), 15, ("buckets", flags))[0]
            over = want[:, 3] == 1
            if flags & UNCLIPPED:
                assert over.sum() == MAX_BUCKET + 1 and (want[over, 1] == 1).all() and (want[:, 1] == MAX_BUCKET).sum() == MAX_BUCKET
                tail = want[2 * MAX_BUCKET + 1:]
                assert tail[:, 1].tolist() == [1, 2, 1, 2, 1, 2, 1, 2, 3, 3, 3, 1]
            else:
                assert not over.any() and want[:, 1].max() == (MAX_BUCKET + 4) // 4
    finally:
        al.close()


# ---- the quality-sum kernel ---------------------------------------------------------------------------------------------------------------

QLENS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 1000)


def qsum_reads(seed=9):
    """(quals, tests): a quality set in which, for every length L of QLENS and every k in 0 .. 15, five reads of that length start at a
    byte offset that is k mod 16, in this order of read numbers:
        z_last   the bytes of t with the last one lowered from 93 to 60,
        z_first  the bytes of t with the first one lowered from 93 to 60,
        p_a      the bytes of t, between neighbours whose adjoining bytes are 0,
        t        first and last byte 93, every other byte 60 .. 93, between neighbours whose adjoining bytes are 93,
        p_b      as p_a.
    The sums are seen only through the representative of a group of two, the greater sum and on a tie the smaller read number, so
    every pair is built so that a fault FLIPS it: (p_a, t) and (t, p_b) are true ties, and a byte taken from in front of or behind the
    read adds 93 to t and 0 to p, so that the greater read number wins one of them; (z_last, t) and (z_first, t) are won by t, the
    greater number, and a last or first byte left out makes them ties, which z wins.  That holds under min_quality 0, 15 and 93 (60
    is below 93, so a lowered byte then counts 0).  A filler between two reads is 2 .. 17 bytes: the byte its left neighbour wants
    behind it, 93s, the byte its right neighbour wants in front.  tests: (L, k, z_last, z_first, p_a, t, p_b) as read numbers."""
    rng = np.random.default_rng(seed)
    quals, tests, at = [], [], 0
    behind = 93                                                          # what the read before the next filler wants behind it

    def put(q):
        nonlocal at
        quals.append(q)
        at += len(q)
        return len(quals) - 1

    for L in QLENS:
        base = rng.integers(60, 94, L).astype(np.uint8)
        if L:
            base[0], base[-1] = 93, 93
        for k in range(16):
            five = []
            for variant in range(5):
                beside = 0 if variant in (2, 4) else 93
                filler = np.full((k - at - 2) % 16 + 2, 93, np.uint8)     # ends where the read must start
                filler[0], filler[-1] = behind, beside
                put(filler)
                assert at % 16 == k
                q = base.copy()
                if L and variant == 0:
                    q[-1] = 60
                if L and variant == 1:
                    q[0] = 60
                five.append(put(q))
                behind = beside
            tests.append((L, k, *five))
    put(np.array([behind] + [93] * 15, np.uint8))
    return quals, tests


def qsum_pairings(tests):
    """The four hit lists of qsum_cases: per (L, k) one group of two read units, (smaller number, greater number)."""
    return [[(t[2], t[5]) for t in tests if t[0]], [(t[3], t[5]) for t in tests if t[0]], [(t[4], t[5]) for t in tests], [(t[5], t[6]) for t in tests]]


def qsum_rows(quals, tests, qsum, pairs):
    """(arrays of the hit list, text lengths, the host statement's rows) for one pairing under the given sums."""
    rows = [(r, 0, 0, 0, 0, 40 * g, 40 * g + 30) for g, pair in enumerate(pairs) for r in pair]
    a = as_arrays(dict(zip(HIT, zip(*rows))))
    text_len = [40 * len(tests) + 100]
    return a, text_len, _native.duplicates_host(len(quals), *a, 0, text_len, **PAR, flags=BY_QUALITY, qsum=qsum)


def test_the_quality_reads_see_a_single_byte_fault():
    """On the CPU: the host statement fed with FAULTY sums — the last byte left out, the first one, one byte taken from behind the read,
    one from in front — gives another representative than with the true sums, for every length, every offset mod 16 and min_quality
    0, 15 and 93.  So the device test below cannot pass with a kernel whose head or tail mask is off by one."""
    quals, tests = qsum_reads()
    blob = np.concatenate(quals).astype(np.int64)
    lens = np.array([len(q) for q in quals])
    off = np.cumsum(lens) - lens
    assert {int(off[t[5]]) % 16 for t in tests} == set(range(16)) and {t[0] for t in tests} == set(QLENS) and len(quals) < 2000
    faults = dict(last_dropped=lambda o, n: (o, o + max(n - 1, 0)), first_dropped=lambda o, n: (o + min(n, 1), o + n),
                  one_behind=lambda o, n: (o, o + n + 1), one_in_front=lambda o, n: (o - 1, o + n))
    pairings = qsum_pairings(tests)
    for minq in (0, 15, 93):
        count = np.where(blob >= minq, blob, 0)
        true = np.array([_native.qsum_host(q, minq) for q in quals], np.int32)
        assert np.array_equal(true, [count[o:o + n].sum() for o, n in zip(off, lens)])
        for t in tests:
            L, k, z_last, z_first, p_a, tt, p_b = t
            assert true[p_a] == true[tt] == true[p_b] and (L == 0 or (true[z_last] < true[tt] and true[z_first] < true[tt]))
        want = [qsum_rows(quals, tests, true, pairs)[2][0] for pairs in pairings]
        for name, span in faults.items():
            faulty = np.array([count[slice(*span(o, n))].sum() for o, n in zip(off, lens)], np.int32)
            seen = set()
            for pairs, rows in zip(pairings, want):
                got = qsum_rows(quals, tests, faulty, pairs)[2][0]
                for g, (r, _) in enumerate(pairs):
                    if got[r].tolist() != rows[r].tolist():
                        seen.add(next((t[0], t[1]) for t in tests if r in t[2:]))
            need = {(t[0], t[1]) for t in tests if t[0] or name.startswith("one_")}
            assert need <= seen, (minq, name, sorted(need - seen)[:8])


def qsum_cases(al):
    """The quality sums through the rule: groups of two forward read units at one place each (qsum_reads says why each pair flips under
    a fault); every row against the host statement fed with wfa_hip_qsum_host's sums."""
    quals, tests = qsum_reads()
    nreads = len(quals)
    Q = Qualities(al, quals)
    texts, pl = seqset(al, [40 * len(tests) + 100]), al.placer(nreads)
    try:
        for minq in (0, 15, 93):
            qsum = Q.sums(minq)
            for n, pairs in enumerate(qsum_pairings(tests)):
                a, _, want = qsum_rows(quals, tests, qsum, pairs)
                pl.clear()
                pl.add_hits(*a)
                got = pl.duplicates(texts, 0, **PAR, qualities=Q.set, min_quality=minq)
                same_rows(got, want, ("qsum", minq, n))
                assert (want[0][:, 1] == 2).sum() == 2 * len(pairs)
    finally:
        pl.close()
        texts.close()
        Q.close()


@pytest.mark.gpu
def test_quality_sums_at_every_offset_and_length(gpu):
    al = _native.Aligner(configs_pair(**KW)[1])
    try:
        qsum_cases(al)
    finally:
        al.close()


@pytest.mark.gpu
def test_under_poison_in_a_fresh_process(gpu):
    """The random cases and the quality sums once more with every recycled pool block filled with 0x7f, then 0xff (WFA_HIP_POISON is
    read when an aligner is created): no row depends on a byte that nothing wrote.  A fresh process, so that its pool starts empty."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(HERE, ".."), HERE] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "poison 127 ok" in out.stdout and "poison 255 ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


@pytest.mark.gpu
def test_refusals_launch_nothing(gpu):
    nc = configs_pair(**KW)[1]
    al, foreign = _native.Aligner(nc), _native.Aligner(nc)
    try:
        a = as_arrays(dict(i=[0, 1], j=[0, 0], reverse=[0, 0], score=[0, -4], status=[0, 0], text_start=[100, 101], text_end=[150, 150]))
        texts, pl = seqset(al, [500]), al.placer(2)
        Q, short, other_q = Qualities(al, [np.full(5, 30, np.uint8)] * 2), Qualities(al, [np.full(5, 30, np.uint8)]), Qualities(foreign, [np.full(5, 30, np.uint8)] * 2)
        with pytest.raises(ValueError, match=r"a negative clip at position 1 of the hit list: lead = -1, trail = 0"):
            pl.add_hits(*a, lead=[0, -1])
        with pytest.raises(ValueError, match=r"lead: one value per hit \(2\)"):
            pl.add_hits(*a, lead=[0])
        assert len(pl) == 0
        pl.add_hits(*a, lead=[0, 1])
        with pytest.raises(ValueError, match=r"a negative clip at position 3 of the hit list: lead = 0, trail = -2"):
            pl.add_hits(*a, trail=[0, -2])
        assert len(pl) == 2
        L = _native.lib()
        reads = np.full((2, 4), 7, np.int32)
        head = (pl._h, texts._h, INT32_MIN, 24, 0, 1000, 0, 0, None, None, reads.ctypes.data, None)
        for tail, msg in (((4, None, 15), "an unknown flag bit"), ((-1, None, 15), "an unknown flag bit"), ((2, None, 15), "WFA_HIP_DUP_BY_QUALITY without qualities"),
                          ((3, None, 15), "without qualities"), ((0, Q.set._h, 15), "qualities without WFA_HIP_DUP_BY_QUALITY"),
                          ((1, Q.set._h, 15), "qualities without"), ((2, Q.set._h, 94), "min_quality = 94 is out of range (0 .. 93)"),
                          ((2, Q.set._h, -1), "min_quality = -1 is out of range"), ((2, other_q.set._h, 15), "quality set of another aligner"),
                          ((3, short.set._h, 15), "the quality set has 1 reads, the placer 2")):
            assert L.wfa_hip_placer_duplicates_ex(*head, *tail) == _native.EINVAL and msg in al.error(), (tail[0], tail[2], al.error())
        assert (reads == 7).all() and pl.kernel_ms() == 0.0                          # no kernel has run, nothing was written
        assert L.wfa_hip_placer_read_clips(pl._h, None, reads.ctypes.data) == _native.EINVAL and "missing array (lead)" in al.error()
        # usable afterwards
        assert pl.duplicates(texts, 0, **PAR)[0].tolist() == [[0, 1, 0, 0], [1, 1, 0, 0]]
        assert pl.duplicates(texts, 0, **PAR, unclipped=True)[0].tolist() == [[0, 2, 0, 0], [0, 2, 1, 0]]
        assert pl.duplicates(texts, 0, **PAR, unclipped=True, qualities=Q.set, min_quality=31)[0].tolist() == [[0, 2, 0, 0], [0, 2, 1, 0]]
        assert [x.tolist() for x in pl.clips()] == [[0, 1], [0, 0]]
        empty = al.placer(0)
        assert [x.shape for x in empty.clips()] == [(0,), (0,)] and [x.shape for x in empty.duplicates(texts, 0, **PAR, unclipped=True)] == [(0, 4), (0, 4)]
        empty.close()
        for x in (Q, short, other_q):
            x.close()
        pl.close()
        texts.close()
    finally:
        al.close()
        foreign.close()


# ---- end to end: 2 references of 4 kb, 64 fragments of 2 x 40 bases, 16 of them copies with a substitution at a 5' end ----------------

GAP, PAD, L, NF, NCOPY = 24, 16, 40, 64, 16
HOW = dict(min_score=-100, min_insert=80, max_insert=400)
HOSTPAR = dict(min_score=-100, full_gap=GAP, min_insert=80, max_insert=400, unpaired=GAP)


def corpus(seed=23):
    """refs, reads (fragment f = reads 2 f and 2 f + 1), qualities, the window list (a read's true place padded by PAD, shuffled) and
    the fragments.  Fragments 0 .. 47 are cut from distinct places, every second one with mate 1 as the reverse mate; fragments
    48 .. 63 copy fragments 0 .. 15 with ONE substitution: in the even copies at the first base of the forward mate, in the odd ones at
    the last reference base of the reverse mate — the two 5' ends of the fragment.  The sources have base quality 20, the copies 40: the
    source has the better alignment score, the copy the better qualities."""
    rng = np.random.default_rng(seed)
    refs = ["".join(LETTERS[rng.integers(0, 4, 4000)]) for _ in range(2)]
    lefts = rng.permutation(np.arange(PAD, 4000 - 400 - PAD))[:NF - NCOPY]
    frags = [(int(rng.integers(0, 2)), int(lefts[f]), int(rng.integers(120, 301)), f % 2 == 1) for f in range(NF - NCOPY)]
    frags += frags[:NCOPY]
    reads, quals, rows = [], [], []
    for f, (r, left, outer, flip) in enumerate(frags):
        pos_l, pos_r = left, left + outer - L
        for k, (pos, right_hand) in enumerate(((pos_r, True), (pos_l, False)) if flip else ((pos_l, False), (pos_r, True))):
            s = list(refs[r][pos:pos + L])
            if f >= NF - NCOPY and f % 2 == 0 and not right_hand:
                s[0] = other(s[0], 1 + f % 3)
            if f >= NF - NCOPY and f % 2 == 1 and right_hand:
                s[-1] = other(s[-1], 1 + f % 3)
            s = "".join(s)
            reads.append(revcomp(s) if right_hand else s)
            quals.append(chr(33 + (40 if f >= NF - NCOPY else 20)) * L)
            rows.append((2 * f + k, r, 0, L, pos - PAD, L + 2 * PAD, int(right_hand)))
    rows = [rows[q] for q in rng.permutation(len(rows))]
    return refs, reads, quals, as_list(rows), frags


REFS, READS, QUALS, W, FRAGS = corpus()
COPIES, SOURCES = list(range(NF - NCOPY, NF)), list(range(NCOPY))


def hits_and_clips(o, Wl):
    """The hit list and the clips the oracle's op strings give for a window list."""
    n = len(o["cigars"])
    ts, te, lead, trail = (np.zeros(n, np.int64) for _ in range(4))
    for q, ops in enumerate(o["cigars"]):
        pl, tl = int(Wl["p_len"][q]), int(Wl["t_len"][q])
        lead[q], trail[q] = py_clips(ops, pl, tl)
        if b"M" in ops and pl and tl:
            first, last = ops.index(b"M"), ops.rindex(b"M")
            ts[q] = Wl["t_start"][q] + sum(c in b"XI" for c in ops[:first])
            te[q] = Wl["t_start"][q] + tl - sum(c in b"XI" for c in ops[last + 1:])
    a = as_arrays(dict(i=Wl["i"], j=Wl["j"], reverse=Wl["reverse"], score=o["score"], status=o["status"], text_start=ts, text_end=te))
    return a, lead.astype(np.int32), trail.astype(np.int32)


_corpus_cache = {}


def corpus_expectation():
    """On the CPU, with the oracle and the host statement: the rows of the corpus under core and under unclipped ends, by score and by
    quality, paired and single-end."""
    if not _corpus_cache:
        o = oracle_windows(KW, READS, REFS, W)[0]
        a, lead, trail = hits_and_clips(o, W)
        qsum = np.array([_native.qsum_host(np.frombuffer(q.encode(), np.uint8) - 33, 15) for q in QUALS], np.int32)
        text_len = [len(r) for r in REFS]
        single = dict(HOSTPAR, min_insert=0, max_insert=1000, unpaired=0)
        _corpus_cache.update(o=o, a=a, lead=lead, trail=trail, qsum=qsum)
        for name, flags in (("core", 0), ("unclipped", UNCLIPPED), ("quality", UNCLIPPED | BY_QUALITY), ("core_quality", BY_QUALITY)):
            q = qsum if flags & BY_QUALITY else None
            _corpus_cache[name] = _native.duplicates_host(len(READS), *a, NF, text_len, **HOSTPAR, lead=lead, trail=trail, flags=flags, qsum=q)
            _corpus_cache["single_" + name] = _native.duplicates_host(len(READS), *a, 0, text_len, **single, lead=lead, trail=trail, flags=flags, qsum=q)
    return _corpus_cache


def test_the_corpus_is_what_it_says():
    """Before anything is asserted on the GPU: core marks none of the 16 copies, unclipped marks all 16; by score the source represents
    its group, by quality the copy; the substituted base is an X at the end of the op string and no shifted alignment ties."""
    e = corpus_expectation()
    o = e["o"]
    assert (o["status"] == 0).all()
    copy_reads = 0
    for q in range(len(W["i"])):
        ops, f, rev = o["cigars"][q], int(W["i"][q]) // 2, int(W["reverse"][q])
        core = ops.strip(b"I")
        want = b"M" * L
        if f >= NF - NCOPY and f % 2 == 0 and not rev:
            want, copy_reads = b"X" + b"M" * (L - 1), copy_reads + 1
        if f >= NF - NCOPY and f % 2 == 1 and rev:
            want, copy_reads = b"M" * (L - 1) + b"X", copy_reads + 1
        assert core == want and len(ops) == L + 2 * PAD and o["score"][q] == (-4 if b"X" in want else 0), (q, f, ops)
        assert ops.index(core) == PAD                                                 # at its place: nothing beside the window shifts it
    assert copy_reads == NCOPY
    assert e["core"][1][:, 2].sum() == 0 and (e["core"][1][:, 1] == 1).all()
    pairs = e["unclipped"][1]
    assert pairs[:, 2].tolist() == [0] * (NF - NCOPY) + [1] * NCOPY and pairs[:, 0].tolist() == list(range(NF - NCOPY)) + SOURCES
    pairs = e["quality"][1]
    assert pairs[:, 2].tolist() == [1] * NCOPY + [0] * (NF - NCOPY) and pairs[:, 0].tolist() == COPIES + list(range(NCOPY, NF))
    assert e["core_quality"][1][:, 2].sum() == 0
    assert e["single_core"][0][:, 2].sum() == NCOPY and e["single_unclipped"][0][:, 2].sum() == 2 * NCOPY


def same_columns(res, want, ctx):
    for part, rows in (("reads", want[0]), ("pairs", want[1])):
        if part in res:
            for name, c in zip(DUP_KEYS, (2, 0, 1, 3)):
                got = res[part][name]
                assert got.dtype == np.int32 and got.tobytes() == np.ascontiguousarray(rows[:, c]).tobytes(), (ctx, part, name, got.tolist(), rows[:, c].tolist())


@pytest.mark.gpu
def test_place_pairs_marks_the_copies_by_their_unclipped_ends(gpu, monkeypatch):
    e = corpus_expectation()
    wa = WavefrontAligner(**KW)
    try:
        kw = dict(full_gap=GAP, duplicates=True, **HOW, **window_kwargs(W))
        plain = wa.place_pairs(READS, REFS, **kw)
        same_columns(plain, e["core"], "core")
        same_columns(wa.place_pairs(READS, REFS, dup_ends="core", **kw), e["core"], "core, named")
        res = wa.place_pairs(READS, REFS, dup_ends="unclipped", **kw)
        assert tuple(res) == tuple(plain) and all(tuple(res[p]) == tuple(plain[p]) for p in ("reads", "pairs"))      # the keys are unchanged
        same_columns(res, e["unclipped"], "unclipped")
        assert res["pairs"]["dup"].tolist() == [0] * (NF - NCOPY) + [1] * NCOPY and plain["pairs"]["dup"].sum() == 0
        assert res["pairs"]["dup_rep"][NF - NCOPY:].tolist() == SOURCES               # by score: the designed high-score copy
        for k in plain["pairs"]:
            if k not in DUP_KEYS:
                assert res["pairs"][k].tobytes() == plain["pairs"][k].tobytes(), k    # place and pair keep the core
        # by quality: the designed high-quality copy; a list of strings, and a QualitySet
        byq = wa.place_pairs(READS, REFS, dup_ends="unclipped", dup_qualities=QUALS, **kw)
        same_columns(byq, e["quality"], "quality")
        assert byq["pairs"]["dup_rep"][:NCOPY].tolist() == COPIES and byq["pairs"]["dup"][:NCOPY].all()
        with wa.quality_set(READS, QUALS) as qs:
            same_columns(wa.place_pairs(READS, REFS, dup_ends="unclipped", dup_qualities=qs, dup_min_quality=15, **kw), e["quality"], "quality set")
            same_columns(wa.place_pairs(READS, REFS, dup_qualities=qs, **kw), e["core_quality"], "core by quality")
            # above every quality of the corpus all sums are 0: ties, the smaller number
            top = wa.place_pairs(READS, REFS, dup_ends="unclipped", dup_qualities=qs, dup_min_quality=41, **kw)
            assert top["pairs"]["dup_rep"][NF - NCOPY:].tolist() == SOURCES
        # a list cut into chunks
        monkeypatch.setenv("WFA_HIP_PAIRS_BAND", "37")
        same_columns(wa.place_pairs(READS, REFS, dup_ends="unclipped", dup_qualities=QUALS, **kw), e["quality"], "chunks of 37")
        monkeypatch.delenv("WFA_HIP_PAIRS_BAND")
        # place_windows on the same reads, unpaired
        skw = dict(full_gap=GAP, min_score=-100, duplicates=True, **window_kwargs(W))
        same_columns(wa.place_windows(READS, REFS, **skw), e["single_core"], "place_windows core")
        same_columns(wa.place_windows(READS, REFS, dup_ends="unclipped", **skw), e["single_unclipped"], "place_windows unclipped")
        same_columns(wa.place_windows(READS, REFS, dup_ends="unclipped", dup_qualities=QUALS, **skw), e["single_quality"], "place_windows quality")
    finally:
        wa.close()


@pytest.mark.gpu
def test_unclipped_duplicates_after_a_rescue(gpu):
    """An even copy (its forward mate carries the substitution) far from the ends of its reference loses the window of its reverse
    mate: without a rescue it is not proper; with rescue=True the mate comes back and the copy is marked by its unclipped ends."""
    f = next(f for f in COPIES if f % 2 == 0 and 800 <= FRAGS[f][1] <= 2800)
    lost_read = 2 * f + (0 if FRAGS[f][3] else 1)                                    # the reverse mate
    keep = W["i"] != lost_read
    Wl = {k: v[keep] for k, v in W.items()}
    wa = WavefrontAligner(**KW)
    try:
        kw = dict(full_gap=GAP, duplicates=True, dup_ends="unclipped", **HOW, **window_kwargs(Wl))
        lost = wa.place_pairs(READS, REFS, **kw)
        assert lost["pairs"]["proper"][f] == 0 and lost["pairs"]["dup_rep"][f] == -1 and lost["pairs"]["dup"].sum() == NCOPY - 1
        res = wa.place_pairs(READS, REFS, rescue=True, rescue_pad=PAD, **kw)
        assert res["pairs"]["proper"][f] == 1 and res["pairs"]["rescued"][f] == 1
        assert res["pairs"]["dup"].tolist() == [0] * (NF - NCOPY) + [1] * NCOPY and res["pairs"]["dup_rep"][f] == f - (NF - NCOPY)
        core = wa.place_pairs(READS, REFS, rescue=True, rescue_pad=PAD, **dict(kw, dup_ends="core"))
        assert core["pairs"]["dup"].sum() == 0
    finally:
        wa.close()


@pytest.mark.gpu
def test_python_refusals(gpu):
    wa, ws = WavefrontAligner(**KW), WavefrontAligner(scope="score", **KW)
    try:
        wk = window_kwargs(W)
        for fn in (wa.place_pairs, wa.place_windows):
            for kw, msg in ((dict(dup_ends="unclipped"), "dup_ends goes with duplicates=True"), (dict(dup_qualities=QUALS), "dup_qualities goes with duplicates=True"),
                            (dict(dup_min_quality=20), "dup_min_quality goes with duplicates=True"),
                            (dict(duplicates=True, dup_ends="soft"), "dup_ends must be 'core' or 'unclipped'"),
                            (dict(duplicates=True, dup_min_quality=20), "dup_min_quality goes with dup_qualities="),
                            (dict(duplicates=True, dup_qualities=QUALS, dup_min_quality=94), "dup_min_quality = 94 is out of range"),
                            (dict(duplicates=True, dup_qualities=QUALS, dup_min_quality=True), "dup_min_quality = True is out of range"),
                            (dict(duplicates=True, dup_qualities=QUALS[:-1]), "qualities has 127 entries, the reads are 128"),
                            (dict(duplicates=True, dup_qualities="IIII"), "qualities must be a list")):
                with pytest.raises(ValueError, match=msg):
                    fn(READS, REFS, **kw, **wk)
        for fn in (ws.place_pairs, ws.place_windows):
            with pytest.raises(ValueError, match="dup_ends='unclipped' needs scope='full'"):
                fn(READS, REFS, duplicates=True, dup_ends="unclipped", **wk)
        with wa.quality_set(READS[:4], QUALS[:4]) as few, ws.quality_set(READS, QUALS) as foreign:
            with pytest.raises(ValueError, match="the quality set was made for other reads"):
                wa.place_pairs(READS, REFS, duplicates=True, dup_qualities=few, **wk)
            with pytest.raises(ValueError, match="quality set of another aligner"):
                wa.place_pairs(READS, REFS, duplicates=True, dup_qualities=foreign, **wk)
        # under scope score the clips are 0: core and by quality still run
        res = ws.place_windows(READS, REFS, duplicates=True, dup_qualities=QUALS, **wk)
        assert set(DUP_KEYS) <= set(res["reads"])
    finally:
        wa.close()
        ws.close()


if __name__ == "__main__":
    for poison in ("127", "255"):
        os.environ["WFA_HIP_POISON"] = poison   # (read when the aligner is created)
        aligner = _native.Aligner(configs_pair(**KW)[1])
        try:
            assert random_cases(aligner) >= 1500
            qsum_cases(aligner)
        finally:
            aligner.close()
        print(f"poison {poison} ok", flush=True)
