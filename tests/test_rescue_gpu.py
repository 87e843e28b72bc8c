"""Mate rescue on the GPU (wfa_hip_placer_rescue, WavefrontAligner.place_pairs(rescue=True)): the device's window list equals the host
statement wfa_hip_rescue_host byte for byte on random cases and at the sizes at which the kernels can go wrong, and
place_pairs(rescue=True) equals the route it composes — place_pairs, the restated rule, align_windows with the free ends set by hand,
the restated pairing over both hit lists — in every array, on a paired corpus from which the window at mate 2's true place was taken
for 27 fragments; every one of them comes back proper at mate 2's true place."""
import ctypes

import numpy as np
import pytest

from common import configs_pair
from pair_common import INT32_MIN, PAIR_COLUMNS, as_hit_arrays, py_pair
from place_common import COLUMNS
from pywfa_amd import WavefrontAligner, _native
from rescue_common import join_hits, py_rescue, random_rescue_case, rescue_corpus, sized_case, window_list

KW = dict(span="ends-free", text_begin_free=20, text_end_free=20)
HIT_KEYS = ("i", "j", "reverse", "score", "status", "text_start", "text_end")
PAR = dict(min_score=INT32_MIN, full_gap=24, min_insert=150, max_insert=600, unpaired=0)


def seqset(al, lengths):
    """A resident set of sequences of the given lengths (the rule reads the lengths alone)."""
    lengths = np.asarray(lengths, np.int32)
    off = np.zeros(len(lengths), np.int64)
    off[1:] = np.cumsum(lengths[:-1])
    return al.seqset(np.full(max(int(lengths.sum()), 1), ord("A"), np.uint8), off, lengths)


def host(nreads, a, mates, par, read_len, text_len, pad, min_len, anchor_mapq, cap=None):
    return _native.rescue_host(nreads, *[a[k] for k in HIT_KEYS], mates, read_len, text_len, pad=pad, min_len=min_len, anchor_mapq=anchor_mapq,
                               cap=cap, **par)


class Device:
    """A placer holding the hits of one case (added in two adds) and the two sets of its lengths."""

    def __init__(self, al, nreads, a, read_len, text_len):
        self.sets = [seqset(al, read_len), seqset(al, text_len)]
        self.pl = al.placer(nreads)
        n = len(a["i"])
        for lo, hi in ((0, n // 3), (n // 3, n)):
            self.pl.add_hits(*[None if a[k] is None else a[k][lo:hi] for k in HIT_KEYS])

    def rescue(self, mates, par, pad, min_len, anchor_mapq, cap=None):
        return self.pl.rescue(self.sets[0], self.sets[1], mates, pad=pad, min_len=min_len, anchor_mapq=anchor_mapq, cap=cap, **par)

    def close(self):
        self.pl.close()
        for s in self.sets:
            s.close()


def same_list(got, want, ctx):
    assert got[0] == want[0] and got[1].dtype == np.int32 and got[1].shape == want[1].shape, (ctx, got[0], want[0], got[1].shape)
    bad = np.flatnonzero((got[1] != want[1]).any(axis=1))
    assert bad.size == 0 and got[1].tobytes() == want[1].tobytes(), (ctx, int(bad[0]), got[1][bad[0]].tolist(), want[1][bad[0]].tolist(), bad.size)


@pytest.mark.gpu
def test_rescue_equals_the_host_statement_on_random_cases(gpu):
    _, nc = configs_pair(**KW)
    al = _native.Aligner(nc)
    try:
        rng = np.random.default_rng(2027)
        made = 0
        for k in range(120):
            nreads, hits, mates, par, read_len, text_len, pad, min_len, anchor_mapq = random_rescue_case(rng)
            a = as_hit_arrays(hits)
            want = host(nreads, a, mates, par, read_len, text_len, pad, min_len, anchor_mapq)
            d = Device(al, nreads, a, read_len, text_len)
            try:
                same_list(d.rescue(mates, par, pad, min_len, anchor_mapq), want, ("random", k, mates, par, pad, min_len, anchor_mapq))
            finally:
                d.close()
            made += want[0]
        assert made >= 20
    finally:
        al.close()


# slot counts round a wave (nfrag 31 .. 33), round one scan chunk of 4 096 slots (2 047 .. 2 049), several chunks with a partial last one
SIZES = [(0, "mixed", False), (1, "mixed", False), (1, "all", True), (31, "mixed", True), (32, "mixed", False), (33, "all", False), (33, "mixed", True),
         (2047, "mixed", False), (2048, "all", True), (2048, "mixed", False), (2049, "mixed", True), (2049, "none", False), (6145, "mixed", True),
         (6145, "all", False)]


@pytest.mark.gpu
def test_rescue_at_the_sizes_of_the_wave_and_the_scan_chunk(gpu):
    _, nc = configs_pair(**KW)
    al = _native.Aligner(nc)
    try:
        rng = np.random.default_rng(7)
        for nfrag, kind, shuffled in SIZES:
            nreads, hits, mates, read_len, text_len = sized_case(rng, nfrag, kind, shuffled)
            a = as_hit_arrays(hits)
            ctx = (nfrag, kind, shuffled)
            want = host(nreads, a, mates, PAR, read_len, text_len, 16, 0, 0)
            if kind == "all":
                assert want[0] == 2 * nfrag, ctx
            elif kind == "none":
                assert want[0] == 0, ctx
            elif nfrag >= 31:
                assert 0 < want[0] < 2 * nfrag and len(set(want[1][:, 4].tolist())) == 2, ctx
            d = Device(al, nreads, a, read_len, text_len)
            try:
                before = d.pl.run_pairs(mates, **PAR)
                got = d.rescue(mates, PAR, 16, 0, 0)
                same_list(got, want, ctx)
                if nfrag:
                    assert d.pl.kernel_ms() > 0.0, ctx
                again = d.rescue(mates, PAR, 16, 0, 0)                                   # two calls: identical bytes
                assert again[0] == got[0] and again[1].tobytes() == got[1].tobytes(), ctx
                after = d.pl.run_pairs(mates, **PAR)                                     # a pair run behind it gives what one in front gave
                assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after)), ctx
                same_list(d.rescue(mates, PAR, 5, 300, 60), host(nreads, a, mates, PAR, read_len, text_len, 5, 300, 60), ctx + ("other parameters",))
                # cap = 0, cap = count - 1, rows = NULL: the count stays full, only cap rows are written
                count = want[0]
                same_list(d.rescue(mates, PAR, 16, 0, 0, cap=0), (count, want[1][:0]), ctx + ("cap 0",))
                if count:
                    same_list(d.rescue(mates, PAR, 16, 0, 0, cap=count - 1), (count, want[1][:count - 1]), ctx + ("cap count - 1",))
                    buf = np.full((count + 1, 8), 7, np.int32)
                    n = ctypes.c_int64(-1)
                    nf, m1, m2 = _native._mate_arrays(mates)
                    args = (d.pl._h, d.sets[0]._h, d.sets[1]._h, INT32_MIN, 24, 150, 600, 0, nf, None if m1 is None else m1.ctypes.data,
                            None if m2 is None else m2.ctypes.data, 16, 0, 0)
                    L = _native.lib()
                    assert L.wfa_hip_placer_rescue(*args, count - 1, ctypes.byref(n), buf.ctypes.data) == _native.OK and n.value == count, ctx
                    assert np.array_equal(buf[:count - 1], want[1][:count - 1]) and (buf[count - 1:] == 7).all(), ctx
                    n.value = -1
                    assert L.wfa_hip_placer_rescue(*args, 0, ctypes.byref(n), None) == _native.OK and n.value == count, ctx
            finally:
                d.close()
    finally:
        al.close()


@pytest.mark.gpu
def test_rescue_refusals_launch_nothing(gpu):
    _, nc = configs_pair(**KW)
    al, other = _native.Aligner(nc), _native.Aligner(nc)
    try:
        a = as_hit_arrays(dict(i=[0, 2], j=[0, 1], reverse=[0, 0], score=[-4, -4], status=[0, 0], text_start=[1000, 5], text_end=[1150, 100]))
        d = Device(al, 4, a, [150, 100, 50, 50], [5000, 300])
        short, one_text, foreign = seqset(al, [150, 100, 50]), seqset(al, [5000]), seqset(other, [5000, 300])
        P, T = d.sets
        L = _native.lib()
        for args, kw, msg in (((P, T, 2), dict(pad=-1), r"pad = -1, min_len = 0 are out of range"),
                              ((P, T, 2), dict(min_len=-1), r"min_len = -1 are out of range"),
                              ((P, T, 2), dict(anchor_mapq=61), r"anchor_mapq = 61 is out of range \(0 \.\. 60\)"),
                              ((P, T, 2), dict(anchor_mapq=-1), r"anchor_mapq = -1 is out of range"),
                              ((P, T, 2), dict(cap=-1), r"cap = -1 is out of range"),
                              ((short, T, 2), {}, r"the pattern set has 3 sequences, the placer 4 reads"),
                              ((P, one_text, 2), {}, r"text index out of range at position 1 of the hit list: j = 1 over 1 texts"),
                              ((foreign, T, 2), {}, r"sequence set of another aligner"), ((P, foreign, 2), {}, r"sequence set of another aligner"),
                              ((P, T, 2), dict(full_gap=0), r"full_gap = 0 is out of range"),
                              ((P, T, 2), dict(min_insert=-1), r"min_insert = -1"), ((P, T, 2), dict(max_insert=100), r"max_insert = 100 are out of range"),
                              ((P, T, 2), dict(unpaired=-1), r"unpaired = -1 is out of range"), ((P, T, -1), {}, r"a negative number of fragments"),
                              ((P, T, 3), {}, r"3 interleaved fragments need 6 reads, there are 4"),
                              ((P, T, [[0, 4]]), {}, r"mate out of range at fragment 0: mate2 = 4 over 4 reads"),
                              ((P, T, [[0, 1], [1, 2]]), {}, r"read 1 is named by two fragments")):
            with pytest.raises(ValueError, match=msg):
                d.pl.rescue(*args, **dict(PAR, **kw))
        n = ctypes.c_int64(-9)
        buf = np.full((4, 8), 7, np.int32)
        head = (d.pl._h, P._h, T._h, INT32_MIN, 24, 150, 600, 0, 2, None, None, 16, 0, 0)
        assert L.wfa_hip_placer_rescue(*head, 4, None, buf.ctypes.data) == _native.EINVAL and "missing array (count)" in al.error()
        assert L.wfa_hip_placer_rescue(*head, 4, ctypes.byref(n), None) == _native.EINVAL and "missing array (rows)" in al.error()
        assert L.wfa_hip_placer_rescue(d.pl._h, None, T._h, *head[3:], 4, ctypes.byref(n), buf.ctypes.data) == _native.EINVAL and "missing sequence set" in al.error()
        assert (buf == 7).all() and n.value == -9 and d.pl.kernel_ms() == 0.0 and len(d.pl) == 2       # no kernel has run, nothing was written
        count, rows = d.pl.rescue(P, T, 2, **PAR)                                                        # usable afterwards
        assert count == 2 and rows.tolist() == [[1, 0, 1034, 582, 1, 0, 0, 0], [3, 1, 89, 211, 1, 1, 1, 0]] and d.pl.kernel_ms() > 0.0
        assert d.pl.rescue(P, T, 0, **PAR)[0] == 0
        d.pl.clear()                                                                                     # the text indices go with the hits
        assert d.pl.rescue(P, one_text, 2, **PAR)[0] == 0
        for s in (short, one_text, foreign):
            s.close()
        d.close()
        # the FIRST hit outside the text set is named, which is not the greatest j: for every number of texts, the host's own words
        # (the hits arrive in two adds, so a position counts over the whole list)
        a = as_hit_arrays(dict(i=[0, 1, 2, 3, 0, 1], j=[1, 0, 2, 2, 4, 3], reverse=[0] * 6, score=[-4] * 6, status=[0] * 6,
                               text_start=[10] * 6, text_end=[60] * 6))
        d = Device(al, 4, a, [50] * 4, [100] * 5)
        for ntexts, at, j in ((1, 0, 1), (2, 2, 2), (3, 4, 4), (4, 4, 4)):
            few = seqset(al, [100] * ntexts)
            with pytest.raises(ValueError) as dev:
                d.pl.rescue(d.sets[0], few, 2, **PAR)
            with pytest.raises(ValueError) as ref:
                host(4, a, 2, PAR, [50] * 4, [100] * ntexts, 16, 0, 0)
            want = f"rescue: text index out of range at position {at} of the hit list: j = {j} over {ntexts} texts"
            assert str(dev.value).endswith(want) and str(ref.value).endswith(want), (ntexts, str(dev.value), str(ref.value))
            few.close()
        assert d.pl.rescue(*d.sets, 2, **PAR)[0] == host(4, a, 2, PAR, [50] * 4, [100] * 5, 16, 0, 0)[0]
        d.close()
    finally:
        al.close()
        other.close()


# ---- end to end: place_pairs(rescue=True) on the corpus without the windows at 27 mates' true places ----

REFS, READS, W, TRUTH, DROPPED = rescue_corpus()
NR, NF, N0 = len(READS), len(TRUTH), len(W["i"])
GAP, PADR = 24, 16
FREE = (600 - 150) + 2 * PADR
HOW = dict(min_score=-100, min_insert=150, max_insert=600)     # (min_score: see test_rescue_abi.py)
PY = dict(min_score=-100, full_gap=GAP, min_insert=150, max_insert=600, unpaired=GAP)
_ROUTE = {}


def window_kwargs(Wl):
    return dict(i=Wl["i"], j=Wl["j"], pattern_start=Wl["p_start"], pattern_len=Wl["p_len"], text_start=Wl["t_start"], text_len=Wl["t_len"],
                reverse=Wl["reverse"])


def hits_from(res, Wl):
    """The hit list of an align_windows(summary=True) result: the interval is the window's start plus columns 8 and 9 of the summary."""
    loc = res["summary"]["locations"]
    t0 = np.asarray(Wl["t_start"], np.int64)
    return dict(i=Wl["i"], j=Wl["j"], reverse=Wl["reverse"], score=res["score"], status=res["status"], text_start=t0 + loc[:, 2],
                text_end=t0 + loc[:, 3])


def composed_route():
    """place_pairs as it is today, py_rescue on its hits and the lengths, align_windows on that list with the free ends set through
    the setters, py_pair over the concatenated hits: computed once, never changed."""
    if not _ROUTE:
        wa = WavefrontAligner(**KW)
        first = wa.place_pairs(READS, REFS, full_gap=GAP, **HOW, **window_kwargs(W))
        hits0 = hits_from(wa.align_windows(READS, REFS, summary=True, **window_kwargs(W)), W)
        read_len, text_len = [len(r) for r in READS], [len(r) for r in REFS]
        found = py_rescue(hits0, NR, NF, PY, read_len, text_len, PADR, FREE, 0)
        Wr = window_list(found, read_len)
        wa.text_begin_free = FREE
        wa.text_end_free = FREE
        hits1 = hits_from(wa.align_windows(READS, REFS, summary=True, **window_kwargs(Wr)), Wr)
        hits = join_hits(hits0, hits1)
        _ROUTE.update(first=first, hits0=hits0, found=found, hits=hits, final=py_pair(hits, NR, NF, *PY.values()))
        wa.close()
    return _ROUTE


@pytest.mark.gpu
def test_place_pairs_with_rescue_equals_the_composed_route(gpu):
    route = composed_route()
    first, found, hits = route["first"], route["found"], route["hits"]
    # without rescue the fragments are lost (so that nothing below passes vacuously), and today's keys are all there is
    assert tuple(first) == ("score", "status", "flag", "reads", "pair_flag", "pairs") and tuple(first["pairs"]) == PAIR_COLUMNS
    assert len(DROPPED) == 27 and not first["pairs"]["proper"][DROPPED].any() and not first["pairs"]["pairings"][DROPPED].any()
    rows0, flags0, pr0, pf0 = py_pair(route["hits0"], NR, NF, *PY.values())
    assert np.array_equal(first["flag"], flags0) and all(np.array_equal(first["pairs"][k], pr0[:, c]) for c, k in enumerate(PAIR_COLUMNS))
    wa = WavefrontAligner(**KW)
    res = wa.place_pairs(READS, REFS, full_gap=GAP, rescue=True, rescue_pad=PADR, **HOW, **window_kwargs(W))
    assert (wa.text_begin_free, wa.text_end_free) == (20, 20)
    rows, flags, pair_rows, pair_flags = route["final"]
    assert tuple(res) == ("score", "status", "flag", "reads", "pair_flag", "pairs", "rescue")
    assert tuple(res["rescue"]) == ("i", "j", "text_start", "text_len", "reverse", "fragment", "anchor") and len(found) >= 27
    for c, name in enumerate(res["rescue"]):
        assert res["rescue"][name].dtype == np.int32 and np.array_equal(res["rescue"][name], found[:, c]), name
    assert np.array_equal(res["score"], hits["score"]) and np.array_equal(res["status"], hits["status"]) and len(res["score"]) == N0 + len(found)
    assert np.array_equal(res["flag"], flags) and np.array_equal(res["pair_flag"], pair_flags)
    assert tuple(res["reads"]) == COLUMNS and tuple(res["pairs"]) == PAIR_COLUMNS + ("rescued",)
    for c, name in enumerate(COLUMNS):
        assert np.array_equal(res["reads"][name], rows[:, c]), name
    for c, name in enumerate(PAIR_COLUMNS):
        bad = np.flatnonzero(res["pairs"][name] != pair_rows[:, c])
        assert res["pairs"][name].dtype == np.int32 and bad.size == 0, (name, bad[:5], pair_rows[bad[:1]].tolist())
    rescued = ((pair_rows[:, 2] == 1) & ((pair_rows[:, 0] >= N0) | (pair_rows[:, 1] >= N0))).astype(np.int32)
    assert res["pairs"]["rescued"].dtype == np.int32 and np.array_equal(res["pairs"]["rescued"], rescued)
    # every dropped fragment is back: proper, mate 2 by a rescue hit, at mate 2's true place (at least half of its 150 bases)
    for f in DROPPED:
        r2, pos2 = TRUTH[f][6]
        h2 = int(pair_rows[f, 1])
        assert pair_rows[f, 2] == 1 and h2 >= N0 and rescued[f] == 1 and hits["j"][h2] == r2, (f, pair_rows[f].tolist())
        assert min(int(hits["text_end"][h2]), pos2 + 150) - max(int(hits["text_start"][h2]), pos2) >= 75, (f, int(hits["text_start"][h2]), pos2)
    # resident sets and mates as an array give the same bytes
    with wa.sequence_set(READS) as R, wa.sequence_set(REFS) as G:
        again = wa.place_pairs(R, G, full_gap=GAP, rescue=True, rescue_pad=PADR, mates=np.arange(NR).reshape(-1, 2), **HOW, **window_kwargs(W))
    assert all(again["pairs"][k].tobytes() == res["pairs"][k].tobytes() for k in res["pairs"]) and again["pair_flag"].tobytes() == res["pair_flag"].tobytes()
    wa.close()


@pytest.mark.gpu
def test_place_pairs_rescue_refusals_and_restored_free_ends(gpu):
    wa = WavefrontAligner(**KW)
    for bad, msg in ((dict(rescue=1), "rescue must be True or False"), (dict(rescue="yes"), "rescue must be True or False"),
                     (dict(rescue=True, rescue_pad=-1), "rescue_pad = -1 is out of range"), (dict(rescue=True, rescue_pad=1.5), "rescue_pad must be an integer"),
                     (dict(rescue=True, rescue_pad=2**30), "rescue_pad = 1073741824 is out of range"),
                     (dict(rescue=True, rescue_mapq=61), r"rescue_mapq = 61 is out of range \(0 \.\. 60\)"),
                     (dict(rescue=True, rescue_mapq=-1), "rescue_mapq = -1 is out of range"), (dict(rescue=True, rescue_mapq=True), "rescue_mapq must be an integer")):
        with pytest.raises(ValueError, match=msg):
            wa.place_pairs(READS, REFS, **dict(window_kwargs(W), **bad))
    # the bound on the insert range and the pad together belongs to a rescue alone: without one, an unbounded max_insert is what it
    # always was, whatever the pad, and gives the bytes of a bound no insert reaches
    with pytest.raises(ValueError, match=r"max_insert - min_insert = 2147483647 with rescue_pad = 16 is out of range for a rescue"):
        wa.place_pairs(READS, REFS, rescue=True, max_insert=2**31 - 1, **window_kwargs(W))
    open_end = wa.place_pairs(READS, REFS, full_gap=GAP, min_score=-100, min_insert=150, max_insert=2**31 - 1, **window_kwargs(W))
    bounded = wa.place_pairs(READS, REFS, full_gap=GAP, min_score=-100, min_insert=150, max_insert=10**6, rescue_pad=2**30, **window_kwargs(W))
    assert tuple(open_end) == ("score", "status", "flag", "reads", "pair_flag", "pairs") and tuple(open_end["pairs"]) == PAIR_COLUMNS
    assert all(open_end["pairs"][k].tobytes() == bounded["pairs"][k].tobytes() for k in PAIR_COLUMNS) and open_end["pairs"]["proper"].any()
    with pytest.raises(ValueError, match="rescue needs scope='full'"):
        WavefrontAligner(scope="score", **KW).place_pairs(READS, REFS, rescue=True, **window_kwargs(W))
    with pytest.raises(ValueError, match="rescue needs span='ends-free'"):
        WavefrontAligner(span="end-to-end").place_pairs(READS, REFS, rescue=True, **window_kwargs(W))
    # a call that raises leaves the free ends as they were: a closed set
    closed = wa.sequence_set(REFS)
    closed.close()
    with pytest.raises(ValueError, match="sequence set is closed"):
        wa.place_pairs(READS, closed, rescue=True, **HOW, **window_kwargs(W))
    assert (wa.text_begin_free, wa.text_end_free) == (20, 20)
    # ... and so does a run of the rescue list that raises
    real = wa._run_windows
    calls = []

    def failing(*args, **kw):
        calls.append((wa.text_begin_free, wa.text_end_free))
        if len(calls) == 2:
            raise RuntimeError("the rescue run failed")
        return real(*args, **kw)

    wa._run_windows = failing
    try:
        with pytest.raises(RuntimeError, match="the rescue run failed"):
            wa.place_pairs(READS, REFS, full_gap=GAP, rescue=True, rescue_pad=PADR, **HOW, **window_kwargs(W))
    finally:
        del wa._run_windows
    assert calls == [(20, 20), (FREE, FREE)] and (wa.text_begin_free, wa.text_end_free) == (20, 20)
    wa.close()
