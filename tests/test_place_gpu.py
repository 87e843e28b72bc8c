"""Placement of reads on the GPU (wfa_hip_placer_*, WavefrontAligner.place_windows): rows and flags equal the host statement
wfa_hip_place_host on synthetic hit lists of every group size around the wave width, and the Python restatement fed with the ORACLE's
scores, statuses and aligned cores on the corpus — under both scopes, in one chunk and in several, with texts=None, under a step limit,
after the sets are closed — and, end to end, seeds -> place_windows -> a pileup of primaries.  Exact equality."""
import numpy as np
import pytest

from common import configs_pair
from oracle import loader
from place_common import COLUMNS, INT32_MIN, corpus, hits_of, py_place
from pywfa_amd import WavefrontAligner, _native, datagen
from test_windows_gpu import materialise, native_set, native_windows

KW = dict(span="ends-free", text_begin_free=20, text_end_free=20)
KW_STEPS = dict(KW, max_steps=50)
REFS, READS, W, ORIGIN = corpus()
NR, N = len(READS), len(W["i"])
GAP = 24
_ORACLE = {}


def expect(kw=KW, full=True, P=READS, T=REFS, Wl=W, key=None):
    """(oracle results, hit list) of the corpus under a configuration: computed once per configuration, never changed."""
    key = key or (tuple(sorted(kw.items())), full)
    if key not in _ORACLE:
        pats, txts = materialise(P, T, Wl)
        o = loader.run(loader.oracle(), loader.make_config(**dict(kw, scope="full" if full else "score")), datagen.from_strings(pats, txts, upper=True))
        _ORACLE[key] = (o, hits_of(o, Wl, full))
    return _ORACLE[key]


def window_kwargs(Wl=W):
    return dict(i=Wl["i"], j=Wl["j"], pattern_start=Wl["p_start"], pattern_len=Wl["p_len"], text_start=Wl["t_start"], text_len=Wl["t_len"],
                reverse=Wl["reverse"])


def check(res, o, hits, nreads, min_score, full_gap, ctx):
    rows, flags = py_place(hits, nreads, min_score, full_gap)
    assert np.array_equal(res["score"], o["score"]) and np.array_equal(res["status"], o["status"]), ctx
    assert res["flag"].dtype == np.uint8 and np.array_equal(res["flag"], flags), (ctx, np.flatnonzero(res["flag"] != flags)[:5])
    assert tuple(res["reads"]) == COLUMNS, ctx
    for c, name in enumerate(COLUMNS):
        got = res["reads"][name]
        assert got.dtype == np.int32 and got.shape == (nreads,), (ctx, name)
        bad = np.flatnonzero(got != rows[:, c])
        assert bad.size == 0, (ctx, name, int(bad[0]), int(got[bad[0]]), rows[bad[0]].tolist(), bad.size)


def synthetic(seed=9):
    """About 3 000 reads and 40 000 hits: every read's group size drawn from 0, 1, 2, 63, 64, 65, 130, one group of 5 000; scores from
    a small range, a few statuses, intervals on a grid of 25 with lengths 0, 50 and 100; the hits of all reads in shuffled order."""
    rng = np.random.default_rng(seed)
    nreads = 3000
    size = rng.choice([0, 1, 2, 63, 64, 65, 130], nreads, p=[0.25, 0.3, 0.3, 0.04, 0.04, 0.04, 0.03])
    size[:7] = [0, 1, 2, 63, 64, 65, 130]
    size[1234] = 5000
    reads = rng.permutation(nreads)                        # (the group sizes land on reads in no order)
    i = rng.permutation(np.repeat(reads, size)).astype(np.int32)
    n = len(i)
    ts = 25 * rng.integers(0, 12, n)
    hits = dict(i=i, j=rng.integers(0, 2, n).astype(np.int32), reverse=rng.integers(0, 2, n).astype(np.uint8),
                score=(-4 * rng.integers(0, 8, n)).astype(np.int32), status=((rng.random(n) < 0.1) * rng.integers(1, 3, n)).astype(np.int32),
                text_start=ts.astype(np.int32), text_end=(ts + rng.choice([0, 50, 100], n)).astype(np.int32))
    return nreads, hits, np.bincount(i, minlength=nreads)


def host(nreads, h, min_score, full_gap):
    return _native.place_host(nreads, h["i"], h["j"], h["reverse"], h["score"], h["status"], h["text_start"], h["text_end"], min_score, full_gap)


@pytest.mark.gpu
def test_add_hits_and_run_equal_the_host_statement(gpu):
    nreads, h, sizes = synthetic()
    n = len(h["i"])
    assert 35000 <= n <= 50000 and set(np.unique(sizes)) == {0, 1, 2, 63, 64, 65, 130, 5000}
    _, nc = configs_pair(**KW)
    al = _native.Aligner(nc)
    try:
        pl = al.placer(nreads)
        assert len(pl) == 0 and pl.kernel_ms() == 0.0
        rows, flags = pl.run(INT32_MIN, GAP)                   # no hits yet: every read unplaced
        assert flags.shape == (0,) and (rows == np.array([-1, INT32_MIN, INT32_MIN, 0, 0, 0, 0, 0])).all()
        cut = n // 3 + 7
        for lo, hi in ((0, cut), (cut, n)):
            pl.add_hits(*[None if h[k] is None else h[k][lo:hi] for k in ("i", "j", "reverse", "score", "status", "text_start", "text_end")])
        assert len(pl) == n
        want = host(nreads, h, INT32_MIN, GAP)
        got = pl.run(INT32_MIN, GAP)
        bad = np.flatnonzero((got[0] != want[0]).any(axis=1))
        assert bad.size == 0, (int(bad[0]), sizes[bad[0]], got[0][bad[0]], want[0][bad[0]], bad.size)
        assert np.array_equal(got[1], want[1]), np.flatnonzero(got[1] != want[1])[:5]
        assert pl.kernel_ms() > 0.0
        again = pl.run(INT32_MIN, GAP)
        assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
        # other parameters, nothing re-added; then rows alone
        for min_score, full_gap in ((-12, 5), (-4, 1), (1, 24)):
            want = host(nreads, h, min_score, full_gap)
            got = pl.run(min_score, full_gap)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (min_score, full_gap)
        assert (got[0][:, 0] == -1).all() and not got[1].any()              # (min_score 1: nothing is eligible)
        rows, none = pl.run(-12, 5, flags=False)
        assert none is None and np.array_equal(rows, host(nreads, h, -12, 5)[0])
        # an add after a run: the next run sees every hit; a cleared placer starts again at hit number 0
        extra = dict(i=[1234, 5], j=[0, 1], reverse=[0, 1], score=[0, 0], status=[0, 0], text_start=[3000, 0], text_end=[3100, 10])
        pl.add_hits(*[extra[k] for k in ("i", "j", "reverse", "score", "status", "text_start", "text_end")])
        both = {k: np.concatenate([h[k], np.asarray(extra[k], h[k].dtype)]) for k in h}
        want = host(nreads, both, INT32_MIN, GAP)
        got = pl.run(INT32_MIN, GAP)
        assert len(pl) == n + 2 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        pl.clear()
        assert len(pl) == 0
        pl.add_hits(*[extra[k] for k in ("i", "j", "reverse", "score", "status", "text_start", "text_end")])
        got = pl.run(INT32_MIN, GAP)
        assert got[1].tolist() == [3, 3] and got[0][1234].tolist() == [0, 0, INT32_MIN, 60, 1, 0, 3000, 3100] and (got[0][:, 0] >= 0).sum() == 2
        pl.close()
        pl.close()
    finally:
        al.close()


@pytest.mark.gpu
def test_place_windows_full_scope(gpu):
    o, hits = expect()
    wa = WavefrontAligner(**KW)
    res = wa.place_windows(READS, REFS, **window_kwargs())
    check(res, o, hits, NR, INT32_MIN, GAP, "full, defaults")                 # (full_gap None: 6 x the mismatch penalty of 4)
    assert (res["reads"]["mapq"] == 60).sum() >= 80 and (res["flag"] == 2).sum() >= 150
    check(wa.place_windows(READS, REFS, min_score=-24, full_gap=7, **window_kwargs()), o, hits, NR, -24, 7, "full, min_score")


@pytest.mark.gpu
def test_place_windows_score_scope(gpu):
    o, hits = expect(full=False)
    assert np.array_equal(np.asarray(hits["text_end"]) - np.asarray(hits["text_start"]), W["t_len"])
    res = WavefrontAligner(scope="score", **KW).place_windows(READS, REFS, full_gap=GAP, **window_kwargs())
    check(res, o, hits, NR, INT32_MIN, GAP, "score")
    assert np.array_equal(res["reads"]["text_end"] - res["reads"]["text_start"], W["t_len"][res["reads"]["hit"]])


@pytest.mark.gpu
def test_chunks_give_the_one_chunk_output(gpu, monkeypatch):
    o, hits = expect()
    wa = WavefrontAligner(**KW)
    with wa.sequence_set(READS) as R, wa.sequence_set(REFS) as G:
        one = wa.place_windows(R, G, **window_kwargs())
        monkeypatch.setenv("WFA_HIP_PAIRS_BAND", "97")                        # (the list is shuffled: every read's group straddles chunks)
        many = wa.place_windows(R, G, **window_kwargs())
    check(many, o, hits, NR, INT32_MIN, GAP, "chunks of 97")
    assert many["flag"].tobytes() == one["flag"].tobytes()
    for name in COLUMNS:
        assert many["reads"][name].tobytes() == one["reads"][name].tobytes(), name
    with pytest.raises(ValueError, match="closed"):                           # the sets are closed by now
        wa.place_windows(R, G, **window_kwargs())
    check(wa.place_windows(READS, REFS, **window_kwargs()), o, hits, NR, INT32_MIN, GAP, "usable afterwards")


@pytest.mark.gpu
def test_texts_none(gpu):
    """One set, the references behind the reads: the reads are the first sequences, the references never get a hit."""
    both = READS + REFS
    Wl = dict(W, j=(W["j"] + NR).astype(np.int32))
    o, hits = expect(P=both, T=None, Wl=Wl, key="texts=None")
    res = WavefrontAligner(**KW).place_windows(both, **window_kwargs(Wl))
    check(res, o, hits, len(both), INT32_MIN, GAP, "texts=None")
    assert (res["reads"]["hit"][NR:] == -1).all() and (res["reads"]["hit"][:NR] >= 0).all()


@pytest.mark.gpu
def test_step_limit(gpu):
    o, hits = expect(KW_STEPS)
    stopped = np.asarray(o["status"]) != 0
    assert 100 <= stopped.sum() <= N - 100
    res = WavefrontAligner(**KW_STEPS).place_windows(READS, REFS, **window_kwargs())
    check(res, o, hits, NR, INT32_MIN, GAP, "step limit")
    assert not res["flag"][stopped].any() and res["flag"][~stopped].all()


@pytest.mark.gpu
def test_refusals(gpu):
    wa = WavefrontAligner(**KW)
    for bad, msg in ((dict(full_gap=0), "full_gap = 0 is out of range"), (dict(full_gap=2.5), "full_gap must be an integer"),
                     (dict(min_score="x"), "min_score must be an integer"), (dict(min_score=True), "min_score must be an integer"),
                     (dict(min_score=2**31), "does not fit 32 bits")):
        with pytest.raises(ValueError, match=msg):
            wa.place_windows(READS, REFS, **dict(window_kwargs(), **bad))
    i = W["i"].copy()
    i[5] = NR
    with pytest.raises(ValueError, match=rf"i\[5\] = {NR} is out of range"):
        wa.place_windows(READS, REFS, **dict(window_kwargs(), i=i))
    _, nc = configs_pair(**KW)
    part = {k: v[:40] for k, v in W.items()}
    al, al2 = _native.Aligner(nc), _native.Aligner(nc)
    try:
        ps, ts = native_set(al, READS), native_set(al, REFS)
        pl = al.placer(NR)
        rb = native_windows(al, ps, ts, part)
        with pytest.raises(ValueError, match="placement needs a finished run of the batch"):
            pl.add(rb, part["i"], part["j"], part["t_start"], part["reverse"])
        rb.run()
        rb.sync()
        for name, at, value, msg in (("i", 9, NR, rf"read index out of range at position 9 of the hit list: i = {NR} over {NR} reads"),
                                     ("i", 3, -1, r"position 3 of the hit list: i = -1 over"),
                                     ("j", 17, -2, r"negative text index at position 17 of the hit list: j = -2"),
                                     ("t_start", 0, -9, r"negative text start at position 0 of the hit list: text_start = -9")):
            arr = {k: part[k].copy() for k in ("i", "j", "t_start")}
            arr[name][at] = value
            with pytest.raises(ValueError, match=msg):
                pl.add(rb, arr["i"], arr["j"], arr["t_start"], part["reverse"])
        with pytest.raises(ValueError, match="one value per pair"):
            pl.add(rb, part["i"][:-1], part["j"][:-1])
        rb2 = native_windows(al2, native_set(al2, READS), native_set(al2, REFS), part)
        rb2.run()
        rb2.sync()
        with pytest.raises(ValueError, match="batch of another aligner"):
            pl.add(rb2, part["i"], part["j"], part["t_start"], part["reverse"])
        with pytest.raises(ValueError, match=r"text_end below text_start at position 1 of the hit list: \[8, 7\)"):
            pl.add_hits([0, 0], [0, 0], None, [0, 0], [0, 0], [0, 8], [5, 7])
        with pytest.raises(ValueError, match=r"full_gap = 0 is out of range"):
            pl.run(INT32_MIN, 0)
        assert len(pl) == 0                                                   # nothing was appended by a refused call
        pl.add(rb, part["i"], part["j"], part["t_start"], part["reverse"])    # usable afterwards
        rb.close()                                                            # the hits outlive their batch
        o, hits = expect()
        sub = {k: (None if v is None else np.asarray(v)[:40]) for k, v in hits.items()}
        rows, flags = pl.run(INT32_MIN, GAP)
        want = py_place(sub, NR, INT32_MIN, GAP)
        assert len(pl) == 40 and np.array_equal(rows, want[0]) and np.array_equal(flags, want[1])
        with pytest.raises(ValueError, match="out of range"):
            al.placer(-1)
    finally:
        al.close()
        al2.close()


@pytest.mark.gpu
def test_seeds_to_placement_to_a_pileup_of_primaries(gpu):
    """seed_index -> seeds(n=4) -> place_windows -> pileup of the primaries.  A read from a unique region has mapq 60 and a primary
    interval that contains its true locus (its ends are never mutated: place_common.EDGE); the pileup's depth is the number of
    placed reads whose primary interval covers the base — a same-locus duplicate piled up as well would raise it."""
    kw = dict(span="ends-free", text_begin_free=40, text_end_free=40)
    wa = WavefrontAligner(**kw)
    with wa.sequence_set(READS) as R, wa.sequence_set(REFS) as G:
        with wa.seed_index(G, k=11) as index:
            s = index.seeds(R, n=4)
        qi, c = np.nonzero(s["j"] >= 0)
        wins = dict(i=qi.astype(np.int32), j=s["j"][qi, c], text_start=s["text_start"][qi, c], text_len=s["text_len"][qi, c], reverse=s["reverse"][qi, c])
        res = wa.place_windows(R, G, **wins)
        reads = res["reads"]
        for k, (r, pos, n, rev, touches) in enumerate(ORIGIN):
            if not touches:
                h = reads["hit"][k]
                assert h >= 0 and reads["mapq"][k] == 60, (k, {name: int(reads[name][k]) for name in COLUMNS})
                assert wins["j"][h] == r and wins["reverse"][h] == rev and reads["text_start"][k] <= pos and pos + n <= reads["text_end"][k], k
        placed = np.nonzero(reads["hit"] >= 0)[0]
        at = reads["hit"][placed]
        assert len(placed) >= 190 and (res["flag"][at] == 3).all()
        with wa.pileup(R, G, i=placed, j=wins["j"][at], text_start=wins["text_start"][at], text_len=wins["text_len"][at],
                       reverse=wins["reverse"][at]) as p:
            assert np.array_equal(p.score, reads["score"][placed]) and (p.status == 0).all()
            for r in range(len(REFS)):
                cover = np.zeros(len(REFS[r]), np.int32)
                for k in placed[wins["j"][at] == r]:
                    cover[reads["text_start"][k]:reads["text_end"][k]] += 1
                assert np.array_equal(p.depth(r), cover), (r, np.flatnonzero(p.depth(r) != cover)[:5])
