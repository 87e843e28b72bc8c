"""Pairing of reads on the GPU (wfa_hip_placer_run_pairs, WavefrontAligner.place_pairs): rows and flags equal the host statement
wfa_hip_pair_host on the random lists and the hand-written edges of test_pair_abi.py and on a list shaped for the wave loop, and the
Python restatement fed with the ORACLE's scores, statuses and aligned cores on the paired corpus — under both scopes, in one chunk and
in several, with texts=None.  Exact equality.  For the repeat fragments of the corpus the outcome is also held to the generator's truth."""
import numpy as np
import pytest

from common import configs_pair
from oracle import loader
from pair_common import INT32_MIN, PAIR_COLUMNS, as_hit_arrays, pair_corpus, py_pair, random_case
from place_common import COLUMNS, hits_of
from pywfa_amd import WavefrontAligner, _native, datagen
from test_pair_abi import EDGES, PAR
from test_windows_gpu import materialise

KW = dict(span="ends-free", text_begin_free=20, text_end_free=20)
REFS, READS, W, TRUTH = pair_corpus()
NR, NF = len(READS), len(TRUTH)
GAP = 24
HIT_KEYS = ("i", "j", "reverse", "score", "status", "text_start", "text_end")
_ORACLE = {}


def expect(full=True, P=READS, T=REFS, Wl=W, key=None):
    """(oracle results, hit list) of the corpus under a scope: computed once, never changed."""
    key = key or full
    if key not in _ORACLE:
        pats, txts = materialise(P, T, Wl)
        o = loader.run(loader.oracle(), loader.make_config(**dict(KW, scope="full" if full else "score")), datagen.from_strings(pats, txts, upper=True))
        _ORACLE[key] = (o, hits_of(o, Wl, full))
    return _ORACLE[key]


def window_kwargs(Wl=W):
    return dict(i=Wl["i"], j=Wl["j"], pattern_start=Wl["p_start"], pattern_len=Wl["p_len"], text_start=Wl["t_start"], text_len=Wl["t_len"],
                reverse=Wl["reverse"])


def host(nreads, a, mates, **par):
    return _native.pair_host(nreads, *[a[k] for k in HIT_KEYS], mates, **par)


def device(al, nreads, a, mates, cut=None, **par):
    """add_hits (in two adds when `cut` is given) + run_pairs on a fresh placer."""
    pl = al.placer(nreads)
    try:
        n = len(a["i"])
        for lo, hi in ((0, n),) if cut is None else ((0, cut), (cut, n)):
            pl.add_hits(*[None if a[k] is None else a[k][lo:hi] for k in HIT_KEYS])
        return pl.run_pairs(mates, **par)
    finally:
        pl.close()


def same(got, want, ctx):
    for name, g, w in zip(("rows", "flags", "pair_rows", "pair_flags"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (ctx, name)
        if g.ndim == 2:
            bad = np.flatnonzero((g != w).any(axis=1))
            assert bad.size == 0, (ctx, name, int(bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist(), bad.size)
        else:
            assert np.array_equal(g, w), (ctx, name, np.flatnonzero(g != w)[:5])


SPECIAL = [(0, 5), (5, 0), (1, 1), (63, 1), (1, 63), (64, 1), (1, 64), (65, 1), (130, 1), (7, 9), (8, 8), (5, 13), (63, 65), (64, 64), (65, 64),
           (130, 130), (256, 256), (257, 256), (256, 257), (300, 300)]


def wave_shaped(seed=4, nfrag=20011):
    """20 011 interleaved fragments, more than the grid has waves and no multiple of it: the first ones with the group sizes SPECIAL
    (every hit eligible: pairings of 0, 1, 63, 64, 65 and 130 on a side, products just under and over 64, at the cap of 65 536 and
    over it), the others with 0, 1, 2 or 3 hits a mate, a tenth of them ineligible.  Mate 1 mostly forward, mate 2 mostly reverse, two
    texts, intervals of 0, 100 or 150 bases that start on a grid of 50, scores from a small range; all hits in shuffled order."""
    rng = np.random.default_rng(seed)
    size = rng.choice([0, 1, 2, 3], 2 * nfrag, p=[0.1, 0.5, 0.3, 0.1])
    for f, (n1, n2) in enumerate(SPECIAL):
        size[2 * f], size[2 * f + 1] = n1, n2
    i = rng.permutation(np.repeat(np.arange(2 * nfrag), size)).astype(np.int32)
    n = len(i)
    ts = 50 * rng.integers(0, 8, n)
    status = ((rng.random(n) < 0.1) * rng.integers(1, 3, n)).astype(np.int32)
    status[i < 2 * len(SPECIAL)] = 0
    hits = dict(i=i, j=(rng.random(n) < 0.15).astype(np.int32), reverse=np.where(rng.random(n) < 0.85, i % 2, 1 - i % 2).astype(np.uint8),
                score=(-4 * rng.integers(0, 6, n)).astype(np.int32), status=status, text_start=ts.astype(np.int32),
                text_end=(ts + rng.choice([0, 100, 150, 150], n)).astype(np.int32))
    return 2 * nfrag, hits, nfrag


@pytest.mark.gpu
def test_run_pairs_equals_the_host_statement_on_random_lists_and_edges(gpu):
    _, nc = configs_pair(**KW)
    al = _native.Aligner(nc)
    try:
        rng = np.random.default_rng(2025)
        for k in range(150):
            nreads, hits, mates, par = random_case(rng)
            a = as_hit_arrays(hits)
            same(device(al, nreads, a, mates, cut=len(a["i"]) // 3, **par), host(nreads, a, mates, **par), ("random", k, mates, par))
        for name, hits, nreads, mates, change, rows, pair_flags in EDGES:
            a = as_hit_arrays(hits)
            par = dict(PAR, **change)
            got = device(al, nreads, a, mates, **par)
            same(got, host(nreads, a, mates, **par), name)
            assert np.array_equal(got[2], np.array(rows, np.int64).reshape(-1, 12)) and got[3].tolist() == list(pair_flags), name
    finally:
        al.close()


@pytest.mark.gpu
def test_run_pairs_on_groups_around_the_wave_width(gpu):
    nreads, h, nfrag = wave_shaped()
    sizes = np.bincount(h["i"], minlength=nreads)
    assert [(sizes[2 * f], sizes[2 * f + 1]) for f in range(len(SPECIAL))] == SPECIAL and 35000 <= len(h["i"]) <= 60000
    par = dict(min_score=INT32_MIN, full_gap=GAP, min_insert=100, max_insert=400, unpaired=8)
    want = host(nreads, h, nfrag, **par)
    pr = want[2]
    # what the list is for: overflow exactly where E1 E2 > 65 536, joins at the cap, every kind of outcome among the small fragments
    assert pr[:len(SPECIAL), 11].tolist() == [int(a * b > 65536) for a, b in SPECIAL] and pr[16, 9] > 0 and not pr[len(SPECIAL):, 11].any()
    assert (pr[:, 2] == 1).sum() >= 2000 and ((pr[:, 2] == 0) & (pr[:, 9] > 0)).sum() >= 20 and (pr[:, 10] > 0).sum() >= 50
    assert ((pr[:, 5] > 0) & (pr[:, 5] < 60)).sum() >= 100 and (want[3] != want[1]).sum() >= 100
    _, nc = configs_pair(**KW)
    al = _native.Aligner(nc)
    try:
        pl = al.placer(nreads)
        assert pl.kernel_ms() == 0.0
        pl.add_hits(*[h[k] for k in HIT_KEYS])
        before = pl.run(INT32_MIN, GAP)                                      # a single-end run in front ...
        got = pl.run_pairs(nfrag, **par)
        same(got, want, "wave-shaped")
        assert pl.kernel_ms() > 0.0
        again = pl.run_pairs(nfrag, **par)                                   # two runs: identical bytes
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
        after = pl.run(INT32_MIN, GAP)                                       # ... and one behind give what they give today
        ref = _native.place_host(nreads, *[h[k] for k in HIT_KEYS], INT32_MIN, GAP)
        for x in (before, after, got[:2]):
            assert np.array_equal(x[0], ref[0]) and np.array_equal(x[1], ref[1])
        # other parameters and mates as a shuffled array over some of the reads, the nullable outputs left out; nothing re-added
        perm = np.random.default_rng(1).permutation(nreads)[:2 * 9001].reshape(-1, 2)
        par2 = dict(min_score=-12, full_gap=5, min_insert=0, max_insert=1000, unpaired=0)
        want2 = host(nreads, h, perm, **par2)
        r, f, p2, pf = pl.run_pairs(perm, rows=False, flags=False, pair_flags=False, **par2)
        assert r is None and f is None and pf is None and np.array_equal(p2, want2[2])
        same(pl.run_pairs(perm, **par2), want2, "shuffled mates")
        # an add after a run: the next run sees every hit
        extra = dict(i=[40, 41], j=[0, 0], reverse=[0, 1], score=[4, 4], status=[0, 0], text_start=[0, 100], text_end=[150, 250])
        pl.add_hits(*[extra[k] for k in HIT_KEYS])
        both = {k: np.concatenate([h[k], np.asarray(extra[k], h[k].dtype)]) for k in h}
        got3 = pl.run_pairs(nfrag, **par)
        same(got3, host(nreads, both, nfrag, **par), "after an add")
        assert got3[2][20, :3].tolist() == [len(h["i"]), len(h["i"]) + 1, 1] and got3[2][20, 8] == 250
        pl.close()
    finally:
        al.close()


def check(res, o, hits, nreads, mates, min_score, full_gap, min_insert, max_insert, unpaired, ctx):
    rows, flags, pair_rows, pair_flags = py_pair(hits, nreads, mates, min_score, full_gap, min_insert, max_insert, unpaired)
    assert np.array_equal(res["score"], o["score"]) and np.array_equal(res["status"], o["status"]), ctx
    assert np.array_equal(res["flag"], flags) and res["pair_flag"].dtype == np.uint8 and np.array_equal(res["pair_flag"], pair_flags), ctx
    assert tuple(res["reads"]) == COLUMNS and tuple(res["pairs"]) == PAIR_COLUMNS, ctx
    for c, name in enumerate(COLUMNS):
        assert np.array_equal(res["reads"][name], rows[:, c]), (ctx, name)
    for c, name in enumerate(PAIR_COLUMNS):
        got = res["pairs"][name]
        assert got.dtype == np.int32 and got.shape == (pair_rows.shape[0],), (ctx, name)
        bad = np.flatnonzero(got != pair_rows[:, c])
        assert bad.size == 0, (ctx, name, int(bad[0]), int(got[bad[0]]), pair_rows[bad[0]].tolist(), bad.size)
    return pair_rows


def truth_holds(res, Wl, ctx):
    """Against the generator, not the code under test: every repeat fragment is proper, mate 1 sits at the copy next to mate 2 (not at
    its image in the other copy) although on its own it has mapq 0, and the pairing lifts its mapq."""
    pairs, reads = res["pairs"], res["reads"]
    seen = 0
    for f, (r, left, outer, flip, repeat, (r1, pos1), (r2, pos2), image) in enumerate(TRUTH):
        if not repeat:
            continue
        seen += 1
        h1, h2 = int(pairs["hit1"][f]), int(pairs["hit2"][f])
        assert pairs["proper"][f] == 1 and h1 >= 0 and h2 >= 0, (ctx, f)
        assert Wl["i"][h1] == 2 * f and Wl["i"][h2] == 2 * f + 1, (ctx, f)
        assert Wl["j"][h1] == r1 and abs(int(Wl["t_start"][h1]) - pos1) <= 10 and Wl["j"][h2] == r2, (ctx, f, h1, image)
        assert reads["mapq"][2 * f] == 0 and pairs["mapq1"][f] > 0, (ctx, f, int(reads["mapq"][2 * f]), int(pairs["mapq1"][f]))
    assert seen == NF // 5, ctx


@pytest.mark.gpu
def test_place_pairs_full_scope(gpu):
    o, hits = expect()
    wa = WavefrontAligner(**KW)
    res = wa.place_pairs(READS, REFS, **window_kwargs())                       # interleaved; full_gap 24 and unpaired = full_gap
    pr = check(res, o, hits, NR, NF, INT32_MIN, GAP, 0, 1000, GAP, "full, defaults")
    truth_holds(res, W, "full")
    assert (pr[:, 2] == 1).sum() >= 90 and (res["pair_flag"] != res["flag"]).sum() >= 5
    for f, t in enumerate(TRUTH):                                              # the insert of a proper fragment is its outer length
        if pr[f, 2] == 1 and W["j"][pr[f, 0]] == t[0] and abs(int(W["t_start"][pr[f, 0]]) - t[5][1]) <= 10:
            assert pr[f, 8] == t[2], (f, pr[f].tolist(), t)
    check(wa.place_pairs(READS, REFS, min_score=-40, full_gap=7, min_insert=250, max_insert=400, unpaired=0, **window_kwargs()),
          o, hits, NR, NF, -40, 7, 250, 400, 0, "full, parameters")


@pytest.mark.gpu
def test_place_pairs_score_scope(gpu):
    o, hits = expect(full=False)
    res = WavefrontAligner(scope="score", **KW).place_pairs(READS, REFS, full_gap=GAP, **window_kwargs())
    check(res, o, hits, NR, NF, INT32_MIN, GAP, 0, 1000, GAP, "score")
    truth_holds(res, W, "score")


@pytest.mark.gpu
def test_chunks_give_the_one_chunk_output(gpu, monkeypatch):
    o, hits = expect()
    wa = WavefrontAligner(**KW)
    with wa.sequence_set(READS) as R, wa.sequence_set(REFS) as G:
        one = wa.place_pairs(R, G, **window_kwargs())
        monkeypatch.setenv("WFA_HIP_PAIRS_BAND", "97")                         # (the list is shuffled: every group straddles chunks)
        many = wa.place_pairs(R, G, **window_kwargs())
    check(many, o, hits, NR, NF, INT32_MIN, GAP, 0, 1000, GAP, "chunks of 97")
    assert many["pair_flag"].tobytes() == one["pair_flag"].tobytes() and many["flag"].tobytes() == one["flag"].tobytes()
    for name in PAIR_COLUMNS:
        assert many["pairs"][name].tobytes() == one["pairs"][name].tobytes(), name


@pytest.mark.gpu
def test_texts_none_and_mates_as_an_array(gpu):
    """One set, the references behind the reads (an odd number of sequences: interleaved mates are refused), the fragments listed
    backwards over the reads."""
    both = READS + REFS
    Wl = dict(W, j=(W["j"] + NR).astype(np.int32))
    o, hits = expect(P=both, T=None, Wl=Wl, key="texts=None")
    wa = WavefrontAligner(**KW)
    with pytest.raises(ValueError, match="an odd number"):
        wa.place_pairs(both, **window_kwargs(Wl))
    mates = np.arange(NR).reshape(-1, 2)[::-1]
    res = wa.place_pairs(both, mates=mates, **window_kwargs(Wl))
    check(res, o, hits, len(both), mates, INT32_MIN, GAP, 0, 1000, GAP, "texts=None")
    assert (res["pairs"]["hit1"][::-1] >= 0).all() and (res["reads"]["hit"][NR:] == -1).all()


@pytest.mark.gpu
def test_refusals_launch_nothing(gpu):
    wa = WavefrontAligner(**KW)
    for bad, msg in ((dict(full_gap=0), "full_gap = 0 is out of range"), (dict(min_insert=-1), "min_insert = -1, max_insert = 1000 are out of range"),
                     (dict(min_insert=5, max_insert=4), "are out of range"), (dict(max_insert=2.5), "max_insert must be an integer"),
                     (dict(unpaired=-1), "unpaired = -1 is out of range"), (dict(unpaired="x"), "unpaired must be an integer or None"),
                     (dict(min_score=2**31), "does not fit 32 bits"), (dict(mates=[0, 1]), r"shape \(F, 2\)"),
                     (dict(mates=[[0, 1], [2, NR]]), rf"mates\[1\] = \(2, {NR}\) is out of range"),
                     (dict(mates=[[0, 1], [3, 3]]), r"mates\[1\] = \(3, 3\): the two mates are one read"),
                     (dict(mates=[[0, 1], [2, 1]]), r"mates\[1\] = \(2, 1\): read 1 belongs to an earlier fragment"),
                     (dict(mates=[[0.5, 1]]), r"shape \(F, 2\)")):
        with pytest.raises(ValueError, match=msg):
            wa.place_pairs(READS, REFS, **dict(window_kwargs(), **bad))
    _, nc = configs_pair(**KW)
    al = _native.Aligner(nc)
    try:
        pl = al.placer(4)
        pl.add_hits([0, 1], [0, 0], [0, 1], [-4, -4], [0, 0], [100, 300], [250, 450])
        for mates, change, msg in ((1, dict(full_gap=0), "full_gap = 0 is out of range"), (1, dict(min_insert=-1), "min_insert = -1"),
                                   (1, dict(max_insert=-1), "max_insert = -1"), (1, dict(unpaired=-1), "unpaired = -1 is out of range"),
                                   (-1, {}, r"a negative number of fragments \(-1\)"), (3, {}, "3 interleaved fragments need 6 reads, there are 4"),
                                   ([[0, 4]], {}, "mate out of range at fragment 0: mate2 = 4 over 4 reads"),
                                   ([[2, 2]], {}, "the mates of fragment 0 are one read: mate1 = mate2 = 2"),
                                   ([[0, 1], [1, 2]], {}, "read 1 is named by two fragments, the second time at fragment 1 as mate1")):
            with pytest.raises(ValueError, match=msg):
                pl.run_pairs(mates, **dict(PAR, **change))
        L = _native.lib()
        m = np.zeros(1, np.int32)
        out = np.full((1, 12), 7, np.int32)
        assert L.wfa_hip_placer_run_pairs(pl._h, INT32_MIN, 24, 0, 1000, 0, 1, m.ctypes.data, None, None, None, out.ctypes.data, None) == _native.EINVAL
        assert "mate2 is missing" in al.error()
        assert L.wfa_hip_placer_run_pairs(pl._h, INT32_MIN, 24, 0, 1000, 0, 1, None, None, None, None, None, None) == _native.EINVAL
        assert (out == 7).all() and pl.kernel_ms() == 0.0 and len(pl) == 2       # no kernel has run, nothing was written
        r, f, pr, pf = pl.run_pairs(1, **PAR)                                   # usable afterwards
        assert pr.tolist() == [[0, 1, 1, -8, INT32_MIN, 60, 60, 60, 350, 1, 0, 0]] and pf.tolist() == [3, 3] and pl.kernel_ms() > 0.0
        assert pl.run_pairs(0, **PAR)[2].shape == (0, 12)
        pl.close()
    finally:
        al.close()
