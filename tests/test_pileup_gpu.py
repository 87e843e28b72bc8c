"""Pileups reduced on the GPU (wfa_hip_pileup_*, WavefrontAligner.pileup): every row of every reference equals the table built on the
host, by the Python restatement of the rule, from the ORACLE's op strings of the materialised pairs — through the C ABI (two adds, a
clear), through pileup() in one chunk and in several, with min_score, with texts=None, with the sets closed, and under a step limit
whose unfinished pairs must not contribute.  Exact equality."""
import numpy as np
import pytest

from common import configs_pair
from oracle import loader
from pywfa_amd import WavefrontAligner, _native, datagen
from reduce_common import expected_tables
from test_windows_gpu import LETTERS, as_list, materialise, mutate, native_set, native_windows, revcomp

KW = dict(span="ends-free", text_begin_free=20, text_end_free=20)
KW_STEPS = dict(KW, max_steps=50)


def corpus(seed=31, nreads=2400):
    """The shape of test_windows_gpu's corpus at ~20x depth: four references of 3-6 kb, the last with N runs; reads of 100-200 bases
    cut from random positions (from the bases under the Ns too), mutated at 3 %, every second one stored reverse-complemented, a few
    holding an N of their own."""
    rng = np.random.default_rng(seed)
    bases = [rng.integers(0, 4, n) for n in (3000, 4500, 6000, 4011)]
    refs = ["".join(LETTERS[b]) for b in bases]
    last = list(refs[3])
    for a, b in [(0, 7), (500, 501), (1200, 1216), (2000, 2100), (4000, 4011)]:
        last[a:b] = "N" * (b - a)
    refs[3] = "".join(last)
    reads, rows = [], []
    for k in range(nreads):
        r = int(rng.integers(0, 4))
        n = int(rng.integers(100, 201))
        pos = int(rng.integers(0, len(bases[r]) - n + 1))
        s = "".join(LETTERS[mutate(rng, bases[r][pos:pos + n], 0.03)])
        if k % 37 == 0:
            s = s[:50] + "N" + s[51:]
        rev = k % 2 == 1
        reads.append(revcomp(s) if rev else s)
        t0, t1 = max(0, pos - int(rng.integers(0, 21))), min(len(refs[r]), pos + n + int(rng.integers(0, 21)))
        rows.append((k, r, 0, len(s), t0, t1 - t0, int(rev)))
    return refs, reads, as_list(rows)


REFS, READS, W = corpus()
N = len(W["i"])


def oracle_of(kw, P, T, Wl):
    pats, txts = materialise(P, T, Wl)
    batch = datagen.from_strings(pats, txts, upper=True)
    return loader.run(loader.oracle(), loader.make_config(**kw), batch), pats


def expect(kw, keep=None):
    o, pats = oracle_of(kw, READS, REFS, W)
    tables, cover = expected_tables([len(r) for r in REFS], o, pats, W["j"], W["t_start"], W["t_len"], keep(o) if keep else None)
    return o, tables, cover


def same_tables(read, tables, ctx):
    for r, want in enumerate(tables):
        got = read(r)
        assert got.dtype == np.int32 and got.shape == want.shape, (ctx, r)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (ctx, r, int(bad[0]), got[bad[0]], want[bad[0]], bad.size)


def test_corpus_covers_what_it_should():
    """No GPU: the conditions on the inputs, from the oracle's results."""
    assert N >= 2000 and 0.4 <= W["reverse"].mean() <= 0.6
    o, tables, cover = expect(KW)
    assert (np.asarray(o["status"]) == 0).all()
    total = sum(t.sum(axis=0) for t in tables)
    assert (total > 0).all(), total                            # every column is used somewhere
    depth = np.concatenate(cover)
    assert 15 <= depth.mean() <= 25, depth.mean()
    o, tables, _ = expect(KW_STEPS)
    stopped = int((np.asarray(o["status"]) != 0).sum())
    assert 1 <= stopped <= N // 2, stopped


def pileup_kwargs(Wl=None):
    Wl = W if Wl is None else Wl
    return dict(i=Wl["i"], j=Wl["j"], pattern_start=Wl["p_start"], pattern_len=Wl["p_len"], text_start=Wl["t_start"], text_len=Wl["t_len"],
                reverse=Wl["reverse"])


@pytest.mark.gpu
def test_c_abi_two_adds_and_a_clear(gpu):
    o, tables, _ = expect(KW)
    _, nc = configs_pair(**KW)
    al = _native.Aligner(nc)
    try:
        ps, ts = native_set(al, READS), native_set(al, REFS)
        pile = al.pileup(ts)
        same_tables(pile.read, [np.zeros_like(t) for t in tables], "zeroed")
        half = N // 2 + 13
        parts = [{k: v[lo:hi] for k, v in W.items()} for lo, hi in ((0, half), (half, N))]
        batches = []
        for part in parts:
            rb = native_windows(al, ps, ts, part)
            rb.run()
            pile.add(rb, part["j"], part["t_start"])             # (waits for the run itself)
            batches.append(rb)
        ps.close()
        ts.close()                                               # the pileup and the batches outlive the sets
        same_tables(pile.read, tables, "two adds")
        assert np.array_equal(pile.read(2, 100, 50), tables[2][100:150]) and pile.read(1, 4500, 0).shape == (0, 8)
        pile.clear()
        same_tables(pile.read, [np.zeros_like(t) for t in tables], "cleared")
        # in the other order, one of them twice: integer adds
        keep = [np.arange(len(p["i"])) % 3 != 0 for p in parts]
        for k in (1, 0, 1):
            pile.add(batches[k], parts[k]["j"], parts[k]["t_start"], keep[k])
        pats = oracle_of(KW, READS, REFS, W)[1]
        k_all = np.concatenate(keep)
        once, _ = expected_tables([len(r) for r in REFS], o, pats, W["j"], W["t_start"], W["t_len"], k_all)
        k_second = np.concatenate([np.zeros(half, bool), keep[1]])
        twice, _ = expected_tables([len(r) for r in REFS], o, pats, W["j"], W["t_start"], W["t_len"], k_second)
        same_tables(pile.read, [a + b for a, b in zip(once, twice)], "keep, three adds")
        for rb in batches:
            rb.close()
        pile.close()
    finally:
        al.close()


def check_handle(p, o, tables, cover, ctx, ref=1):
    assert p.COLUMNS == ("A", "C", "G", "T", "other", "del", "ins", "mismatch") and len(p) == len(tables)
    assert np.array_equal(p.score, o["score"]) and np.array_equal(p.status, o["status"]), ctx
    same_tables(p.counts, tables, ctx)
    for r in range(len(tables)):
        assert np.array_equal(p.depth(r), cover[r]), (ctx, "depth", r)      # the contributing pairs whose core covers the base
    assert np.array_equal(p.counts(ref, 10, 300), tables[ref][10:300]) and np.array_equal(p.depth(ref, 10, 300), cover[ref][10:300])


@pytest.mark.gpu
def test_pileup_one_chunk_and_several(gpu, monkeypatch):
    o, tables, cover = expect(KW)
    wa = WavefrontAligner(**KW)
    with wa.pileup(READS, REFS, **pileup_kwargs()) as p:
        check_handle(p, o, tables, cover, "one chunk")
    with pytest.raises(ValueError, match="closed"):
        p.counts(0)
    monkeypatch.setenv("WFA_HIP_PAIRS_BAND", "700")
    p = wa.pileup(READS, REFS, **pileup_kwargs())
    check_handle(p, o, tables, cover, "chunks of 700")
    p.close()
    p.close()
    with pytest.raises(ValueError, match="closed"):
        p.depth(0)


@pytest.mark.gpu
def test_min_score_and_closed_sets(gpu):
    scores = loader.run(loader.oracle(), loader.make_config(**KW), datagen.from_strings(*materialise(READS, REFS, W), upper=True))["score"]
    bar = int(np.median(scores))
    o, tables, cover = expect(KW, keep=lambda o: np.asarray(o["score"]) >= bar)
    assert 0.3 * N < (np.asarray(o["score"]) >= bar).sum() < N
    wa = WavefrontAligner(**KW)
    with wa.sequence_set(READS) as R, wa.sequence_set(REFS) as G:
        p = wa.pileup(R, G, min_score=bar, **pileup_kwargs())
        other = wa.align_windows(R, G, **pileup_kwargs())            # the sets serve other calls in between
        assert np.array_equal(other["score"], o["score"])
    check_handle(p, o, tables, cover, "min_score, sets closed")          # both sets are closed by now
    p.close()
    with pytest.raises(ValueError, match="closed"):
        wa.pileup(R, G, **pileup_kwargs())


@pytest.mark.gpu
def test_texts_none(gpu):
    """One set: the reads and the references together, windows of it against windows of it; the reads' own rows stay zero."""
    both = READS + REFS
    Wl = dict(W, j=(W["j"] + len(READS)).astype(np.int32))
    o, pats = oracle_of(KW, both, None, Wl)
    tables, cover = expected_tables([len(s) for s in both], o, pats, Wl["j"], Wl["t_start"], Wl["t_len"])
    assert not any(t.any() for t in tables[:len(READS)])
    wa = WavefrontAligner(**KW)
    with wa.pileup(both, **pileup_kwargs(Wl)) as p:
        check_handle(p, o, tables, cover, "texts=None", ref=len(READS) + 1)


@pytest.mark.gpu
def test_step_limit(gpu):
    o, tables, cover = expect(KW_STEPS)
    stopped = np.asarray(o["status"]) != 0
    assert 1 <= stopped.sum() <= N // 2
    with WavefrontAligner(**KW_STEPS).pileup(READS, REFS, **pileup_kwargs()) as p:
        check_handle(p, o, tables, cover, "step limit")
        assert int(sum(p.depth(r).sum() for r in range(4))) == int(sum(c.sum() for c in cover))


@pytest.mark.gpu
def test_refusals(gpu):
    _, nc = configs_pair(**KW)
    ns = nc.copy()
    ns.scope = 0
    part = {k: v[:60] for k, v in W.items()}
    al, al2 = _native.Aligner(nc), _native.Aligner(nc)
    try:
        ps, ts, foreign = native_set(al, READS), native_set(al, REFS), native_set(al2, REFS)
        with pytest.raises(ValueError, match="another aligner"):
            al.pileup(foreign)
        pile = al.pileup(ts)
        rb = native_windows(al, ps, ts, part)
        with pytest.raises(ValueError, match="pileup needs a finished run"):
            pile.add(rb, part["j"], part["t_start"])
        rb.run()
        rb.sync()
        j, t0 = part["j"].copy(), part["t_start"].copy()
        j[11] = 4
        with pytest.raises(ValueError, match=r"text index out of range at position 11 of the pair list: j = 4 over a set of 4 sequences"):
            pile.add(rb, j, t0)
        j[11] = -1
        with pytest.raises(ValueError, match=r"position 11 of the pair list: j = -1 "):
            pile.add(rb, j, t0)
        j = part["j"].copy()
        t0[7] = -5
        with pytest.raises(ValueError, match=r"negative text start at position 7 of the pair list: t_start = -5"):
            pile.add(rb, j, t0)
        t0 = part["t_start"].copy()
        t0[23] = len(REFS[j[23]]) - part["t_len"][23] + 1
        with pytest.raises(ValueError, match=rf"text window out of range at position 23 of the pair list: \[{t0[23]}, {t0[23]} \+ {part['t_len'][23]}\) "
                                             rf"of sequence {j[23]} \({len(REFS[j[23]])} bases\)"):
            pile.add(rb, j, t0)
        with pytest.raises(ValueError, match="one value per pair"):
            pile.add(rb, j[:-1], t0[:-1])
        rb2 = native_windows(al2, native_set(al2, READS), foreign, part)
        rb2.run()
        rb2.sync()
        with pytest.raises(ValueError, match="batch of another aligner"):
            pile.add(rb2, part["j"], part["t_start"])
        al.set_config(ns)
        rs = native_windows(al, ps, ts, part)
        rs.run()
        rs.sync()
        with pytest.raises(ValueError, match="pileup needs scope=full"):
            pile.add(rs, part["j"], part["t_start"])
        al.set_config(nc)
        same_tables(pile.read, [np.zeros((len(r), 8), np.int32) for r in REFS], "nothing was added by a refused call")
        for bad in ((4, 0, 1), (-1, 0, 1), (0, -1, 5), (0, 2990, 11), (0, 0, 3001)):
            with pytest.raises(ValueError, match="out of range"):
                pile.read(*bad)
        pile.add(rb, part["j"], part["t_start"])                      # usable afterwards
        assert sum(int(pile.read(r).sum()) for r in range(4)) > 0
    finally:
        al.close()
        al2.close()
    with pytest.raises(ValueError, match="pileup needs scope='full'"):
        WavefrontAligner(scope="score").pileup(READS, REFS, **pileup_kwargs())
