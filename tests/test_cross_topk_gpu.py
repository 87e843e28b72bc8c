"""Top-k per row of the score matrices on the GPU (WavefrontAligner.nearest, wfa_hip_cross_run_k / wfa_hip_cross_topk): for every
row, the k best cells with status 0 (all-vs-all: j != i), larger score first, ties to the smaller j, padded with j = -1 and
score = INT32_MIN — exactly what a host reference computes from score_matrix, across configurations, band and chunk sizes, ties,
read lengths and wildcards, and against completed_pairs on a large all-vs-all run."""
import os

import numpy as np
import pytest

from pywfa_amd import WavefrontAligner, _native

INT32_MIN = np.iinfo(np.int32).min


def families(seed, founders, copies, lo, hi, div=0.03, empty=2, alphabet="ACGT"):
    """Reads in families: random founders of lo..hi bases, copies with substitutions / insertions / deletions at `div`, shuffled,
    plus `empty` empty reads (as tests/test_cross_gpu.py)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(founders):
        f = list(rng.choice(list(alphabet), size=int(rng.integers(lo, hi + 1))))
        for _ in range(copies):
            s = []
            for ch in f:
                r = rng.random()
                if r < div / 3:
                    s.append(str(rng.choice(list("ACGT"))))
                elif r < 2 * div / 3:
                    continue
                elif r < div:
                    s += [ch, str(rng.choice(list("ACGT")))]
                else:
                    s.append(ch)
            out.append("".join(s))
    out += [""] * empty
    rng.shuffle(out)
    return out


def ref_topk(score, status, k, all_vs_all):
    """Host reference: per row, the eligible cells (status 0; all-vs-all: j != i) ordered by (-score, j), the first k, padded."""
    m, n = score.shape
    rj = np.full((m, k), -1, np.int32)
    rs = np.full((m, k), INT32_MIN, np.int32)
    for i in range(m):
        ok = status[i] == 0
        if all_vs_all and i < n:
            ok[i] = False
        cols = np.nonzero(ok)[0]
        sel = cols[np.lexsort((cols, -score[i, cols].astype(np.int64)))][:k]
        rj[i, :len(sel)] = sel
        rs[i, :len(sel)] = score[i, sel]
    return rj, rs


def assert_topk(got, ref, what=""):
    rj, rs = ref
    assert got["j"].dtype == np.int32 and got["score"].dtype == np.int32
    assert got["j"].shape == rj.shape and got["score"].shape == rs.shape, what
    assert np.array_equal(got["j"], rj), what
    assert np.array_equal(got["score"], rs), what


READS = families(11, 24, 5, 0, 300)            # 122 reads of 0-300 bases, two empty
READS_NE = [s for s in READS if len(s) >= 8]   # (free ends of up to 8 need reads at least that long)

GRID = [
    ("affine_default", dict()),
    ("affine_e2e", dict(span="end-to-end")),
    ("affine2p", dict(distance="affine2p", span="end-to-end")),
    ("edit", dict(distance="levenshtein", span="end-to-end")),
    ("indel", dict(distance="indel", span="end-to-end")),
    ("linear", dict(distance="linear", span="end-to-end")),
    ("match_neg", dict(match=-1, span="end-to-end")),
    ("ends_free_sym", dict(pattern_begin_free=5, pattern_end_free=8, text_begin_free=5, text_end_free=8)),
    ("ends_free_asym", dict(pattern_begin_free=8, pattern_end_free=0, text_begin_free=2, text_end_free=6)),
    ("adaptive", dict(heuristic="adaptive", span="end-to-end")),
    ("xdrop", dict(heuristic="X-drop", xdrop=30, span="end-to-end")),
    ("max_steps", dict(max_steps=40, span="end-to-end")),
    ("biwfa", dict(memory_mode="biwfa", span="end-to-end")),
    ("scope_full", dict(scope="full")),
]


def _reads_for(kw):
    return READS_NE if any(kw.get(k, 0) for k in ("pattern_begin_free", "pattern_end_free", "text_begin_free", "text_end_free")) else READS


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", GRID, ids=[g[0] for g in GRID])
def test_grid_all_vs_all_and_rectangle(gpu, name, kw):
    reads = _reads_for(kw)
    al = WavefrontAligner(**kw)
    score, status = al.score_matrix(reads)
    pats, texts = reads[:37], reads[37:]
    rs, rt = al.score_matrix(pats, texts)
    for k in (1, 5):
        assert_topk(al.nearest(reads, k=k), ref_topk(score, status, k, True), (name, "all-vs-all", k))
        assert_topk(al.nearest(pats, texts, k=k), ref_topk(rs, rt, k, False), (name, "rectangle", k))


@pytest.mark.gpu
def test_one_run_two_outputs(gpu):
    """One run with DENSE | TOPK (and COMPLETED | TOPK): the top-k is the reference's of that same run's own results."""
    al = WavefrontAligner(span="end-to-end", max_steps=60)
    pset = al._seqset(READS)
    tset = al._seqset(READS[:70])
    try:
        run = al._native.cross(pset, None, _native.CROSS_DENSE | _native.CROSS_TOPK, k=7)
        s, t = run.dense()
        assert_topk(run.topk(), ref_topk(s, t, 7, True))
        run.close()
        run = al._native.cross(pset, tset, _native.CROSS_DENSE | _native.CROSS_COMPLETED | _native.CROSS_TOPK, k=3)
        s, t = run.dense()
        c = run.completed()
        ii, jj = np.nonzero(t == 0)
        assert np.array_equal(c["i"], ii) and np.array_equal(c["j"], jj)
        assert_topk(run.topk(), ref_topk(s, t, 3, False))
        run.close()
    finally:
        pset.close()
        tset.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, "64"])
@pytest.mark.parametrize("band", [1, 37, 500])
def test_band_boundaries(gpu, band, chunk, monkeypatch):
    """Small bands (and chunks: the knobs are read when the aligner is created): column contributions of triangle bands merged over
    many bands, rows split into chunks, identical to the default sizes.  Mirror (end-to-end) and non-mirror (adaptive)."""
    for kw in (dict(span="end-to-end", max_steps=80), dict(heuristic="adaptive", span="end-to-end")):
        monkeypatch.delenv("WFA_HIP_CROSS_BAND", raising=False)
        monkeypatch.delenv("WFA_HIP_CROSS_TOPK_CHUNK", raising=False)
        base = WavefrontAligner(**kw)
        ref_a = base.nearest(READS, k=6)
        ref_r = base.nearest(READS[:50], READS[50:], k=6)
        s, t = base.score_matrix(READS)
        assert_topk(ref_a, ref_topk(s, t, 6, True), kw)
        monkeypatch.setenv("WFA_HIP_CROSS_BAND", str(band))
        if chunk:
            monkeypatch.setenv("WFA_HIP_CROSS_TOPK_CHUNK", chunk)
        al = WavefrontAligner(**kw)
        assert_topk(al.nearest(READS, k=6), (ref_a["j"], ref_a["score"]), (kw, band, chunk))
        assert_topk(al.nearest(READS[:50], READS[50:], k=6), (ref_r["j"], ref_r["score"]), (kw, band, chunk))


@pytest.mark.gpu
def test_rows_spanning_chunks_with_ties(gpu, monkeypatch):
    """3 queries x ~20 000 short reads with many exact duplicates at k = 64: ties resolve to the smallest j, whatever the chunks."""
    rng = np.random.default_rng(77)
    distinct = ["".join(rng.choice(list("ACGT"), size=int(rng.integers(12, 24)))) for _ in range(400)]
    texts = [distinct[int(x)] for x in rng.integers(0, 12, 8000)] + [distinct[int(x)] for x in rng.integers(0, 400, 12000)]
    rng.shuffle(texts)
    queries = [distinct[0], distinct[5], distinct[0][:-2] + "AC"]
    kw = dict(span="end-to-end")
    al = WavefrontAligner(**kw)
    s, t = al.score_matrix(queries, texts)
    ref = ref_topk(s, t, 64, False)
    assert (ref[1][:2] == 0).all()                       # (every one of the first 64 of the exact queries is a tie at 0)
    got = al.nearest(queries, texts, k=64)
    assert_topk(got, ref, "default chunk")
    for chunk in ("64", "320", "100000"):
        monkeypatch.setenv("WFA_HIP_CROSS_TOPK_CHUNK", chunk)
        assert_topk(WavefrontAligner(**kw).nearest(queries, texts, k=64), ref, chunk)
    # all-vs-all over the duplicates, rows split into chunks
    reads = texts[:3000]
    monkeypatch.setenv("WFA_HIP_CROSS_TOPK_CHUNK", "256")
    al = WavefrontAligner(**kw)
    s, t = al.score_matrix(reads)
    assert_topk(al.nearest(reads, k=64), ref_topk(s, t, 64, True), "all-vs-all")


@pytest.mark.gpu
def test_padding(gpu):
    al = WavefrontAligner(span="end-to-end")
    few = READS[:10]
    s, t = al.score_matrix(few)
    got = al.nearest(few, k=20)
    assert_topk(got, ref_topk(s, t, 20, True))
    assert (got["j"][:, 9:] == -1).all() and (got["score"][:, 9:] == INT32_MIN).all()
    s, t = al.score_matrix(few[:3], few)
    assert_topk(al.nearest(few[:3], few, k=11), ref_topk(s, t, 11, False))
    al = WavefrontAligner(span="end-to-end", max_steps=12)
    s, t = al.score_matrix(READS)
    got = al.nearest(READS, k=4)
    ref = ref_topk(s, t, 4, True)
    assert_topk(got, ref)
    filled = (got["j"] >= 0).sum(1)
    assert (filled == 0).any() and ((filled > 0) & (filled < 4)).any()


@pytest.mark.gpu
def test_long_reads_and_wildcards(gpu):
    long_reads = families(41, 4, 4, 600, 1200, div=0.02, empty=0) + families(42, 5, 4, 100, 300, empty=1)
    for kw in (dict(span="end-to-end"), dict(span="end-to-end", max_steps=400)):
        al = WavefrontAligner(**kw)
        s, t = al.score_matrix(long_reads)
        assert_topk(al.nearest(long_reads, k=5), ref_topk(s, t, 5, True), kw)
        s, t = al.score_matrix(long_reads[:6], long_reads[6:])
        assert_topk(al.nearest(long_reads[:6], long_reads[6:], k=5), ref_topk(s, t, 5, False), kw)
    wild = families(5, 8, 4, 20, 200, alphabet="ACGTN", empty=1) + families(6, 4, 3, 20, 200)
    for kw in (dict(wildcard="N"), dict(wildcard="N", span="end-to-end", max_steps=60)):
        al = WavefrontAligner(**kw)
        s, t = al.score_matrix(wild)
        assert_topk(al.nearest(wild, k=3), ref_topk(s, t, 3, True), kw)
        s, t = al.score_matrix(wild[:9], wild[9:])
        assert_topk(al.nearest(wild[:9], wild[9:], k=3), ref_topk(s, t, 3, False), kw)


def _section_6_4_reads():
    """DESIGN §6.4's workload (tools/probes/cross_scores.py): 256 founders x 16 copies of 150 bp at 2 %, shuffled."""
    rng = np.random.default_rng(2024)
    reads = []
    for _ in range(256):
        f = rng.integers(0, 4, 150)
        for _ in range(16):
            r = rng.random(150)
            sub = rng.integers(0, 4, 150)
            out = []
            for k in range(150):
                if r[k] < 0.02 / 3:
                    out.append(sub[k])
                elif r[k] < 0.04 / 3:
                    continue
                elif r[k] < 0.02:
                    out += [f[k], sub[k]]
                else:
                    out.append(f[k])
            reads.append("".join("ACGT"[x] for x in out))
    order = rng.permutation(len(reads))
    return [reads[k] for k in order]


@pytest.mark.gpu
def test_repeatable_and_equal_to_completed_pairs(gpu):
    """The 4 096-read workload at k = 8: two calls agree, and equal a top-k built from completed_pairs mirrored to both (i, j) and
    (j, i) — no dense matrix anywhere."""
    reads = _section_6_4_reads()
    n, k = len(reads), 8
    al = WavefrontAligner(span="end-to-end", scope="score", max_steps=90)
    a = al.nearest(reads, k=k)
    b = al.nearest(reads, k=k)
    assert np.array_equal(a["j"], b["j"]) and np.array_equal(a["score"], b["score"])
    c = al.completed_pairs(reads)
    rows = np.concatenate([c["i"], c["j"]]).astype(np.int64)
    cols = np.concatenate([c["j"], c["i"]]).astype(np.int64)
    sc = np.concatenate([c["score"], c["score"]]).astype(np.int64)
    order = np.lexsort((cols, -sc, rows))
    rows, cols, sc = rows[order], cols[order], sc[order]
    start = np.searchsorted(rows, np.arange(n))
    rank = np.arange(len(rows)) - start[rows]
    keep = rank < k
    rj = np.full((n, k), -1, np.int32)
    rs = np.full((n, k), INT32_MIN, np.int32)
    rj[rows[keep], rank[keep]] = cols[keep]
    rs[rows[keep], rank[keep]] = sc[keep]
    assert len(c["i"]) > n
    assert_topk(a, (rj, rs))


@pytest.mark.gpu
def test_errors(gpu):
    al = WavefrontAligner(span="end-to-end")
    for k in (0, 65, 2.5, -3):
        with pytest.raises(ValueError):
            al.nearest(READS[:5], k=k)
    with pytest.raises(ValueError, match="Ends-free"):
        WavefrontAligner(pattern_begin_free=10).nearest(["ACGTACGTACGTACGT", "ACGT"], k=1)
    cfg = _native.default_config()
    cfg.scope = 0
    na = _native.Aligner(cfg)
    try:
        blob = np.frombuffer(b"ACGTTACGTA" + b"\0" * 64, np.uint8)
        s = na.seqset(blob, np.array([0, 5], np.int64), np.array([5, 5], np.int32))
        with pytest.raises(ValueError, match="want"):   # the TOPK bit through the old entry point
            na.cross(s, None, _native.CROSS_TOPK)
        with pytest.raises(ValueError, match="want"):
            na.cross(s, None, _native.CROSS_DENSE | _native.CROSS_TOPK)
        for bad in (0, 65):
            with pytest.raises(ValueError, match="k"):
                na.cross(s, None, _native.CROSS_TOPK, k=bad)
        with pytest.raises(ValueError, match="want"):
            na.cross(s, None, 8, k=1)
        run = na.cross(s, None, _native.CROSS_DENSE, k=0)   # (k is read only with TOPK)
        j = np.zeros((2, 1), np.int32)
        sc = np.zeros((2, 1), np.int32)
        assert _native.lib().wfa_hip_cross_topk(run._h, j.ctypes.data, sc.ctypes.data) == _native.EINVAL
        with pytest.raises(ValueError):
            run.topk()
        run.close()
        run = na.cross(s, None, _native.CROSS_DENSE)
        assert _native.lib().wfa_hip_cross_topk(run._h, j.ctypes.data, sc.ctypes.data) == _native.EINVAL
        run.close()
        s.close()
    finally:
        na.close()


@pytest.mark.gpu
def test_empty_sets(gpu):
    al = WavefrontAligner()
    r = al.nearest([], k=3)
    assert r["j"].shape == (0, 3) and r["score"].shape == (0, 3)
    r = al.nearest([], ["ACGT"], k=2)
    assert r["j"].shape == (0, 2)
    for r in (al.nearest(["ACGT", "AC"], [], k=4), al.nearest(["ACGT"], k=4)):
        m = r["j"].shape[0]
        assert r["j"].shape == (m, 4) and (r["j"] == -1).all() and (r["score"] == INT32_MIN).all()
