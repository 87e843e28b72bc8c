"""Score matrices on the GPU (WavefrontAligner.score_matrix / completed_pairs, wfa_hip_cross_run): every cell equals what the explicit
batch path gives for that pair with scope="score", in all-vs-all and in rectangular mode, across configurations, band sizes and read
lengths; the completed-pairs list is the dense result filtered and ordered row-major."""
import os

import numpy as np
import pytest

from oracle import loader
from pywfa_amd import WavefrontAligner, _native, datagen

from common import configs_pair

FULL = os.environ.get("WFA_TEST_FULL") == "1"


def families(seed, founders, copies, lo, hi, div=0.03, empty=2, alphabet="ACGT"):
    """Reads in families: random founders of lo..hi bases, copies with substitutions / insertions / deletions at `div`, shuffled,
    plus `empty` empty reads."""
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


def explicit(kw, patterns, texts):
    """The explicit path: all len(patterns) x len(texts) pairs through wavefront_align_batch, scope score."""
    kw = dict(kw, scope="score")
    al = WavefrontAligner(**kw)
    pp = [p for p in patterns for _ in texts]
    tt = [t for _ in patterns for t in texts]
    r = al.wavefront_align_batch(tt, pp)
    shape = (len(patterns), len(texts))
    return np.asarray(r["score"]).reshape(shape), np.asarray(r["status"]).reshape(shape)


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
def test_all_vs_all_matches_explicit(gpu, name, kw):
    reads = _reads_for(kw)
    al = WavefrontAligner(**kw)
    score, status = al.score_matrix(reads)
    es, et = explicit(kw, reads, reads)
    assert score.shape == (len(reads), len(reads)) and score.dtype == np.int32
    assert np.array_equal(status, et), name
    assert np.array_equal(score, es), name


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", GRID, ids=[g[0] for g in GRID])
def test_rectangle_matches_explicit(gpu, name, kw):
    reads = _reads_for(kw)
    pats, texts = reads[:37], reads[37:]
    al = WavefrontAligner(**kw)
    for p, t in ((pats, texts), (pats[:1], texts), (pats, texts[:1]), (pats[:1], texts[-1:])):
        score, status = al.score_matrix(p, t)
        es, et = explicit(kw, p, t)
        assert score.shape == (len(p), len(t))
        assert np.array_equal(status, et), name
        assert np.array_equal(score, es), name


@pytest.mark.gpu
def test_wildcard_reads(gpu):
    reads = families(5, 12, 4, 20, 200, alphabet="ACGTN", empty=1) + families(6, 4, 3, 20, 200)
    for kw in (dict(wildcard="N"), dict(wildcard="N", span="end-to-end", max_steps=60), dict(wildcard="A")):
        al = WavefrontAligner(**kw)
        score, status = al.score_matrix(reads)
        es, et = explicit(kw, reads, reads)
        assert np.array_equal(status, et) and np.array_equal(score, es), kw
        score, status = al.score_matrix(reads[:9], reads[9:])
        es, et = explicit(kw, reads[:9], reads[9:])
        assert np.array_equal(status, et) and np.array_equal(score, es), kw


ORACLE_KWS = [dict(scope="score", span="end-to-end"), dict(scope="score", distance="affine2p"), dict(scope="score", max_steps=30)]


@pytest.mark.gpu
def test_against_oracle(gpu):
    reads = families(21, 8, 6, 0, 200)[:48]
    for kw in ORACLE_KWS:
        oc, nc = configs_pair(**kw)
        al = WavefrontAligner(**kw)
        score, status = al.score_matrix(reads)
        batch = datagen.from_strings([p for p in reads for _ in reads], [t for _ in reads for t in reads], upper=True)
        o = loader.run(loader.oracle(), oc, batch)
        n = len(reads)
        assert np.array_equal(status, o["status"].reshape(n, n)), kw
        assert np.array_equal(score, o["score"].reshape(n, n)), kw


@pytest.mark.gpu
@pytest.mark.parametrize("band", [1, 37, 500])
def test_band_boundaries(gpu, band, monkeypatch):
    """Small bands (the knob is read when the aligner is created): ragged triangle bands, rows split over bands, the same cells."""
    kw = dict(span="end-to-end", max_steps=80)
    ref_s, ref_t = WavefrontAligner(**kw).score_matrix(READS)
    ref_r = WavefrontAligner(**kw).score_matrix(READS[:50], READS[50:])
    ref_c = WavefrontAligner(**kw).completed_pairs(READS)
    monkeypatch.setenv("WFA_HIP_CROSS_BAND", str(band))
    al = WavefrontAligner(**kw)
    s, t = al.score_matrix(READS)
    assert np.array_equal(s, ref_s) and np.array_equal(t, ref_t)
    s, t = al.score_matrix(READS[:50], READS[50:])
    assert np.array_equal(s, ref_r[0]) and np.array_equal(t, ref_r[1])
    c = al.completed_pairs(READS)
    for k in ("i", "j", "score"):
        assert np.array_equal(c[k], ref_c[k])
    # adaptive: both orders aligned, rectangular bands over the square
    kwa = dict(heuristic="adaptive", span="end-to-end")
    monkeypatch.delenv("WFA_HIP_CROSS_BAND")
    ref = WavefrontAligner(**kwa).score_matrix(READS)
    monkeypatch.setenv("WFA_HIP_CROSS_BAND", str(band))
    got = WavefrontAligner(**kwa).score_matrix(READS)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


@pytest.mark.gpu
def test_pilot_reuse_over_large_bands(gpu, monkeypatch):
    """Bands of >= 64 k pairs: the first one runs the pilots of the cascade, the second reuses their picks."""
    reads = families(31, 100 if not FULL else 200, 4, 140, 160, div=0.02, empty=0)
    kw = dict(span="end-to-end")
    monkeypatch.setenv("WFA_HIP_CROSS_BAND", "66000")
    s, t = WavefrontAligner(**kw).score_matrix(reads)
    es, et = explicit(kw, reads, reads)
    assert np.array_equal(t, et) and np.array_equal(s, es)


@pytest.mark.gpu
def test_long_reads(gpu):
    rng_reads = families(41, 2, 3, 2000, 4000 if not FULL else 12000, div=0.02, empty=0) + families(42, 6, 3, 100, 300, empty=1)
    for kw in (dict(span="end-to-end"), dict(span="end-to-end", max_steps=2000)):
        al = WavefrontAligner(**kw)
        s, t = al.score_matrix(rng_reads)
        es, et = explicit(kw, rng_reads, rng_reads)
        assert np.array_equal(t, et) and np.array_equal(s, es), kw
        s, t = al.score_matrix(rng_reads[:4], rng_reads[4:])
        es, et = explicit(kw, rng_reads[:4], rng_reads[4:])
        assert np.array_equal(t, et) and np.array_equal(s, es), kw


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(span="end-to-end", max_steps=40), dict(heuristic="adaptive", max_steps=40, span="end-to-end"),
                                dict(wildcard="N", max_steps=50)])
def test_completed_pairs(gpu, kw):
    reads = READS + families(7, 3, 3, 20, 100, alphabet="ACGTN", empty=0)
    al = WavefrontAligner(**kw)
    s, t = al.score_matrix(reads)
    c1 = al.completed_pairs(reads)
    c2 = al.completed_pairs(reads)
    ii, jj = np.nonzero((t == 0) & np.triu(np.ones_like(t, dtype=bool), 1))
    assert np.array_equal(c1["i"], ii) and np.array_equal(c1["j"], jj)
    assert np.array_equal(c1["score"], s[ii, jj])
    assert 0 < len(ii) < t.size
    for k in ("i", "j", "score"):
        assert c1[k].dtype == np.int32 and np.array_equal(c1[k], c2[k])
    p, q = reads[:40], reads[40:]
    s, t = al.score_matrix(p, q)
    c = al.completed_pairs(p, q)
    ii, jj = np.nonzero(t == 0)
    assert np.array_equal(c["i"], ii) and np.array_equal(c["j"], jj) and np.array_equal(c["score"], s[ii, jj])


@pytest.mark.gpu
def test_errors(gpu):
    al = WavefrontAligner(pattern_begin_free=10, text_end_free=10)
    with pytest.raises(ValueError, match="Ends-free parameters must be not larger than the sequences"):
        al.score_matrix(["ACGTACGTACGTACGT", "ACGT"])
    with pytest.raises(ValueError, match="Ends-free"):
        al.completed_pairs(["ACGTACGTACGTACGT"], ["ACGTACGTACGTACGT", "ACG"])
    # a set packed under one wildcard, run under another
    cfg = _native.default_config()
    cfg.scope = 0
    na = _native.Aligner(cfg)
    try:
        blob = np.frombuffer(b"ACGTNACGTT" + b"\0" * 64, np.uint8)
        s = na.seqset(blob, np.array([0, 5], np.int64), np.array([5, 5], np.int32))
        na.cross(s).close()
        # a refused run gives no handle back: its reason is in wfa_hip_global_error() too, whichever unit of the library raised it
        q = na.seqset(np.frombuffer(b"ACGTTGCAACGTTGCAACGT" * 4 + b"\0" * 64, np.uint8), np.arange(4, dtype=np.int64) * 20, np.full(4, 20, np.int32))
        assert not _native.lib().wfa_hip_cross_run_k(na._h, q._h, None, 0, 0)
        assert _native.lib().wfa_hip_global_error().decode().startswith("want: a combination of WFA_HIP_CROSS_DENSE")
        q.close()
        cfg.wildcard = ord("N")
        na.set_config(cfg)
        with pytest.raises(ValueError, match="wildcard"):
            na.cross(s)
        s.close()
    finally:
        na.close()
    with pytest.raises(UnicodeEncodeError):
        WavefrontAligner().score_matrix(["ACGT", "ACGÄ"])


@pytest.mark.gpu
def test_empty_sets(gpu):
    al = WavefrontAligner()
    s, t = al.score_matrix([])
    assert s.shape == (0, 0)
    s, t = al.score_matrix(["ACGT"], [])
    assert s.shape == (1, 0)
    c = al.completed_pairs([], ["ACGT"])
    assert all(len(c[k]) == 0 for k in ("i", "j", "score"))
