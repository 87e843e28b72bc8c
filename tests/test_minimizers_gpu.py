"""The minimizer index on the GPU (wfa_hip_seed_index_create_minimizer, WavefrontAligner.seed_index(w=...)): for every read of
minimizer_common.edge_set(k, w) the rows of seeds and chains equal the host statements wfa_hip_seeds_host_minimizer and
wfa_hip_chains_host_minimizer, all columns and overflow; w = 1 is the dense index; the indexed count is the sum of the host flags;
two builds agree; the index outlives its set; a stride index built after a minimizer index is what it is alone; the workflow end to
end; the Python surface.

Locus share (seed_common.corpus(nreads=300): 150-base reads at 2 %, against its four references; the host statement's figure, which
the device's equals because the rows do): at k = 13, w = 10, min_hits = 2 it is 0.9900, above the floor of 0.95 of the dense index's
test, so w = 10 is the window of the end-to-end test; a dense index (stride = 1) gives 0.9900 on the same reads, and (13, 5) and
(15, 10) give 0.9900 too."""
import functools

import numpy as np
import pytest

from pywfa_amd import WavefrontAligner, _native, datagen
import seed_common
from minimizer_common import CHAIN_KEYS, SEED_KEYS, edge_set, host_chain_rows, host_seed_rows, same

GRID = [(k, w) for k in (9, 13) for w in (1, 2, 5, 10, 32)] + [(15, 10)]
LOCUS_SHARE_13_10 = 0.9900   # the host statement's, k = 13, w = 10, min_hits = 2 on corpus(nreads=300)


def native_set(al, seqs):
    b = datagen.from_strings(b"", [s.decode() for s in seqs], upper=False)
    return al.seqset(b["seqs"], b["t_off"], b["t_len"])


@pytest.fixture(scope="module")
def al(gpu):
    a = _native.Aligner(_native.default_config(), 0)
    yield a
    a.close()


@functools.lru_cache(maxsize=None)
def host(kind, k, w, min_hits, max_occ=64):
    """The host statement's rows for edge_set(k, w), computed once."""
    texts, reads = edge_set(k, w)
    rows = host_seed_rows if kind == "seeds" else host_chain_rows
    return rows(reads, texts, k=k, w=w, min_hits=min_hits, max_occ=max_occ)


@pytest.mark.gpu
@pytest.mark.parametrize("k,w", GRID)
def test_seeds_and_chains_equal_the_host_statement_for_every_read(al, k, w):
    texts, reads = edge_set(k, w)
    T, P = native_set(al, texts), native_set(al, reads)
    idx = al.seed_index(T, k, 1, 64, w)
    try:
        assert idx.params() == dict(k=k, stride=1, w=w)
        for min_hits in (1, 2):
            same(idx.query(P, min_hits=min_hits), host("seeds", k, w, min_hits), SEED_KEYS, ("seeds", k, w, min_hits))
            same(idx.chain(P, min_hits=min_hits), host("chains", k, w, min_hits), CHAIN_KEYS, ("chains", k, w, min_hits))
        # the indexed count: the sum of the host flags over the texts; the records are allocated by it
        count = sum(int(_native.minimizers_host(t, k, w).sum()) for t in texts)
        st = idx.stats()
        assert st["positions"] == count and st["table_bytes"] == 4 * (4 ** k + 1) + 8 * count
        seeds = host("seeds", k, w, 1)
        assert (seeds["j"][:300, 0] >= 0).mean() > 0.9 and seeds["overflow"][-2] == 0     # the reads do find their texts
    finally:
        for h in (idx, P, T):
            h.close()


@pytest.mark.gpu
def test_the_all_ties_bucket_without_the_repeat_mask(al):
    """max_occ = 10^6: the homopolymer's bucket (every position ties, all are selected) yields its hits."""
    k, w = 13, 10
    texts, reads = edge_set(k, w)
    T, P = native_set(al, texts), native_set(al, reads)
    idx = al.seed_index(T, k, 1, 10 ** 6, w)
    try:
        want_s, want_c = host("seeds", k, w, 1, 10 ** 6), host("chains", k, w, 1, 10 ** 6)
        same(idx.query(P, min_hits=1), want_s, SEED_KEYS, "seeds, max_occ 10^6")
        same(idx.chain(P, min_hits=1), want_c, CHAIN_KEYS, "chains, max_occ 10^6")
        short, long_ = len(reads) - 3, len(reads) - 2         # A * (k + 3) and A * 150
        assert want_s["overflow"][short] == 0 and want_s["hits"][short, 0] == 4 * (300 - k + 1) and want_s["j"][short, 0] == len(texts) - 1
        assert want_s["overflow"][long_] == 1 and want_c["overflow"][long_] == 1
        assert idx.stats()["masked_kmers"] == 0
    finally:
        for h in (idx, P, T):
            h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [9, 13])
def test_w_1_is_the_dense_index(al, k):
    texts, reads = edge_set(k, 10)
    T, P = native_set(al, texts), native_set(al, reads)
    mini, dense = al.seed_index(T, k, 1, 64, 1), al.seed_index(T, k, 1, 64)
    try:
        assert mini.stats()["positions"] == dense.stats()["positions"]
        assert mini.params() == dict(k=k, stride=1, w=1) and dense.params() == dict(k=k, stride=1, w=0)
        same(mini.query(P), dense.query(P), SEED_KEYS, ("seeds", k))
        same(mini.chain(P), dense.chain(P), CHAIN_KEYS, ("chains", k))
    finally:
        for h in (mini, dense, P, T):
            h.close()


@pytest.mark.gpu
def test_two_builds_a_closed_set_and_a_stride_index_afterwards(al):
    k, w = 13, 10
    texts, reads = edge_set(k, w)
    T, P = native_set(al, texts), native_set(al, reads)
    alone = al.seed_index(T, k, 4, 64)
    stride_rows = alone.query(P), alone.chain(P)
    alone.close()
    one, two = al.seed_index(T, k, 1, 64, w), al.seed_index(T, k, 1, 64, w)
    try:
        same(one.query(P), two.query(P), SEED_KEYS, "two builds, seeds")
        same(one.chain(P), two.chain(P), CHAIN_KEYS, "two builds, chains")
        assert one.stats()["positions"] == two.stats()["positions"]
        T2 = native_set(al, texts)
        T.close()
        same(one.query(P, min_hits=1), host("seeds", k, w, 1), SEED_KEYS, "the texts' set closed")
        same(one.chain(P, min_hits=1), host("chains", k, w, 1), CHAIN_KEYS, "the texts' set closed")
        after = al.seed_index(T2, k, 4, 64)          # a stride index after minimizer indexes, in the same process
        assert after.params() == dict(k=k, stride=4, w=0)
        same(after.query(P), stride_rows[0], SEED_KEYS, "stride index, seeds")
        same(after.chain(P), stride_rows[1], CHAIN_KEYS, "stride index, chains")
        same(after.query(P), seed_common.host_rows(reads, texts, k=k, stride=4), SEED_KEYS, "stride index, host statement")
        same(one.query(P, min_hits=1), host("seeds", k, w, 1), SEED_KEYS, "the minimizer index beside it")
        after.close()
        T2.close()
    finally:
        for h in (one, two, P):
            h.close()


@pytest.mark.gpu
def test_the_workflow_end_to_end(gpu):
    """sequence_set -> seed_index(w=10) -> seeds -> align_windows(summary=True) on the 150-base reads of seed_common.corpus()."""
    k, w = 13, 10
    refs, reads, origin = seed_common.corpus(nreads=300)
    reads, reads_s, refs_s = reads[:300], [r.decode() for r in reads[:300]], [r.decode() for r in refs]
    want = host_seed_rows(reads, refs, k=k, w=w, min_hits=2)
    host_share = seed_common.locus_share(want, origin)
    a = WavefrontAligner(span="ends-free", text_begin_free=10, text_end_free=10)
    with a.sequence_set(reads_s) as R, a.sequence_set(refs_s) as G, a.seed_index(G, k=k, w=w) as idx:
        assert (idx.k, idx.w, idx.stride, len(idx)) == (k, w, 1, 4)
        s = idx.seeds(R, n=4, min_hits=2)
        same(s, want, SEED_KEYS, "seeds()")
        share = seed_common.locus_share(s, origin)
        print(f"locus share at k = {k}, w = {w}, min_hits = 2: device {share:.4f}, host statement {host_share:.4f}")
        assert share == host_share
        assert round(host_share, 4) == LOCUS_SHARE_13_10 and share >= 0.95
        # the windows that hold the true locus, into align_windows
        true = np.zeros(s["j"].shape, bool)
        for i, (j, pos, span, rev) in enumerate(origin):
            true[i] = (s["j"][i] == j) & (s["reverse"][i] == rev) & (s["text_start"][i] <= pos) & \
                      (s["text_start"][i] + s["text_len"][i] >= pos + span)
        i = np.nonzero(true)[0]
        hits = a.align_windows(R, G, i=i, j=s["j"][true], text_start=s["text_start"][true], text_len=s["text_len"][true],
                               reverse=s["reverse"][true].astype(np.uint8), summary=True)
        assert len(hits["score"]) == len(i) >= 0.95 * 300 and (hits["status"] == 0).all()
        assert hits["summary"]["locations"].shape == (len(i), 4) and np.median(hits["score"]) > -100
        c = idx.chains(R, min_hits=2, min_score=20)
        same(c, host_chain_rows(reads, refs, k=k, w=w, min_hits=2, min_score=20), CHAIN_KEYS, "chains()")
        st = idx.stats()
        assert set(st) == {"positions", "masked_kmers", "table_bytes", "build_ms", "query_ms", "chain_ms", "chain_workspace_bytes"}
        assert 0.15 * 160000 < st["positions"] < 0.22 * 160000
    a.close()


@pytest.mark.gpu
def test_the_python_surface(gpu):
    a = WavefrontAligner()
    text = seed_common.corpus()[0][0][:2000].decode()
    with pytest.raises(ValueError, match="w = 10 goes with stride = 1 only"):
        a.seed_index([text], w=10, stride=2)
    for w in (0, 33):
        with pytest.raises(ValueError, match=rf"\bw = {w} is out of range"):
            a.seed_index([text], w=w)
    with a.sequence_set([text]) as G:
        for w in (0, 33):     # the C entry's own refusal, nothing launched
            with pytest.raises(ValueError, match=rf"wfa_hip_seed_index_create_minimizer: seed index: w = {w} is out of range \(1 \.\. 32\)"):
                a._native.seed_index(G._set, 13, 1, 64, w)
    idx = a.seed_index([text], k=11, w=7)
    assert (idx.k, idx.w, idx.stride) == (11, 7, 1)
    assert idx.seeds([text[100:250]], min_hits=1)["j"][0, 0] == 0
    dense = a.seed_index([text], k=9, stride=3)
    assert (dense.k, dense.w, dense.stride) == (9, None, 3)
    dense.close()
    idx.close()
    for call in (lambda: idx.k, lambda: idx.w, lambda: idx.stride, lambda: idx.seeds([text]), lambda: idx.chains([text]), idx.stats):
        with pytest.raises(ValueError, match="seed index is closed"):
            call()
    a.close()
