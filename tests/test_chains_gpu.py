"""Chaining on the GPU (wfa_hip_seed_index_chain, SeedIndex.chains): the device result equals the host statement wfa_hip_chains_host
for every read of chain_common.long_corpus() plus the first 256 short reads of seed_common.corpus(), array for array, overflow
included.

The grid.  Every combination of (k, stride, max_occ) x lookback x (max_dist, band) x (min_hits, min_score) is one case; inside it
max_anchors takes the exact N of the corpus's first 6 kb read, N - 1 (that read and every read with as many anchors overflow) and
65 536.  n: the host statement is evaluated once with n = 16 and the device is queried with n = 1, 4 and 16 — the first n rounds of
one selection.  At max_occ = 64 the tandem block gives buckets of up to 60 records, where the order inside a bucket decides the rows."""
import itertools

import numpy as np
import pytest

from pywfa_amd import WavefrontAligner, _native, datagen
from chain_common import anchor_count, host_chain_rows, long_corpus, same_rows
from seed_common import corpus, locus_share, revcomp

INDEX = list(itertools.product((8, 11, 13), (1, 4), (4, 64)))            # k, stride, max_occ
QUERY = list(itertools.product((1, 32, 64), ((5000, 500), (200, 10)), ((3, 40), (1, 0))))   # lookback, (max_dist, band), (min_hits, min_score)


def all_reads():
    return long_corpus()[1] + corpus()[1][:256]


def native_set(al, seqs):
    b = datagen.from_strings(b"", [s.decode() for s in seqs], upper=True)
    return al.seqset(b["seqs"], b["t_off"], b["t_len"])


@pytest.fixture(scope="module")
def sets(gpu):
    al = _native.Aligner(_native.default_config(), 0)
    T, P = native_set(al, long_corpus()[0]), native_set(al, all_reads())
    yield al, T, P, _native.seeds_host_texts(long_corpus()[0])
    P.close()
    T.close()
    al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lookback,dist_band,hits_score", QUERY)
@pytest.mark.parametrize("k,stride,max_occ", INDEX)
def test_every_index_and_query_equals_the_host_statement(sets, k, stride, max_occ, lookback, dist_band, hits_score):
    al, T, P, blob = sets
    refs, reads = long_corpus()[0], all_reads()
    N = anchor_count(reads[0], refs, k, stride, max_occ)
    assert 2 <= N <= 65536
    q = dict(lookback=lookback, max_dist=dist_band[0], band=dist_band[1], min_hits=hits_score[0], min_score=hits_score[1])
    idx = al.seed_index(T, k, stride, max_occ)
    try:
        for max_anchors in (N, N - 1, 65536):
            want = host_chain_rows(reads, blob, k=k, stride=stride, max_occ=max_occ, n=16, max_anchors=max_anchors, **q)
            assert want["overflow"][0] == (max_anchors == N - 1)
            for n in (1, 4, 16):
                got = idx.chain(P, n=n, max_anchors=max_anchors, **q)
                same_rows(got, want, (k, stride, max_occ, q, max_anchors, n), cols=n)
        st = idx.chain_stats()
        assert st["kernel_ms"] > 0 and st["workspace_bytes"] >= 32 * 65536
    finally:
        idx.close()


@pytest.mark.gpu
def test_two_indexes_a_closed_set_and_the_locus_share(gpu):
    refs, reads, origin = long_corpus()
    want = host_chain_rows(reads, refs, k=11, stride=4)
    al = _native.Aligner(_native.default_config(), 0)
    try:
        T, P = native_set(al, refs), native_set(al, reads)
        one, two = al.seed_index(T, 11, 4, 64), al.seed_index(T, 11, 4, 64)
        first = one.chain(P)
        same_rows(first, want, "the first index")
        same_rows(two.chain(P), first, "a second index of the same set")
        same_rows(one.chain(P), first, "a second query")
        T.close()
        same_rows(one.chain(P), want, "the texts' set closed")
        empty = native_set(al, [])
        assert one.chain(empty)["pattern_len"].shape == (0, 4)
        for h in (one, two, P, empty):
            h.close()
        # the share of the simulated reads whose locus lies inside one of their windows: exactly the host statement's
        share, host_share = locus_share(first, origin), locus_share(want, origin)
        print(f"locus share: device {share:.4f}, host statement {host_share:.4f}")
        assert share == host_share
        assert share >= 0.95
    finally:
        al.close()


@pytest.mark.gpu
def test_six_kb_reads_overflow_the_seed_finder_and_chain(gpu):
    refs, reads, origin = long_corpus()
    six = [i for i, o in enumerate(origin) if o[2] == 6000]
    assert len(six) >= 8
    a = WavefrontAligner()
    with a.sequence_set([reads[i].decode() for i in six]) as R, a.seed_index([r.decode() for r in refs], k=9, stride=1) as idx:
        seeds = idx.seeds(R, max_hits=4096)
        chains = idx.chains(R)
    assert (seeds["overflow"] == 1).all() and (seeds["j"] == -1).all()
    assert (chains["overflow"] == 0).all()
    assert locus_share(chains, [origin[i] for i in six]) == 1.0


@pytest.mark.gpu
def test_refusals_on_the_device(gpu):
    al = _native.Aligner(_native.default_config(), 0)
    other = _native.Aligner(_native.default_config(), 0)
    try:
        T = native_set(al, [b"ACGTACGTACGTACGTACGTAAAA"])
        idx = al.seed_index(T, 8)
        for kw, name in ((dict(n=0), "n = 0"), (dict(n=17), "n = 17"), (dict(min_hits=0), "min_hits = 0"), (dict(min_score=-1), "min_score = -1"),
                         (dict(lookback=0), "lookback = 0"), (dict(lookback=65), "lookback = 65"), (dict(max_dist=0), "max_dist = 0"),
                         (dict(max_dist=1048577), "max_dist = 1048577"), (dict(band=-1), "band = -1"), (dict(band=65537), "band = 65537"),
                         (dict(pad=-2), "pad = -2"), (dict(max_anchors=0), "max_anchors = 0"), (dict(max_anchors=65537), "max_anchors = 65537")):
            with pytest.raises(ValueError, match=name + " is out of range"):
                idx.chain(T, **kw)
        with pytest.raises(ValueError, match="another aligner"):
            idx.chain(native_set(other, [b"ACGT"]))
        assert idx.chain_stats() == dict(kernel_ms=0.0, workspace_bytes=0)      # nothing was launched, nothing allocated
        row = idx.chain(T, min_hits=1, min_score=0, max_anchors=256)
        assert row["j"][0, 0] == 0 and row["overflow"][0] == 0                     # the index still works
        st = idx.chain_stats()
        assert st["kernel_ms"] > 0 and st["workspace_bytes"] == 32 * 256
        idx.close()
    finally:
        other.close()
        al.close()


@pytest.mark.gpu
def test_the_workflow_end_to_end(gpu):
    """sequence_set -> seed_index -> chains -> align_windows(summary=True), with the whole read and with the chain's part of it; the
    scores and statuses of wavefront_align_batch on the materialised strings, for every window."""
    refs, reads, origin = long_corpus()
    reads_s, refs_s = [r.decode() for r in reads], [r.decode() for r in refs]
    a = WavefrontAligner(span="ends-free", text_begin_free=100, text_end_free=100, heuristic="adaptive")   # (WFA's wf-adaptive)
    with a.sequence_set(reads_s) as R, a.sequence_set(refs_s) as G, a.seed_index(G, k=11, stride=4) as idx:
        c = idx.chains(R)
        same_rows(c, host_chain_rows(reads, refs, k=11, stride=4), "chains()")
        same_rows(idx.chains(reads_s[:20]), {key: v[:20] for key, v in c.items()}, "a list of str")
        st = idx.stats()
        assert st["chain_ms"] > 0 and st["chain_workspace_bytes"] >= 32 * 16384
        keep = c["j"] >= 0
        i = np.nonzero(keep)[0]
        j, ts, tl, rev = c["j"][keep], c["text_start"][keep], c["text_len"][keep], c["reverse"][keep].astype(np.uint8)
        ps, pl = c["pattern_start"][keep], c["pattern_len"][keep]
        assert keep[:len(origin), 0].all()
        whole = a.align_windows(R, G, i=i, j=j, text_start=ts, text_len=tl, reverse=rev, summary=True)
        part = a.align_windows(R, G, i=i, j=j, pattern_start=ps, pattern_len=pl, text_start=ts, text_len=tl, reverse=rev, summary=True)
        assert whole["summary"]["locations"].shape == (len(i), 4) == part["summary"]["locations"].shape
    txts = [refs_s[j[q]][ts[q]:ts[q] + tl[q]] for q in range(len(i))]
    for got, pats in ((whole, [reads[i[q]] for q in range(len(i))]), (part, [reads[i[q]][ps[q]:ps[q] + pl[q]] for q in range(len(i))])):
        pats = [(revcomp(p) if rev[q] else p).decode() for q, p in enumerate(pats)]
        want = a.wavefront_align_batch(txts, pats)
        assert np.array_equal(got["score"], want["score"]) and np.array_equal(got["status"], want["status"])
    # a read's best window holds its alignment: 8 % of errors, far from the score of unrelated sequences
    best = whole["score"][np.unique(i, return_index=True)[1]][:len(origin)]
    spans = np.array([o[2] for o in origin])
    assert (best > -spans).mean() > 0.9
