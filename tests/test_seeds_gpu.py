"""The seed finder on the GPU (wfa_hip_seed_index_*, WavefrontAligner.seed_index): the device result equals the host statement
wfa_hip_seeds_host for every read of seed_common.corpus(), array for array, overflow included.

The grid.  Every one of the 4 x 2 x 3 combinations of (k, stride, max_occ) is built, and queried under every one of the 2 x 2 x 2
combinations of (gap, pad, max_hits).  n: the host statement is evaluated once per combination with n = 16 and the device is queried
with n = 1, 4 and 16 — the first n columns of one ranking (test_seeds_abi.py holds the host statement to that): 576 queries in all.
The host statement scans the texts once per read, so a combination costs one pass over the corpus on the host's cores."""
import itertools

import numpy as np
import pytest

from pywfa_amd import WavefrontAligner, _native, datagen
from seed_common import KEYS, corpus, host_rows, locus_share, revcomp, same_rows

QUERY = list(itertools.product((0, 16), (0, 16), (64, 2048)))            # gap, pad, max_hits
INDEX = list(itertools.product((8, 11, 13, 15), (1, 4), (1, 8, 64)))     # k, stride, max_occ


def native_set(al, seqs):
    b = datagen.from_strings(b"", [s.decode() for s in seqs], upper=True)
    return al.seqset(b["seqs"], b["t_off"], b["t_len"])


@pytest.fixture(scope="module")
def sets(gpu):
    refs, reads, _ = corpus()
    al = _native.Aligner(_native.default_config(), 0)
    T, P = native_set(al, refs), native_set(al, reads)
    yield al, T, P
    P.close()
    T.close()
    al.close()


def check(idx, P, index_params, gap, pad, max_hits):
    refs, reads, _ = corpus()
    want = host_rows(reads, refs, n=16, gap=gap, pad=pad, max_hits=max_hits, **index_params)
    for n in (1, 4, 16):
        got = idx.query(P, n=n, gap=gap, pad=pad, max_hits=max_hits)
        same_rows(got, want, (index_params, n, gap, pad, max_hits), cols=n)
    return want


def test_corpus_covers_what_it_should():
    """No GPU: the conditions on the inputs, from the host statement under the default parameters."""
    refs, reads, origin = corpus()
    assert len(origin) == 2048 and [len(r) for r in refs] == [20011, 33333, 47777, 60000]
    assert sum(o[3] for o in origin) == 1024 and refs[2].count(b"N") > 500
    rows = host_rows(reads, refs)
    extra = slice(len(origin), None)
    assert rows["overflow"][extra].tolist() == [0] * 9 + [1, 0]            # the long read from the tandem block overflows
    assert (rows["j"][len(origin) + 4:len(origin) + 8] == -1).all()           # shorter than k
    assert rows["hits"][len(origin) + 8, 0] > 1000                            # a 1.5 kb read with one long cluster
    assert 1 <= rows["overflow"][:len(origin)].sum() <= 100                   # reads inside the repeats
    assert (rows["j"][:, 1] >= 0).sum() >= 10                                 # more than one cluster per read occurs
    assert locus_share(rows, origin) >= 0.95


@pytest.mark.gpu
@pytest.mark.parametrize("k,stride,max_occ", INDEX)
def test_every_index_and_query_equals_the_host_statement(sets, k, stride, max_occ):
    al, T, P = sets
    idx = al.seed_index(T, k, stride, max_occ)
    try:
        for gap, pad, max_hits in QUERY:
            check(idx, P, dict(k=k, stride=stride, max_occ=max_occ), gap, pad, max_hits)
        st = idx.stats()
        refs = corpus()[0]
        valid = sum(1 for r in refs for t in range(0, len(r) - k + 1, stride) if b"N" not in r[t:t + k])
        assert st["positions"] == valid and st["table_bytes"] >= 4 * 4 ** k + 8 * valid
        assert st["build_ms"] > 0 and st["query_ms"] > 0 and st["masked_kmers"] >= 1   # (the AC run)
    finally:
        idx.close()


@pytest.mark.gpu
def test_two_queries_a_closed_set_and_the_locus_share(gpu):
    refs, reads, origin = corpus()
    want = host_rows(reads, refs)
    al = _native.Aligner(_native.default_config(), 0)
    try:
        T, P = native_set(al, refs), native_set(al, reads)
        idx = al.seed_index(T)
        first = idx.query(P)
        same_rows(first, want, "first query")
        same_rows(idx.query(P, min_hits=1, n=2), host_rows(reads, refs, min_hits=1, n=2), "min_hits = 1")
        same_rows(idx.query(P), want, "second query")
        T.close()
        same_rows(idx.query(P), want, "the texts' set closed")
        P.close()
        P2 = native_set(al, reads[::-1])
        again = idx.query(P2)
        same_rows({key: again[key][::-1].copy() for key in KEYS + ("overflow",)}, want, "another pattern set, reversed order")
        empty = native_set(al, [])
        assert idx.query(empty)["j"].shape == (0, 4)
        for h in (idx, P2, empty):
            h.close()
        # the share of the simulated reads whose locus lies inside one of their windows: the host statement's, and at least 0.95
        share, host_share = locus_share(first, origin), locus_share(want, origin)
        print(f"locus share: device {share:.4f}, host statement {host_share:.4f}")
        assert share == host_share
        assert share >= 0.95
    finally:
        al.close()


@pytest.mark.gpu
def test_refusals_on_the_device(gpu):
    al = _native.Aligner(_native.default_config(), 0)
    other = _native.Aligner(_native.default_config(), 0)
    try:
        T = native_set(al, [b"ACGTACGTACGTACGTACGTAAAA"])
        for kw, name in ((dict(k=7), "k = 7"), (dict(k=16), "k = 16"), (dict(stride=0), "stride = 0"), (dict(max_occ=0), "max_occ = 0")):
            with pytest.raises(ValueError, match=name + " is out of range"):
                al.seed_index(T, **dict(dict(k=13, stride=1, max_occ=64), **kw))
        with pytest.raises(ValueError, match="another aligner"):
            other.seed_index(T)
        with pytest.raises(ValueError, match="0 sequences"):
            al.seed_index(native_set(al, []))
        idx = al.seed_index(T, 8)
        for kw, name in ((dict(n=0), "n = 0"), (dict(n=17), "n = 17"), (dict(min_hits=0), "min_hits = 0"), (dict(gap=-1), "gap = -1"),
                         (dict(pad=-2), "pad = -2"), (dict(max_hits=4097), "max_hits = 4097"), (dict(max_hits=0), "max_hits = 0")):
            with pytest.raises(ValueError, match=name + " is out of range"):
                idx.query(T, **kw)
        with pytest.raises(ValueError, match="another aligner"):
            idx.query(native_set(other, [b"ACGT"]))
        assert idx.query(T, min_hits=1)["j"][0, 0] == 0      # the index still works
        idx.close()
    finally:
        other.close()
        al.close()


@pytest.mark.gpu
def test_the_workflow_end_to_end(gpu):
    """sequence_set -> seed_index -> seeds -> align_windows(summary=True), and on a sample the scores of wavefront_align_batch on the
    materialised windows."""
    refs, reads, origin = corpus()
    reads_s, refs_s = [r.decode() for r in reads], [r.decode() for r in refs]
    a = WavefrontAligner(span="ends-free", text_begin_free=10, text_end_free=10)   # (no window is shorter than k)
    with a.sequence_set(reads_s) as R, a.sequence_set(refs_s) as G, a.seed_index(G) as idx:
        assert len(idx) == 4
        s = idx.seeds(R, n=4)
        same_rows(s, host_rows(reads, refs), "seeds()")
        same_rows(idx.seeds(reads_s[:300], n=4), {key: v[:300] for key, v in s.items()}, "a list of str")
        keep = s["j"] >= 0
        i = np.nonzero(keep)[0]
        j, ts, tl, rev = s["j"][keep], s["text_start"][keep], s["text_len"][keep], s["reverse"][keep].astype(np.uint8)
        hits = a.align_windows(R, G, i=i, j=j, text_start=ts, text_len=tl, reverse=rev, summary=True)
        assert len(hits["score"]) == len(i) > 1900 and hits["summary"]["locations"].shape == (len(i), 4)
        st = idx.stats()
        assert st["positions"] > 150000 and st["query_ms"] > 0
    sample = np.random.default_rng(3).choice(len(i), 96, replace=False)
    pats = [revcomp(reads[i[q]]).decode() if rev[q] else reads_s[i[q]] for q in sample]
    txts = [refs_s[j[q]][ts[q]:ts[q] + tl[q]] for q in sample]
    want = a.wavefront_align_batch(txts, pats)
    assert np.array_equal(hits["score"][sample], want["score"]) and np.array_equal(hits["status"][sample], want["status"])
    # a read's best window holds its alignment: 2 % of errors and the windows' padding, far from the score of unrelated sequences
    best = hits["score"][np.unique(i, return_index=True)[1]]
    assert np.median(best) > -100
