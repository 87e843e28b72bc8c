"""Shared by the chaining tests (test_chains_abi.py, test_chains_gpu.py): the Python restatement of the rule of include/wfa_hip.h
("chains") on k-mer STRINGS with a dict, sorted() and a plain double loop, the host statement wfa_hip_chains_host over many reads,
and the long-read corpus."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from pywfa_amd import _native
from seed_common import LETTERS, corpus, mutate, py_index, revcomp

KEYS = _native.CHAIN_KEYS
DEFAULTS = dict(k=13, stride=1, max_occ=64, n=4, min_hits=3, min_score=40, lookback=32, max_dist=5000, band=500, pad=64, max_anchors=16384)


def cost(g, k):
    return 0 if g == 0 else ((g * k) >> 6) + ((g.bit_length() - 1) >> 1)


def py_anchors(read, index, k, max_occ):
    """The read's anchors (s, r, j, t) in the order of the rule.  `index` = py_index(texts, k, stride)."""
    anchors = []
    for s, strand in enumerate((read, revcomp(read))):
        for r in range(len(read) - k + 1):
            where = index.get(strand[r:r + k], ())     # (a k-mer over a letter outside ACGT is in no bucket)
            if len(where) <= max_occ:
                anchors += [(s, r, j, t) for j, t in where]
    return sorted(anchors)


def py_chains(read, texts, index, k=13, stride=1, max_occ=64, n=4, min_hits=3, min_score=40, lookback=32, max_dist=5000, band=500, pad=64,
              max_anchors=16384):
    """The row of one read by the definitions: dict of lists of n values and overflow."""
    L = len(read)
    row = {key: [0] * n for key in KEYS}
    row["j"], row["overflow"] = [-1] * n, 0
    anchors = py_anchors(read, index, k, max_occ)
    if len(anchors) > max_anchors:
        row["overflow"] = 1
        return row
    f, cnt, d_lo, d_hi, r_first = [], [], [], [], []
    for a, (s, r, j, t) in enumerate(anchors):
        d = t - r
        candidates = []
        for b in range(max(0, a - lookback), a):
            sb, rb, jb, tb = anchors[b]
            dr, dt = r - rb, t - tb
            if (sb, jb) == (s, j) and 0 < dr <= max_dist and 0 < dt <= max_dist and abs(dt - dr) <= band:
                candidates.append((f[b] + min(dr, dt, k) - cost(abs(dt - dr), k), b))
        value, b = max(candidates) if candidates else (0, None)     # the largest value, then the largest index
        if value > k:
            f.append(value), cnt.append(cnt[b] + 1), d_lo.append(min(d_lo[b], d)), d_hi.append(max(d_hi[b], d)), r_first.append(r_first[b])
        else:
            f.append(k), cnt.append(1), d_lo.append(d), d_hi.append(d), r_first.append(r)
    covered = [False] * len(anchors)
    for q in range(n):
        ranked = [(-f[a], a) for a in range(len(anchors)) if not covered[a] and cnt[a] >= min_hits and f[a] >= min_score]
        if not ranked:
            break
        a = min(ranked)[1]
        s, r, j, t = anchors[a]
        start, end = max(0, d_lo[a] - pad), min(len(texts[j]), d_hi[a] + L + pad)
        assert start <= t and t + k <= end
        row["j"][q], row["reverse"][q], row["text_start"][q], row["text_len"][q] = j, s, start, end - start
        row["hits"][q], row["score"][q] = cnt[a], f[a]
        row["pattern_start"][q], row["pattern_len"][q] = (L - (r + k) if s else r_first[a]), r + k - r_first[a]
        for c, (sc, rc, jc, tc) in enumerate(anchors):
            if (sc, jc) == (s, j) and start <= tc and tc + k <= end:
                covered[c] = True
    return row


def host_chain_rows(reads, texts, **params):
    """wfa_hip_chains_host for every read: the arrays of a chain query (int32[M, n] and overflow uint8[M])."""
    p = dict(DEFAULTS, **params)
    blob = texts if isinstance(texts, dict) else _native.seeds_host_texts(texts)
    m = len(reads)
    out = {key: np.zeros((m, p["n"]), np.int32) for key in KEYS}
    out["overflow"] = np.zeros(m, np.uint8)

    def work(lo):
        for i in range(lo, min(lo + 2, m)):
            row = _native.chains_host(reads[i], blob, **p)
            for key in KEYS:
                out[key][i] = row[key]
            out["overflow"][i] = row["overflow"]

    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:   # (the C call releases the GIL)
        list(pool.map(work, range(0, m, 2)))
    return out


def same_rows(got, want, ctx, cols=None):
    """Array for array, overflow included; `cols`: compare against the first columns of `want` (the first n rounds of one selection)."""
    for key in KEYS + ("overflow",):
        w = want[key] if cols is None or key == "overflow" else want[key][:, :cols]
        g = got[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (ctx, key, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
        assert bad.size == 0, (ctx, key, int(bad[0]), g[bad[0]], w[bad[0]], bad.size)


def anchor_count(read, texts, k, stride, max_occ):
    """N of the rule for one read, from the dict."""
    return len(py_anchors(read, py_index_cached(tuple(texts), k, stride), k, max_occ))


@functools.lru_cache(maxsize=8)
def py_index_cached(texts, k, stride):
    return py_index(texts, k, stride)


# ---- the long-read corpus ----------------------------------------------------------------------------------------------------

SPANS = (6000, 1000, 3000, 2000, 4500)     # the spans on the reference of the reads, in turn
CODE = np.zeros(256, np.int64)
for _c, _v in zip(b"ACGT", range(4)):
    CODE[_c] = _v


@functools.lru_cache(maxsize=None)
def long_corpus(seed=77):
    """The four references of seed_common.corpus() (20-60 kb; N runs in the third; a 60-copy tandem block and an AC run in the fourth).
    48 reads whose spans on the reference run through SPANS (1-6 kb), mutated at 8 % (substitutions, deletions, insertions), every second
    one stored reverse-complemented.  Read q comes from reference q % 4 at a random position, except that the 6 kb reads come from the
    first three references only (the fourth holds the repeats, where a long read has more anchors than any index keeps) and that three
    reads of at most 3 kb are placed by hand: over the tandem block with both flanks, over the AC run, and over the long N run (the bases
    under the Ns count as A).  Behind them: three random reads of 2 kb, an empty read, reads of 5 and 7 bases, and one read joined from
    two distant loci (1.5 kb of reference 0 and 1.5 kb of reference 1, unmutated).
    Returns (references, reads, origin): bytes, and for the 48 simulated reads (j, position, span on the reference, stored
    reverse-complemented)."""
    refs = corpus()[0]
    bases = [CODE[np.frombuffer(r, np.uint8)] for r in refs]
    rng = np.random.default_rng(seed)
    placed = {9: (3, 29600, 3000), 15: (3, 44500, 2000), 21: (2, 19500, 1500)}
    reads, origin = [], []
    for q in range(48):
        span = SPANS[q % len(SPANS)]
        j = q % 3 if span == 6000 else q % 4
        pos = int(rng.integers(0, len(bases[j]) - span + 1))
        if q in placed:
            j, pos, span = placed[q]
        s = LETTERS[mutate(rng, bases[j][pos:pos + span], 0.08)].tobytes()
        rev = q % 2 == 1
        reads.append(revcomp(s) if rev else s)
        origin.append((j, pos, span, int(rev)))
    rand = lambda n: LETTERS[rng.integers(0, 4, n)].tobytes()   # noqa: E731
    reads += [rand(2000) for _ in range(3)]
    reads += [b"", rand(5), rand(7)]
    reads.append(refs[0][2000:3500] + refs[1][25000:26500])
    return refs, reads, origin
