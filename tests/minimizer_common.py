"""Shared by the minimizer tests (test_minimizers_abi.py, test_minimizers_gpu.py): the Python restatement of the rule of
include/wfa_hip.h ("minimizers") as a plain loop over strings, the seed and chain rules of seed_common.py / chain_common.py restated
over a minimizer-filtered index and minimizer-filtered read positions, the host statements over many reads, and the text set and the
reads of the GPU tests."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from pywfa_amd import _native
from chain_common import KEYS as CHAIN_KEYS, cost
from seed_common import ACGT, KEYS as SEED_KEYS, LETTERS, mutate, revcomp

INF = float("inf")
CHAIN_DEFAULTS = dict(k=13, max_occ=64, n=4, min_hits=3, min_score=40, lookback=32, max_dist=5000, band=500, pad=64, max_anchors=16384)
SEED_DEFAULTS = dict(k=13, max_occ=64, n=4, min_hits=2, gap=16, pad=16, max_hits=2048)


def mix32(h):
    h ^= h >> 16
    h = (h * 0x85ebca6b) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def code(kmer):
    """The 2-bit code of a k-mer of ACGT: letter i in bits 2 i .. 2 i + 1, A 0, C 1, T 2, G 3 ((c >> 1) & 3)."""
    return sum(((c >> 1) & 3) << (2 * i) for i, c in enumerate(kmer))


def py_keys(seq, k):
    """key(p) for p in 0 .. len(seq) - 1 (+inf where the k-mer runs over the end or over a letter outside ACGT)."""
    keys = []
    for p in range(len(seq)):
        kmer = seq[p:p + k]
        if len(kmer) < k or not ACGT.issuperset(kmer):
            keys.append(INF)
        else:
            keys.append(mix32(min(code(kmer), code(revcomp(kmer)))))
    return keys


def py_minimizers(seq, k, w):
    """The flags of the rule, position by position: l and r as worded, each capped at w - 1; selected iff l + r + 1 >= w."""
    keys = py_keys(seq, k)
    key = lambda p: keys[p] if 0 <= p < len(keys) else INF   # noqa: E731
    flags = []
    for p in range(len(seq)):
        if keys[p] == INF:
            flags.append(False)
            continue
        l = 0
        while l < w - 1 and key(p - 1 - l) >= keys[p]:
            l += 1
        r = 0
        while r < w - 1 and key(p + 1 + r) >= keys[p]:
            r += 1
        flags.append(l + r + 1 >= w)
    return flags


def py_min_index(texts, k, w):
    """k-mer string -> the list of its indexed positions (j, t): the minimizers of every text."""
    index = {}
    for j, t in enumerate(texts):
        for p, sel in enumerate(py_minimizers(t, k, w)):
            if sel:
                index.setdefault(t[p:p + k], []).append((j, p))
    return index


def py_min_anchors(read, index, k, w, max_occ):
    """(s, r, j, t) for the read positions r of R_s that are minimizers of R_s, sorted."""
    anchors = []
    for s, strand in enumerate((read, revcomp(read))):
        for r, sel in enumerate(py_minimizers(strand, k, w)):
            if sel:
                where = index.get(strand[r:r + k], ())
                if len(where) <= max_occ:
                    anchors += [(s, r, j, t) for j, t in where]
    return sorted(anchors)


def py_min_seeds(read, texts, index, k=13, w=10, max_occ=64, n=4, min_hits=2, gap=16, pad=16, max_hits=2048):
    """seed_common.py_seeds with the hits taken from the read's minimizers only."""
    L = len(read)
    row = dict(j=[-1] * n, reverse=[0] * n, text_start=[0] * n, text_len=[0] * n, hits=[0] * n, overflow=0)
    hits = sorted((s, j, t - r) for s, r, j, t in py_min_anchors(read, index, k, w, max_occ))
    if len(hits) > max_hits:
        row["overflow"] = 1
        return row
    clusters = []
    for h in hits:
        if clusters and clusters[-1][-1][:2] == h[:2] and h[2] - clusters[-1][-1][2] <= gap:
            clusters[-1].append(h)
        else:
            clusters.append([h])
    ranked = sorted((-len(c), c[0][0], c[0][1], c[0][2], c[-1][2]) for c in clusters if len(c) >= min_hits)
    for q, (negc, s, j, d_lo, d_hi) in enumerate(ranked[:n]):
        start, end = max(0, d_lo - pad), min(len(texts[j]), d_hi + L + pad)
        row["j"][q], row["reverse"][q], row["text_start"][q], row["text_len"][q], row["hits"][q] = j, s, start, end - start, -negc
    return row


def py_min_chains(read, texts, index, k=13, w=10, max_occ=64, n=4, min_hits=3, min_score=40, lookback=32, max_dist=5000, band=500, pad=64,
                  max_anchors=16384):
    """chain_common.py_chains with the anchors taken from the read's minimizers only."""
    L = len(read)
    row = {key: [0] * n for key in CHAIN_KEYS}
    row["j"], row["overflow"] = [-1] * n, 0
    anchors = py_min_anchors(read, index, k, w, max_occ)
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
        value, b = max(candidates) if candidates else (0, None)
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
        row["j"][q], row["reverse"][q], row["text_start"][q], row["text_len"][q] = j, s, start, end - start
        row["hits"][q], row["score"][q] = cnt[a], f[a]
        row["pattern_start"][q], row["pattern_len"][q] = (L - (r + k) if s else r_first[a]), r + k - r_first[a]
        for c, (sc, rc, jc, tc) in enumerate(anchors):
            if (sc, jc) == (s, j) and start <= tc and tc + k <= end:
                covered[c] = True
    return row


def _host_rows(call, keys, reads, texts, params, chunk):
    blob = texts if isinstance(texts, dict) else _native.seeds_host_texts(texts)
    m = len(reads)
    out = {key: np.zeros((m, params["n"]), np.int32) for key in keys}
    out["overflow"] = np.zeros(m, np.uint8)

    def work(lo):
        for i in range(lo, min(lo + chunk, m)):
            row = call(reads[i], blob, **params)
            for key in keys:
                out[key][i] = row[key]
            out["overflow"][i] = row["overflow"]

    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:   # (the C call releases the GIL)
        list(pool.map(work, range(0, m, chunk)))
    return out


def host_seed_rows(reads, texts, **params):
    """wfa_hip_seeds_host_minimizer (w given) or wfa_hip_seeds_host for every read: the arrays of a seed query."""
    return _host_rows(_native.seeds_host, SEED_KEYS, reads, texts, dict(SEED_DEFAULTS, **params), 16)


def host_chain_rows(reads, texts, **params):
    """wfa_hip_chains_host_minimizer (w given) or wfa_hip_chains_host for every read: the arrays of a chain query."""
    return _host_rows(_native.chains_host, CHAIN_KEYS, reads, texts, dict(CHAIN_DEFAULTS, **params), 4)


def same(got, want, keys, ctx):
    """Array for array, overflow included."""
    for key in keys + ("overflow",):
        g, w = got[key], want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (ctx, key, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
        assert bad.size == 0, (ctx, key, int(bad[0]), g[bad[0]], w[bad[0]], bad.size)


# ---- the text set and the reads of the GPU tests ----------------------------------------------------------------------------

def rand(rng, n):
    return LETTERS[rng.integers(0, 4, n)].tobytes()


@functools.lru_cache(maxsize=None)
def edge_set(k, w, seed=31):
    """(texts, reads) for one (k, w), every sequence there to hit one edge.
    Texts: 0: 40 000 random bases; 1 - 3: 4096 + k - 1 bases (4096 k-mer starts: one tile of 256 words, if the build is tiled) and that
    - w and + w; 4 - 43: forty texts of 17 - 60 bases in a row (many sequences inside one tile); 44 - 47: texts of 5 - 12 bases (shorter
    than k = 13; two shorter than 9); 48: 3000 bases with N runs (one longer than w + k, one at position 0, one at the end, single
    Ns); 49: a 300-base homopolymer.
    Reads: 300 of 150 bases cut from text 0 (and every tenth from texts 1 - 3 and 48) at 2 - 3 % divergence, every second one stored
    reverse-complemented; 20 of 1 - 3 kb from text 0 at 8 % with indels; reads of length k - 1, k, k + 1 and k + w - 2 (cut from text
    0, unmutated); a read with an N in the middle; a read lying across the end of text 0; a short read (k + 3) and a 150-base read
    from the homopolymer; one random read."""
    rng = np.random.default_rng(seed + 100 * k + w)
    base0 = rng.integers(0, 4, 40000)
    texts = [LETTERS[base0].tobytes()]
    texts += [rand(rng, 4096 + k - 1 + d) for d in (0, -w, w)]
    texts += [rand(rng, int(n)) for n in rng.integers(17, 61, 40)]
    texts += [rand(rng, n) for n in (5, 8, 10, 12)]
    t = bytearray(rand(rng, 3000))
    for a, b in [(0, 3), (500, 501), (900, 900 + w + k + 5), (1500, 1502), (2990, 3000)]:
        t[a:b] = b"N" * (b - a)
    texts.append(bytes(t))
    texts.append(b"A" * 300)
    code = np.zeros(256, np.int64)
    for c, v in zip(b"ACGT", range(4)):
        code[c] = v
    bases = {j: code[np.frombuffer(texts[j], np.uint8)] for j in (0, 1, 2, 3, 48)}
    reads = []
    for q in range(300):
        j = (1, 2, 3, 48)[(q // 10) % 4] if q % 10 == 9 else 0
        pos = int(rng.integers(0, len(bases[j]) - 150 + 1))
        s = LETTERS[mutate(rng, bases[j][pos:pos + 150], (0.02, 0.03)[q % 2])].tobytes()
        reads.append(revcomp(s) if (q // 2) % 2 else s)
    for q in range(20):
        span = int(rng.integers(1000, 3001))
        pos = int(rng.integers(0, 40000 - span + 1))
        s = LETTERS[mutate(rng, base0[pos:pos + span], 0.08)].tobytes()
        reads.append(revcomp(s) if q % 2 else s)
    reads += [texts[0][7000:7000 + n] for n in (k - 1, k, k + 1, k + w - 2)]
    mid = bytearray(texts[0][9000:9150])
    mid[75] = ord("N")
    reads.append(bytes(mid))
    reads.append(texts[0][-100:] + rand(rng, 50))
    reads += [b"A" * (k + 3), b"A" * 150, rand(rng, 150)]
    return texts, reads
