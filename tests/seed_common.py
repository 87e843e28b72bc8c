"""Shared by the seed finder's tests (test_seeds_abi.py, test_seeds_gpu.py): the Python restatement of the rule of
include/wfa_hip.h ("seed finder") on k-mer STRINGS with a dict and sorted(), the host statement wfa_hip_seeds_host over many reads,
and the simulated corpus of the GPU tests."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from pywfa_amd import _native

ACGT = frozenset(b"ACGT")
COMP = bytes.maketrans(b"ACGT", b"TGCA")
KEYS = _native.SEED_KEYS
DEFAULTS = dict(k=13, stride=1, max_occ=64, n=4, min_hits=2, gap=16, pad=16, max_hits=2048)


def revcomp(b):
    return b.translate(COMP)[::-1]


def py_index(texts, k, stride):
    """k-mer string -> the list of its indexed positions (j, t)."""
    index = {}
    for j, t in enumerate(texts):
        for p in range(0, len(t) - k + 1, stride):
            kmer = t[p:p + k]
            if ACGT.issuperset(kmer):
                index.setdefault(kmer, []).append((j, p))
    return index


def py_seeds(read, texts, index, k=13, stride=1, max_occ=64, n=4, min_hits=2, gap=16, pad=16, max_hits=2048):
    """The row of one read by the definitions: dict of lists of n values and overflow.  `index` = py_index(texts, k, stride)."""
    L = len(read)
    row = dict(j=[-1] * n, reverse=[0] * n, text_start=[0] * n, text_len=[0] * n, hits=[0] * n, overflow=0)
    hits = []
    for s, strand in enumerate((read, revcomp(read))):
        for r in range(L - k + 1):
            where = index.get(strand[r:r + k], ())     # (a k-mer over a letter outside ACGT is in no bucket)
            if len(where) <= max_occ:
                hits += [(s, j, t - r) for j, t in where]
    if len(hits) > max_hits:
        row["overflow"] = 1
        return row
    hits = sorted(hits)
    clusters = []
    for h in hits:
        if clusters and clusters[-1][-1][:2] == h[:2] and h[2] - clusters[-1][-1][2] <= gap:
            clusters[-1].append(h)
        else:
            clusters.append([h])
    ranked = sorted((-len(c), c[0][0], c[0][1], c[0][2], c[-1][2]) for c in clusters if len(c) >= min_hits)
    for q, (negc, s, j, d_lo, d_hi) in enumerate(ranked[:n]):
        start, end = max(0, d_lo - pad), min(len(texts[j]), d_hi + L + pad)
        assert end > start
        row["j"][q], row["reverse"][q], row["text_start"][q], row["text_len"][q], row["hits"][q] = j, s, start, end - start, -negc
    return row


def host_rows(reads, texts, **params):
    """wfa_hip_seeds_host for every read: the arrays of a seed query (int32[M, n] and overflow uint8[M])."""
    p = dict(DEFAULTS, **params)
    blob = _native.seeds_host_texts(texts)
    m = len(reads)
    out = {key: np.zeros((m, p["n"]), np.int32) for key in KEYS}
    out["overflow"] = np.zeros(m, np.uint8)

    def work(lo):
        for i in range(lo, min(lo + 64, m)):
            row = _native.seeds_host(reads[i], blob, **p)
            for key in KEYS:
                out[key][i] = row[key]
            out["overflow"][i] = row["overflow"]

    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:   # (the C call releases the GIL)
        list(pool.map(work, range(0, m, 64)))
    return out


def same_rows(got, want, ctx, cols=None):
    """Array for array, overflow included; `cols`: compare against the first columns of `want` (the first n of one ranking)."""
    for key in KEYS + ("overflow",):
        w = want[key] if cols is None or key == "overflow" else want[key][:, :cols]
        g = got[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (ctx, key, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
        assert bad.size == 0, (ctx, key, int(bad[0]), g[bad[0]], w[bad[0]], bad.size)


# ---- the corpus of the GPU tests ------------------------------------------------------------------------------------------

LETTERS = np.frombuffer(b"ACGT", np.uint8)


def mutate(rng, f, div):
    """A copy of the base array `f` (values 0-3) with substitutions, deletions and insertions at `div` in all."""
    n = len(f)
    r = rng.random(n)
    sub = rng.integers(0, 4, n)
    out = np.where(r < div / 3, sub, f)
    counts = np.where((r >= div / 3) & (r < 2 * div / 3), 0, np.where((r >= 2 * div / 3) & (r < div), 2, 1))
    rep = np.repeat(np.arange(n), counts)
    res = out[rep]
    dup = np.r_[False, rep[1:] == rep[:-1]]
    res[dup] = sub[rep[dup]]
    return res


@functools.lru_cache(maxsize=None)
def corpus(seed=2024, nreads=2048):
    """Four references of 20-60 kb: the third with several N runs, the fourth with a block of 60 tandem copies of a 37-base unit and
    a 600-base run of the dinucleotide AC.  `nreads` reads of 150 bases cut from random positions of them (the repeats and the bases
    under the Ns included) and mutated at 2 %, every second one stored reverse-complemented; behind them reads that come from nowhere:
    random sequence, shorter than any k (one of them empty), and 1-2 kb (two cut from a reference, one of them from the tandem block,
    one random).  Returns (references, reads, origin): bytes, and for the simulated reads (j, position, span on the reference,
    stored reverse-complemented)."""
    rng = np.random.default_rng(seed)
    bases = [rng.integers(0, 4, n) for n in (20011, 33333, 47777, 60000)]
    unit = rng.integers(0, 4, 37)
    bases[3][30000:30000 + 37 * 60] = np.tile(unit, 60)
    bases[3][45000:45600] = np.tile(np.array([0, 1]), 300)
    refs = [bytearray(LETTERS[b].tobytes()) for b in bases]
    for a, b in [(0, 9), (5000, 5001), (12000, 12016), (20000, 20400), (33010, 33024), (47700, 47777)]:
        refs[2][a:b] = b"N" * (b - a)
    refs = [bytes(r) for r in refs]
    reads, origin = [], []
    for q in range(nreads):
        j = int(rng.integers(0, 4))
        pos = int(rng.integers(0, len(bases[j]) - 150 + 1))
        s = LETTERS[mutate(rng, bases[j][pos:pos + 150], 0.02)].tobytes()
        rev = q % 2 == 1
        reads.append(revcomp(s) if rev else s)
        origin.append((j, pos, 150, int(rev)))
    rand = lambda n: LETTERS[rng.integers(0, 4, n)].tobytes()   # noqa: E731
    reads += [rand(150) for _ in range(4)]
    reads += [b"", rand(5), rand(7), rand(7)]
    reads += [LETTERS[mutate(rng, bases[1][7000:8500], 0.02)].tobytes(), revcomp(LETTERS[mutate(rng, bases[3][29500:31200], 0.02)].tobytes()),
              rand(1200)]
    return refs, reads, origin


def locus_share(rows, origin):
    """The share of the simulated reads whose true locus lies inside one of their windows, on the right text and strand."""
    found = 0
    for i, (j, pos, span, rev) in enumerate(origin):
        ok = (rows["j"][i] == j) & (rows["reverse"][i] == rev) & (rows["text_start"][i] <= pos) & \
             (rows["text_start"][i] + rows["text_len"][i] >= pos + span)
        found += bool(ok.any())
    return found / len(origin)
