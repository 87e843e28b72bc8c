"""Probe of the seed finder (WavefrontAligner.seed_index, wfa_hip_seed_index_*).

Workload: that of windows_index.py — 8 references of 1 Mb (fixed seed), 16 384 reads of 150 bp cut from random positions of them at
2 %, every second one stored reverse-complemented.  Default parameters (k = 13, stride 1, max_occ 64; n = 4, min_hits 2, gap 16,
pad 16, max_hits 2048); gap-affine, ends-free with 10 free text bases on either side, scope full.
(1) The index build and the query kernel by HIP events (SeedIndex.stats()), medians of REPS builds / queries.
(2) seeds() from Python on open handles (both sets resident), medians of REPS.
(3) The share of reads whose true locus lies inside one of their windows, on the right reference and strand.
(4) align_windows(summary=True) on the returned windows, from Python on open handles, and the query's share of that time.
Usage: seed_index.py [--reps N]"""
import hashlib
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pywfa_amd import WavefrontAligner  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
LUT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
READ, NREF, REFLEN = 150, 8, 1 << 20


def copy_of(rng, f, div=0.02):
    """A copy of f (codes 0..3) with substitutions, deletions and insertions in equal parts at `div`, cut or padded to READ bases."""
    L = len(f)
    r = rng.random(L)
    sub = rng.integers(0, 4, L)
    first = np.where(r < div / 3, sub, f)
    cnt = np.where((r >= div / 3) & (r < 2 * div / 3), 0, np.where((r >= 2 * div / 3) & (r < div), 2, 1))
    vals = np.stack([first, sub], 1).ravel()
    keep = np.stack([cnt >= 1, cnt == 2], 1).ravel()
    out = vals[keep][:READ]
    return LUT[np.r_[out, sub[:READ - len(out)]]].tobytes()


def source_hash():
    h = hashlib.sha256()
    for name in ("k_seed.hip", "k_seed.hpp", "wfa_seed.hpp"):
        h.update(open(os.path.join(ROOT, "pywfa_amd", "csrc", name), "rb").read())
    return h.hexdigest()[:12]


def med(x):
    return float(np.median(x))


rng = np.random.default_rng(2027)
codes = [rng.integers(0, 4, REFLEN) for _ in range(NREF)]
refs = [LUT[c].tobytes().decode() for c in codes]
nreads = 16384
ref_of = rng.integers(0, NREF, nreads)
pos_of = rng.integers(200, REFLEN - 400, nreads)
stored_rev = (np.arange(nreads) % 2).astype(np.uint8)
reads = []
for q in range(nreads):
    s = copy_of(rng, codes[ref_of[q]][pos_of[q]:pos_of[q] + READ + 8])
    reads.append((s.translate(COMP)[::-1] if stored_rev[q] else s).decode())
print(f"{nreads} reads of {READ} bp, {NREF} references of {REFLEN} bp; k_seed.hip + k_seed.hpp + wfa_seed.hpp sha256 {source_hash()}", flush=True)

al = WavefrontAligner(span="ends-free", text_begin_free=10, text_end_free=10)
with al.sequence_set(reads) as R, al.sequence_set(refs) as G:
    build_ms = []
    for _ in range(REPS):
        with al.seed_index(G) as idx:
            build_ms.append(idx.stats()["build_ms"])
    with al.seed_index(G) as idx:
        st = idx.stats()
        print(f"index: {st['positions']} positions, {st['masked_kmers']} k-mers over max_occ, {st['table_bytes'] / 2**20:.1f} MiB; build "
              f"median {med(build_ms):.3f} ms (min {min(build_ms):.3f}, max {max(build_ms):.3f})", flush=True)
        idx.seeds(R)   # warm-up
        q_ms, q_py = [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            s = idx.seeds(R)
            q_py.append(time.perf_counter() - t0)
            q_ms.append(idx.stats()["query_ms"])
        print(f"query: kernel median {med(q_ms):.3f} ms (min {min(q_ms):.3f}, max {max(q_ms):.3f}); seeds() from Python on open handles "
              f"median {med(q_py) * 1e3:.2f} ms (min {min(q_py) * 1e3:.2f}, max {max(q_py) * 1e3:.2f})", flush=True)
        inside = ((s["j"] == ref_of[:, None]) & (s["reverse"] == stored_rev[:, None]) & (s["text_start"] <= pos_of[:, None]) &
                  (s["text_start"] + s["text_len"] >= pos_of[:, None] + READ)).any(axis=1)
        print(f"locus inside a returned window: {inside.mean():.4f} of the reads; overflow {int(s['overflow'].sum())}; "
              f"{int((s['j'] >= 0).sum())} windows", flush=True)
        keep = s["j"] >= 0
        i = np.nonzero(keep)[0]
        args = dict(i=i, j=s["j"][keep], text_start=s["text_start"][keep], text_len=s["text_len"][keep],
                    reverse=s["reverse"][keep].astype(np.uint8), summary=True)
        al.align_windows(R, G, **args)   # warm-up
        a_py = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            al.align_windows(R, G, **args)
            a_py.append(time.perf_counter() - t0)
        print(f"align_windows(summary=True) on the {len(i)} windows, from Python on open handles: median {med(a_py) * 1e3:.2f} ms (min "
              f"{min(a_py) * 1e3:.2f}, max {max(a_py) * 1e3:.2f}); seeds() / align_windows = {med(q_py) / med(a_py):.3f}, query kernel / "
              f"align_windows = {med(q_ms) / (med(a_py) * 1e3):.3f}", flush=True)
al.close()
