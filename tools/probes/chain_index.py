"""Probe of chaining on the seed index (SeedIndex.chains, wfa_hip_seed_index_chain).

Workload: 8 references of 1 Mb (fixed seed), 4 096 reads of 10 kb cut from random positions of them at 8 % (substitutions, deletions
and insertions in equal parts), every second one stored reverse-complemented.  Index k = 13, stride 8, max_occ 64; chains() with its
defaults (n = 4, min_hits 3, min_score 40, lookback 32, max_dist 5000, band 500, pad 64, max_anchors 16 384); gap-affine, ends-free
with 200 free text bases on either side, scope full, heuristic "adaptive" (WFA's wf-adaptive).
(1) The index build and the chain kernel by HIP events (SeedIndex.stats()), and chains() from Python on open handles; medians of REPS.
(2) The share of reads whose true locus lies inside one of their windows, on the right reference and strand.
(3) The share of the same reads for which seeds() (the same index, max_hits 4 096) overflows.
(4) align_windows(summary=True) on the returned windows, from Python on open handles, and the chain kernel's share of that time.
Usage: chain_index.py [--reps N] [--reads N]"""
import hashlib
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pywfa_amd import WavefrontAligner  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPS, NREADS = arg("--reps", 5), arg("--reads", 4096)
LUT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
READ, NREF, REFLEN, DIV = 10000, 8, 1 << 20, 0.08


def copy_of(rng, f, div):
    """A copy of f (codes 0..3) with substitutions, deletions and insertions in equal parts at `div`."""
    L = len(f)
    r = rng.random(L)
    sub = rng.integers(0, 4, L)
    first = np.where(r < div / 3, sub, f)
    cnt = np.where((r >= div / 3) & (r < 2 * div / 3), 0, np.where((r >= 2 * div / 3) & (r < div), 2, 1))
    vals = np.stack([first, sub], 1).ravel()
    keep = np.stack([cnt >= 1, cnt == 2], 1).ravel()
    return LUT[vals[keep]].tobytes()


def source_hash():
    h = hashlib.sha256()
    for name in ("k_chain.hip", "wfa_chain.hpp", "k_seed.hpp", "wfa_seed.hpp"):
        h.update(open(os.path.join(ROOT, "pywfa_amd", "csrc", name), "rb").read())
    return h.hexdigest()[:12]


def med(x):
    return float(np.median(x))


rng = np.random.default_rng(2028)
codes = [rng.integers(0, 4, REFLEN) for _ in range(NREF)]
refs = [LUT[c].tobytes().decode() for c in codes]
ref_of = rng.integers(0, NREF, NREADS)
pos_of = rng.integers(200, REFLEN - READ - 400, NREADS)
stored_rev = (np.arange(NREADS) % 2).astype(np.uint8)
reads = []
for q in range(NREADS):
    s = copy_of(rng, codes[ref_of[q]][pos_of[q]:pos_of[q] + READ], DIV)
    reads.append((s.translate(COMP)[::-1] if stored_rev[q] else s).decode())
print(f"{NREADS} reads cut from {READ} bp at {DIV:.0%}, {NREF} references of {REFLEN} bp; k_chain.hip + wfa_chain.hpp + k_seed.hpp + "
      f"wfa_seed.hpp sha256 {source_hash()}", flush=True)

al = WavefrontAligner(span="ends-free", text_begin_free=200, text_end_free=200, heuristic="adaptive")
with al.sequence_set(reads) as R, al.sequence_set(refs) as G:
    build_ms = []
    for _ in range(REPS):
        with al.seed_index(G, stride=8) as idx:
            build_ms.append(idx.stats()["build_ms"])
    with al.seed_index(G, stride=8) as idx:
        st = idx.stats()
        print(f"index: {st['positions']} positions, {st['masked_kmers']} k-mers over max_occ, {st['table_bytes'] / 2**20:.1f} MiB; build "
              f"median {med(build_ms):.3f} ms (min {min(build_ms):.3f}, max {max(build_ms):.3f})", flush=True)
        idx.chains(R)   # warm-up (allocates the workspace)
        c_ms, c_py = [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            c = idx.chains(R)
            c_py.append(time.perf_counter() - t0)
            c_ms.append(idx.stats()["chain_ms"])
        print(f"chains: kernel median {med(c_ms):.3f} ms (min {min(c_ms):.3f}, max {max(c_ms):.3f}); chains() from Python on open handles "
              f"median {med(c_py) * 1e3:.2f} ms (min {min(c_py) * 1e3:.2f}, max {max(c_py) * 1e3:.2f}); workspace "
              f"{idx.stats()['chain_workspace_bytes'] / 2**20:.1f} MiB", flush=True)
        inside = ((c["j"] == ref_of[:, None]) & (c["reverse"] == stored_rev[:, None]) & (c["text_start"] <= pos_of[:, None]) &
                  (c["text_start"] + c["text_len"] >= pos_of[:, None] + READ)).any(axis=1)
        print(f"locus inside a returned window: {inside.mean():.4f} of the reads; overflow {int(c['overflow'].sum())}; "
              f"{int((c['j'] >= 0).sum())} windows; hits of the first chain: median {int(np.median(c['hits'][:, 0]))}", flush=True)
        s = idx.seeds(R, max_hits=4096)
        print(f"seeds(max_hits=4096) on the same reads: overflow for {s['overflow'].mean():.4f} of them", flush=True)
        keep = c["j"] >= 0
        i = np.nonzero(keep)[0]
        args = dict(i=i, j=c["j"][keep], text_start=c["text_start"][keep], text_len=c["text_len"][keep],
                    reverse=c["reverse"][keep].astype(np.uint8), summary=True)
        al.align_windows(R, G, **args)   # warm-up
        a_py = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            al.align_windows(R, G, **args)
            a_py.append(time.perf_counter() - t0)
        print(f"align_windows(summary=True, heuristic adaptive) on the {len(i)} windows, from Python on open handles: median "
              f"{med(a_py) * 1e3:.2f} ms (min {min(a_py) * 1e3:.2f}, max {max(a_py) * 1e3:.2f}); chains() / align_windows = "
              f"{med(c_py) / med(a_py):.4f}, chain kernel / align_windows = {med(c_ms) / (med(a_py) * 1e3):.4f}", flush=True)
al.close()
