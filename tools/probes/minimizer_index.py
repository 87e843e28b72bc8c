"""Probe of the minimizer index (WavefrontAligner.seed_index(w=...), wfa_hip_seed_index_create_minimizer) beside the
stride index of the nearest density, on the two workloads of seed_index.py and chain_index.py, from the same generators and seeds.

Short: 8 references of 1 Mb, 16 384 reads of 150 bp at 2 %, every second one stored reverse-complemented; seeds() with its defaults
(n = 4, min_hits 2, gap 16, pad 16, max_hits 2048); ends-free with 10 free text bases, scope full.
Long: 8 references of 1 Mb, 4 096 reads of 10 kb at 8 %; chains() with its defaults (n = 4, min_hits 3, min_score 40, lookback 32,
max_dist 5000, band 500, pad 64, max_anchors 16 384); ends-free with 200 free text bases, heuristic "adaptive".
Indexes: (k = 13, w = 10) and (k = 15, w = 10), and beside each the stride index of the same k with stride 6 (density 1/6 = 0.167
against 2/11 = 0.182; stride 5 would be 0.200), max_occ 64.
Per index and workload: indexed positions and bytes; build ms, query-kernel ms (short) or chain-kernel ms and chains() wall time
(long) — kernels by HIP events (SeedIndex.stats()), medians of REPS after a warm-up, min and max shown; hits or anchors per read (the
first window's); the locus share; align_windows(summary=True) on the returned windows, from Python on open handles.
Usage: minimizer_index.py [--reps N] [--short-reads N] [--long-reads N]"""
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


REPS, NSHORT, NLONG = arg("--reps", 5), arg("--short-reads", 16384), arg("--long-reads", 4096)
LUT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
NREF, REFLEN = 8, 1 << 20
INDEXES = [dict(k=13, w=10), dict(k=13, stride=6), dict(k=15, w=10), dict(k=15, stride=6)]


def copy_of(rng, f, div, cut=None):
    """A copy of f (codes 0..3) with substitutions, deletions and insertions in equal parts at `div`; `cut`: cut or padded to that
    many bases (seed_index.py), otherwise as long as it comes (chain_index.py)."""
    L = len(f)
    r = rng.random(L)
    sub = rng.integers(0, 4, L)
    first = np.where(r < div / 3, sub, f)
    cnt = np.where((r >= div / 3) & (r < 2 * div / 3), 0, np.where((r >= 2 * div / 3) & (r < div), 2, 1))
    vals = np.stack([first, sub], 1).ravel()
    keep = np.stack([cnt >= 1, cnt == 2], 1).ravel()
    out = vals[keep]
    if cut is not None:
        out = out[:cut]
        out = np.r_[out, sub[:cut - len(out)]]
    return LUT[out].tobytes()


def source_hash():
    h = hashlib.sha256()
    for name in ("k_seed.hip", "k_seed.hpp", "wfa_seed.hpp", "k_chain.hip", "wfa_chain.hpp"):
        h.update(open(os.path.join(ROOT, "pywfa_amd", "csrc", name), "rb").read())
    return h.hexdigest()[:12]


def mmm(x, scale=1.0):
    return f"median {float(np.median(x)) * scale:.3f} ms (min {min(x) * scale:.3f}, max {max(x) * scale:.3f})"


def workload(seed, nreads, read, div, margin, cut):
    """seed_index.py (seed 2027) / chain_index.py (seed 2028): the references, the stored reads and where they come from."""
    rng = np.random.default_rng(seed)
    codes = [rng.integers(0, 4, REFLEN) for _ in range(NREF)]
    refs = [LUT[c].tobytes().decode() for c in codes]
    ref_of = rng.integers(0, NREF, nreads)
    pos_of = rng.integers(200, REFLEN - margin, nreads)
    stored_rev = (np.arange(nreads) % 2).astype(np.uint8)
    reads = []
    for q in range(nreads):
        s = copy_of(rng, codes[ref_of[q]][pos_of[q]:pos_of[q] + read + (8 if cut else 0)], div, read if cut else None)
        reads.append((s.translate(COMP)[::-1] if stored_rev[q] else s).decode())
    return refs, reads, ref_of, pos_of, stored_rev


def inside(rows, ref_of, pos_of, stored_rev, span):
    return ((rows["j"] == ref_of[:, None]) & (rows["reverse"] == stored_rev[:, None]) & (rows["text_start"] <= pos_of[:, None]) &
            (rows["text_start"] + rows["text_len"] >= pos_of[:, None] + span)).any(axis=1).mean()


def run(al, name, long_reads, refs, reads, ref_of, pos_of, stored_rev, span):
    with al.sequence_set(reads) as R, al.sequence_set(refs) as G:
        for params in INDEXES:
            label = ", ".join(f"{key} = {v}" for key, v in params.items())
            with al.seed_index(G, **params):
                pass   # warm-up
            build = []
            for _ in range(REPS):
                with al.seed_index(G, **params) as idx:
                    build.append(idx.stats()["build_ms"])
            with al.seed_index(G, **params) as idx:
                st = idx.stats()
                print(f"[{name}; {label}] {st['positions']} positions, {st['table_bytes']} bytes ({st['table_bytes'] / 2**20:.1f} MiB), "
                      f"{st['masked_kmers']} k-mers over max_occ; build {mmm(build)}", flush=True)
                call = idx.chains if long_reads else idx.seeds
                call(R)   # warm-up
                kern, wall = [], []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    rows = call(R)
                    wall.append(time.perf_counter() - t0)
                    kern.append(idx.stats()["chain_ms" if long_reads else "query_ms"])
                what = "chain" if long_reads else "query"
                print(f"[{name}; {label}] {what} kernel {mmm(kern)}; {call.__name__}() from Python on open handles {mmm(wall, 1e3)}", flush=True)
                print(f"[{name}; {label}] {'anchors' if long_reads else 'hits'} of the first window per read: median "
                      f"{int(np.median(rows['hits'][:, 0]))}, mean {rows['hits'][:, 0].mean():.1f}; overflow {int(rows['overflow'].sum())}; "
                      f"{int((rows['j'] >= 0).sum())} windows; locus inside a returned window: "
                      f"{inside(rows, ref_of, pos_of, stored_rev, span):.4f} of the reads", flush=True)
                keep = rows["j"] >= 0
                i = np.nonzero(keep)[0]
                args = dict(i=i, j=rows["j"][keep], text_start=rows["text_start"][keep], text_len=rows["text_len"][keep],
                            reverse=rows["reverse"][keep].astype(np.uint8), summary=True)
                al.align_windows(R, G, **args)   # warm-up
                a_py = []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    al.align_windows(R, G, **args)
                    a_py.append(time.perf_counter() - t0)
                print(f"[{name}; {label}] align_windows(summary=True) on the {len(i)} windows, from Python on open handles: {mmm(a_py, 1e3)}",
                      flush=True)


print(f"k_seed.hip + k_seed.hpp + wfa_seed.hpp + k_chain.hip + wfa_chain.hpp sha256 {source_hash()}; medians of {REPS}", flush=True)
al = WavefrontAligner(span="ends-free", text_begin_free=10, text_end_free=10)
run(al, f"{NSHORT} reads of 150 bp at 2 %", False, *workload(2027, NSHORT, 150, 0.02, 400, True), 150)
al.close()
al = WavefrontAligner(span="ends-free", text_begin_free=200, text_end_free=200, heuristic="adaptive")
run(al, f"{NLONG} reads of 10 kb at 8 %", True, *workload(2028, NLONG, 10000, 0.08, 10000 + 400, False), 10000)
al.close()
