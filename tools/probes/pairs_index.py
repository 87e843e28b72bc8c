"""Probe of the indexed batches (WavefrontAligner.align_pairs, wfa_hip_batch_create_indexed).

Workload: 16 384 reads of 150 bp in 1 024 families of 16 at 2 % (fixed seed), 1 M listed pairs within families (every read against
the 16 reads of its family, 4 times over in a shuffled order: each read in ~64 pairs on either side), gap-affine end-to-end, scope
score and scope full.
(1) Kernel time, same pairs: last_kernel() of the indexed batch against last_kernel() of an explicit resident batch holding the same
    pairs in the same order; the two alternate in one process, medians of REPS runs, and the explicit batch's own spread (max - min).
(2) End to end from Python: align_pairs on two open handles, align_pairs including the two sequence_set uploads, and
    wavefront_align_batch on the materialised pair strings (building the strings is not timed); alternated, medians of REPS.
The generator's own time comes from a separate run under the kernel tracer:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o pairs -- python3 tools/probes/pairs_index.py --once
(--once: one creation and one run per scope, no repeats, so the trace holds exactly those).
Usage: pairs_index.py [--once] [--pairs N]"""
import hashlib
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pywfa_amd import WavefrontAligner, datagen  # noqa: E402

ONCE = "--once" in sys.argv
REPS = 1 if ONCE else 7
NPAIRS = int(sys.argv[sys.argv.index("--pairs") + 1]) if "--pairs" in sys.argv else 1 << 20
LUT = np.frombuffer(b"ACGT", np.uint8)


def copy_of(rng, f, div=0.02):
    """A copy of founder f (codes 0..3) with substitutions, deletions and insertions in equal parts at `div`."""
    L = len(f)
    r = rng.random(L)
    sub = rng.integers(0, 4, L)
    first = np.where(r < div / 3, sub, f)
    cnt = np.where((r >= div / 3) & (r < 2 * div / 3), 0, np.where((r >= 2 * div / 3) & (r < div), 2, 1))
    vals = np.stack([first, sub], 1).ravel()
    keep = np.stack([cnt >= 1, cnt == 2], 1).ravel()
    return LUT[vals[keep]].tobytes().decode()


def source_hash():
    h = hashlib.sha256()
    for name in ("k_pairs.hip", "wfa_cross.hpp"):
        h.update(open(os.path.join(ROOT, "pywfa_amd", "csrc", name), "rb").read())
    return h.hexdigest()[:12]


rng = np.random.default_rng(2026)
reads = []
for _ in range(1024):
    f = rng.integers(0, 4, 150)
    reads += [copy_of(rng, f) for _ in range(16)]
r = np.arange(16384)
i = np.tile(np.repeat(r, 16), 4)
j = np.tile(np.repeat(r // 16 * 16, 16) + np.tile(np.arange(16), 16384), 4)
order = rng.permutation(len(i))[:NPAIRS]
i, j = i[order].astype(np.int32), j[order].astype(np.int32)
n = len(i)
words = sum(((len(reads[a]) + 15) // 16 + (len(reads[b]) + 15) // 16) for a, b in zip(i[:4096], j[:4096])) / 4096
print(f"{len(reads)} reads, {n} listed pairs, {words:.1f} slot words per pair; k_pairs.hip + wfa_cross.hpp sha256 {source_hash()}", flush=True)
pats, texts = [reads[a] for a in i], [reads[b] for b in j]
explicit = datagen.from_strings(pats, texts, upper=True)


def med(x):
    return float(np.median(x))


for scope in ("score", "full"):
    al = WavefrontAligner(span="end-to-end", scope=scope)
    al.align_pairs(reads[:64], i=np.arange(64), j=np.arange(64)[::-1])   # (warm-up: first-run allocations, run-time kernels)
    al.wavefront_align_batch(texts[:2048], patterns=pats[:2048])
    # (1) kernel time, same pairs
    S = al.sequence_set(reads)
    rb_i = al._native.batch_indexed(S._set, None, i, j)
    rb_e = al.resident_batch(explicit)
    for rb in (rb_i, rb_e):   # warm-up
        rb.run()
        rb.sync()
    ms_i, ms_e = [], []
    for _ in range(REPS):
        for rb, ms in ((rb_e, ms_e), (rb_i, ms_i)):
            rb.run()
            rb.sync()
            ms.append(rb.last_kernel()[0])
    same = np.array_equal(rb_i.results(False)[0], rb_e.results(False)[0])
    rb_i.close()
    rb_e.close()
    print(f"[{scope}] kernel ms, {n} pairs: indexed median {med(ms_i):.3f} (min {min(ms_i):.3f}, max {max(ms_i):.3f}); explicit median "
          f"{med(ms_e):.3f} (min {min(ms_e):.3f}, max {max(ms_e):.3f}, spread {max(ms_e) - min(ms_e):.3f}); ratio "
          f"{med(ms_i) / med(ms_e):.4f}; difference of medians {med(ms_i) - med(ms_e):+.3f} ms; same scores: {same}", flush=True)
    # (2) end to end from Python
    t_open, t_up, t_ex = [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        al.wavefront_align_batch(texts, patterns=pats)
        t_ex.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        al.align_pairs(S, i=i, j=j)
        t_open.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        with al.sequence_set(reads) as A, al.sequence_set(reads) as B:
            al.align_pairs(A, B, i=i, j=j)
        t_up.append(time.perf_counter() - t0)
    S.close()
    print(f"[{scope}] end to end ms: align_pairs on open handles median {med(t_open) * 1e3:.1f} (min {min(t_open) * 1e3:.1f}, max "
          f"{max(t_open) * 1e3:.1f}); with two sequence_set uploads median {med(t_up) * 1e3:.1f} (min {min(t_up) * 1e3:.1f}, max "
          f"{max(t_up) * 1e3:.1f}); wavefront_align_batch on the pair strings median {med(t_ex) * 1e3:.1f} (min {min(t_ex) * 1e3:.1f}, "
          f"max {max(t_ex) * 1e3:.1f}, spread {(max(t_ex) - min(t_ex)) * 1e3:.1f})", flush=True)
    al.close()
