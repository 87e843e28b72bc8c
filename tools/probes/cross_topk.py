"""Probe of the top-k per row of the score matrices (WavefrontAligner.nearest).

(1) The §6.4 workload (256 founders x 16 copies of 150 bp at 2 %, fixed seed, all-vs-all, end-to-end, max_steps 90) with k = 1, 8 and
64: end-to-end nearest() time against completed_pairs(), and wfa_hip_cross_kernel_ms (the alignment kernels) of both runs.
(2) A rectangle of 256 queries x 262 144 candidates of 150 bp (16 384 founders x 16 copies; each query one more copy of one of 256
founders), max_steps 90, k = 16: end-to-end nearest() against score_matrix() followed by a host argpartition, and both agree.
The reduction kernels' own time comes from a separate run under the kernel tracer:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o topk -- python3 tools/probes/cross_topk.py --once
(--once: every run once, no timing repeats, so the trace holds exactly the runs above).
Usage: cross_topk.py [--once] [--skip-rect] [--skip-ava]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np  # noqa: E402

from pywfa_amd import WavefrontAligner, _native, datagen  # noqa: E402

ONCE = "--once" in sys.argv
REPS = 1 if ONCE else 3
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


def section_6_4_reads():
    """tools/probes/cross_scores.py's reads (the same seed and the same draws)."""
    rng = np.random.default_rng(2024)
    reads = []
    for _ in range(256):
        f = rng.integers(0, 4, 150)
        for _ in range(16):
            r = rng.random(150)
            sub = rng.integers(0, 4, 150)
            out = []
            for k in range(150):
                if r[k] < 0.02 / 3:
                    out.append(sub[k])
                elif r[k] < 0.04 / 3:
                    continue
                elif r[k] < 0.02:
                    out += [f[k], sub[k]]
                else:
                    out.append(f[k])
            reads.append("".join("ACGT"[x] for x in out))
    order = rng.permutation(len(reads))
    return [reads[k] for k in order]


def timed(fn):
    best, out = None, None
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def kernel_ms(al, sets, want, k=None):
    x = al._native.cross(sets[0], sets[1] if len(sets) > 1 else None, want, k)
    ms, pairs = x.kernel_ms()
    x.close()
    return ms, pairs


kw = dict(span="end-to-end", scope="score", max_steps=90)
al = WavefrontAligner(**kw)
al.completed_pairs(["ACGT" * 30] * 64)   # (warm-up: first-run allocations)

# (1) all-vs-all, k = 1 / 8 / 64 against completed_pairs
reads = [] if "--skip-ava" in sys.argv else section_6_4_reads()
n = len(reads)
if n:
    print(f"(1) {n} reads (256 founders x 16 copies, 150 bp, 2 %), all-vs-all, max_steps 90", flush=True)
    t_c, c = timed(lambda: al.completed_pairs(reads))
    blob = datagen.from_strings(b"", reads, upper=True)
    ss = al._native.seqset(blob["seqs"], blob["t_off"], blob["t_len"])
    ms_c, pairs = kernel_ms(al, [ss], _native.CROSS_COMPLETED)
    print(f"completed_pairs: {t_c * 1e3:.1f} ms end to end, alignment kernels {ms_c:.2f} ms for {pairs} pairs, {len(c['i'])} pairs", flush=True)
    for k in (1, 8, 64):
        t_k, r = timed(lambda: al.nearest(reads, k=k))
        ms_k, _ = kernel_ms(al, [ss], _native.CROSS_TOPK, k)
        print(f"nearest k={k}: {t_k * 1e3:.1f} ms end to end ({t_k / t_c:.3f} x completed_pairs), alignment kernels {ms_k:.2f} ms; "
              f"rows with k hits {int((r['j'][:, -1] >= 0).sum())} / {n}", flush=True)
    ss.close()

if "--skip-rect" in sys.argv:
    sys.exit(0)

# (2) rectangle 256 x 262 144, k = 16, against score_matrix + host argpartition
rng = np.random.default_rng(7)
cands = []
founders = [rng.integers(0, 4, 150) for _ in range(16384)]
for f in founders:
    for _ in range(16):
        cands.append(copy_of(rng, f))
perm = rng.permutation(len(cands))
cands = [cands[p] for p in perm]
queries = [copy_of(rng, founders[int(x)]) for x in rng.choice(len(founders), 256, replace=False)]
K = 16
NONE = -(1 << 40)   # (a key below every score, and one that negates)
print(f"(2) {len(queries)} queries x {len(cands)} candidates, 150 bp, max_steps 90, k = {K}", flush=True)
t_n, r = timed(lambda: al.nearest(queries, cands, k=K))


def dense_topk():
    score, status = al.score_matrix(queries, cands)
    key = np.where(status == 0, score.astype(np.int64), NONE)
    part = np.argpartition(-key, K, axis=1)[:, :K]   # (K < N: the K largest, unordered, ties arbitrary at the edge)
    return key, part


t_d, (key, part) = timed(dense_topk)
ok = True   # agree on the scores of the K best (ties at the K-th may pick other columns in argpartition)
for i in range(len(queries)):
    want = np.sort(key[i, part[i]])[::-1]
    got = np.where(r["j"][i] >= 0, r["score"][i].astype(np.int64), NONE)
    ok &= bool(np.array_equal(got, want))
blob_q = datagen.from_strings(b"", queries, upper=True)
blob_t = datagen.from_strings(b"", cands, upper=True)
sq = al._native.seqset(blob_q["seqs"], blob_q["t_off"], blob_q["t_len"])
st = al._native.seqset(blob_t["seqs"], blob_t["t_off"], blob_t["t_len"])
ms_n, pairs = kernel_ms(al, [sq, st], _native.CROSS_TOPK, K)
ms_d, _ = kernel_ms(al, [sq, st], _native.CROSS_DENSE)
sq.close()
st.close()
print(f"nearest: {t_n * 1e3:.1f} ms end to end (alignment kernels {ms_n:.2f} ms for {pairs} pairs); score_matrix + argpartition "
      f"{t_d * 1e3:.1f} ms (alignment kernels {ms_d:.2f} ms); {t_d / t_n:.2f}x; same top-{K} scores: {ok}; "
      f"rows with {K} hits {int((r['j'][:, -1] >= 0).sum())} / {len(queries)}", flush=True)
