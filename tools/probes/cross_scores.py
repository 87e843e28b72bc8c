"""Probe of the score matrices: all-vs-all of read families (founders x copies at 2 % divergence, 150 bp, fixed seed) under max_steps.

Reports (1) the cross run's kernel time (wfa_hip_cross_kernel_ms) against wfa_hip_batch_last_kernel_ms of a resident explicit batch of
the same upper-triangle pairs, (2) end-to-end Python time of completed_pairs against building those pairs and calling
wavefront_align_batch, (3) the completed pairs both find.  Usage: cross_scores.py [founders] [copies] [max_steps]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np  # noqa: E402

from pywfa_amd import WavefrontAligner, _native, datagen  # noqa: E402

founders = int(sys.argv[1]) if len(sys.argv) > 1 else 256
copies = int(sys.argv[2]) if len(sys.argv) > 2 else 16
rng = np.random.default_rng(2024)
reads = []
for _ in range(founders):
    f = rng.integers(0, 4, 150)
    for _ in range(copies):
        r = rng.random(150)
        sub = rng.integers(0, 4, 150)
        out = []
        for k in range(150):   # 2 %: substitutions, deletions, insertions in equal parts
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
reads = [reads[k] for k in order]
n = len(reads)
# within a family two copies differ by ~4 % of 150 bases: ~6 edits, ~30 under affine 4/6/2 -> max_steps 3x that
max_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 90
kw = dict(span="end-to-end", scope="score", max_steps=max_steps)
print(f"{n} reads ({founders} founders x {copies} copies, 150 bp, 2 %), all-vs-all, max_steps {max_steps}", flush=True)

# (1) kernel time: the cross run against a resident explicit batch of the same upper-triangle pairs (i <= j: what the mirror rule aligns)
al = WavefrontAligner(**kw)
al.completed_pairs(reads[:64])   # (warm-up: first-run allocations)
blob = datagen.from_strings(b"", reads, upper=True)
ss = al._native.seqset(blob["seqs"], blob["t_off"], blob["t_len"])
cross_ms = []
for rep in range(3):
    x = al._native.cross(ss, None, _native.CROSS_COMPLETED)
    ms, pairs = x.kernel_ms()
    cross_ms.append(ms)
    x.close()
ss.close()
iu, ju = np.triu_indices(n)
pp = [reads[i] for i in iu]
tt = [reads[j] for j in ju]
batch = datagen.from_strings(pp, tt, upper=True)
rb = al.resident_batch(batch)
batch_ms = []
for rep in range(3):
    rb.run()
    rb.sync()
    batch_ms.append(rb.last_kernel()[0])
rb.close()
del batch
cm, bm = min(cross_ms), min(batch_ms)
print(f"kernel: cross {cm:.2f} ms for {pairs} pairs ({pairs / cm / 1e6:.2f} G aln/s); resident explicit batch {bm:.2f} ms for {len(iu)} pairs "
      f"({len(iu) / bm / 1e6:.2f} G aln/s); cross / batch = {cm / bm:.3f}", flush=True)

# (2) end to end from Python strings
t0 = time.perf_counter()
c = al.completed_pairs(reads)
t_cross = time.perf_counter() - t0
t0 = time.perf_counter()
iu, ju = np.triu_indices(n, 1)
pp = [reads[i] for i in iu]
tt = [reads[j] for j in ju]
r = al.wavefront_align_batch(tt, pp)
keep = np.asarray(r["status"]) == 0
ei, ej, es = iu[keep], ju[keep], np.asarray(r["score"])[keep]
t_expl = time.perf_counter() - t0
print(f"end to end: completed_pairs {t_cross * 1e3:.1f} ms; build {len(iu)} pairs + wavefront_align_batch + filter {t_expl * 1e3:.1f} ms; "
      f"{t_expl / t_cross:.1f}x", flush=True)

# (3) the same pairs
same = np.array_equal(c["i"], ei) and np.array_equal(c["j"], ej) and np.array_equal(c["score"], es)
print(f"completed pairs: cross {len(c['i'])}, explicit {int(keep.sum())}, identical lists: {same}")
