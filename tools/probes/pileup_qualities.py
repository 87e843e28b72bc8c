"""Probe of base qualities in the pileup (pileup(qualities=), Pileup.genotypes(qualities=True)).

Workload: that of tools/probes/pileup_strands.py — 8 references of 1 Mb (fixed seed), 16 384 reads of 150 bp cut from them at 2 %,
every second one stored reverse-complemented; 1 M listed pairs against 300 bp windows; a seeded quality per base in 0 .. 93.  In one
process, medians of REPS after a warm-up, with min and max:
 (1) pileup()                           (2) pileup(qualities=Q, min_base_quality=13)   — (2) - (1) is the cost of the quality table
 (3) genotypes() and (4) genotypes(qualities=True) over every reference, on the open pileup of (2)
and the HIP-event times of the two table kernels alone, the plain one and the one with qualities, on the same batches
(WFA_HIP_REDUCE_TIMING=1 makes the library print them): one more byte load and one more atomic per op.
Run it under `timeout`.  Usage: pileup_qualities.py [--pairs N] [--reps R]"""
import hashlib
import os
import re
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
os.environ["WFA_HIP_REDUCE_TIMING"] = "1"   # (read when an aligner is created)
import numpy as np  # noqa: E402

from pywfa_amd import WavefrontAligner  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
NPAIRS = int(sys.argv[sys.argv.index("--pairs") + 1]) if "--pairs" in sys.argv else 1 << 20
LUT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
READ, WIN, NREF, REFLEN = 150, 300, 8, 1 << 20
MIN_BASE_QUALITY, QUALITY_CAP = 13, 40


def source_hash():
    h = hashlib.sha256()
    for name in ("k_pileup.hip", "k_calls.hip", "wfa_pileup.hpp", "wfa_calls.hpp"):
        h.update(open(os.path.join(ROOT, "pywfa_amd", "csrc", name), "rb").read())
    return h.hexdigest()[:16]


def copy_of(rng, f, div=0.02):
    L = len(f)
    r = rng.random(L)
    sub = rng.integers(0, 4, L)
    first = np.where(r < div / 3, sub, f)
    cnt = np.where((r >= div / 3) & (r < 2 * div / 3), 0, np.where((r >= 2 * div / 3) & (r < div), 2, 1))
    vals = np.stack([first, sub], 1).ravel()
    keep = np.stack([cnt >= 1, cnt == 2], 1).ravel()
    out = vals[keep][:READ]
    return np.r_[out, sub[:READ - len(out)]]


rng = np.random.default_rng(2027)
codes = [rng.integers(0, 4, REFLEN) for _ in range(NREF)]
refs = [LUT[c].tobytes().decode() for c in codes]
nreads = 16384
ref_of = rng.integers(0, NREF, nreads)
pos_of = rng.integers(200, REFLEN - 400, nreads)
stored_rev = (np.arange(nreads) % 2).astype(np.uint8)
reads = []
for k in range(nreads):
    s = LUT[copy_of(rng, codes[ref_of[k]][pos_of[k]:pos_of[k] + READ + 8])].tobytes()
    reads.append((s.translate(COMP)[::-1] if stored_rev[k] else s).decode())
i = np.repeat(np.arange(nreads), 64)
t_start = np.repeat(pos_of, 64) - 75 + np.tile(np.arange(-32, 32), nreads)
order = rng.permutation(len(i))[:NPAIRS]
i, t_start = i[order].astype(np.int32), t_start[order].astype(np.int32)
j = ref_of[i].astype(np.int32)
n = len(i)
quals = [rng.integers(0, 94, READ).astype(np.uint8) for _ in range(nreads)]
print(f"{nreads} reads of {READ} bp, {NREF} references of {REFLEN} bp, {n} listed pairs against {WIN} bp windows; qualities 0 .. 93, "
      f"min_base_quality {MIN_BASE_QUALITY}, quality_cap {QUALITY_CAP}", flush=True)
print(f"k_pileup.hip + k_calls.hip + wfa_pileup.hpp + wfa_calls.hpp sha256 {source_hash()}; medians of {REPS}", flush=True)


def med(x):
    return float(np.median(x))


class Stderr:
    """The library's stderr lines of a block, for the kernels' HIP-event times."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode()
        self.tmp.close()
        return False

    def ms(self, what):
        return [float(x) for x in re.findall(rf"\[wfa_hip\] {what} kernel ([0-9.]+) ms", self.text)]


KW = dict(span="ends-free", text_begin_free=READ, text_end_free=READ)
al = WavefrontAligner(scope="full", **KW)
R, G = al.sequence_set(reads), al.sequence_set(refs)
Q = al.quality_set(R, quals)
wkw = dict(i=i, j=j, text_start=t_start, text_len=np.full(n, WIN, np.int32), reverse=stored_rev[i])
qkw = dict(qualities=Q, min_base_quality=MIN_BASE_QUALITY, quality_cap=QUALITY_CAP)
tracked = al.pileup(R, G, **qkw, **wkw)
GKW = dict(min_depth=8, min_frac=0.2, err_q=20)
routes = {
    "(1) pileup()": lambda: al.pileup(R, G, **wkw).close(),
    "(2) pileup(qualities=Q)": lambda: al.pileup(R, G, **qkw, **wkw).close(),
    "(3) genotypes(), every reference": lambda: tracked.genotypes(G, **GKW),
    "(4) genotypes(qualities=True), every reference": lambda: tracked.genotypes(G, qualities=True, **GKW),
}
times = {name: [] for name in routes}
with Stderr() as err:
    for fn in routes.values():
        fn()                                                # warm-up
    for _ in range(REPS):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
for name, t in times.items():
    print(f"{name}: median {med(t) * 1e3:.2f} ms (min {min(t) * 1e3:.2f}, max {max(t) * 1e3:.2f}; {len(t)} runs)", flush=True)
for what in ("pileup", "pileup qualities", "genotypes count", "genotypes scatter"):
    ms = err.ms(what)
    if ms:
        print(f"{what} kernel alone, HIP events: median {med(ms):.4f} ms per launch (min {min(ms):.4f}, max {max(ms):.4f}; {len(ms)} launches, "
              f"{sum(ms):.3f} ms in all)", flush=True)
plain_ms, qual_ms = err.ms("pileup"), err.ms("pileup qualities")
if plain_ms and len(plain_ms) == len(qual_ms):   # (a pileup() is one launch per batch of the list: the same batches both ways)
    print(f"quality table kernel / plain table kernel, summed over the same batches and runs: {sum(qual_ms) / sum(plain_ms):.4f}", flush=True)
t1, t2 = med(times["(1) pileup()"]), med(times["(2) pileup(qualities=Q)"])
print(f"qualities cost (2) - (1) = {(t2 - t1) * 1e3:.2f} ms, (2) / (1) = {t2 / t1:.4f}; (4) / (3) = "
      f"{med(times['(4) genotypes(qualities=True), every reference']) / med(times['(3) genotypes(), every reference']):.4f}", flush=True)
g = tracked.genotypes(G, qualities=True, **GKW)
print(f"{len(g['gt'])} rows, {int((g['gt'] == 1).sum())} 0/1, {int((g['gt'] == 2).sum())} 1/1; "
      f"{int(tracked.depth(0).sum())} counted bases on reference 0", flush=True)
tracked.close()
Q.close()
R.close()
G.close()
al.close()
