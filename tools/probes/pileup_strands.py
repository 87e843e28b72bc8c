"""Probe of the per-strand pileup and the genotyped sites (pileup(strands=True), Pileup.genotypes).

Workload: that of tools/probes/pileup_index.py / pileup_insertions.py — 8 references of 1 Mb (fixed seed), 16 384 reads of 150 bp cut
from them at 2 %, every second one stored reverse-complemented; 1 M listed pairs against 300 bp windows.  In one process, medians of
REPS after a warm-up, with min and max:
 (1) pileup()                           (2) pileup(strands=True)             — (2) - (1) is the cost of the forward table
 (3) genotypes() over every reference, on the open pileup of (2)
 (4) the route (3) replaces: sites(), the forward counts of the sites' rows from counts(strand="+"), and the rule in NumPy — checked
     against (3)
and the HIP-event times of the two table kernels alone, the plain one and the stranded one, on the same batches
(WFA_HIP_REDUCE_TIMING=1 makes the library print them): about half the pairs add twice in the stranded one.
Run it under `timeout`.  Usage: pileup_strands.py [--pairs N] [--reps R]"""
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
MIN_DEPTH, PERMILLE, ERR_Q, MIN_ALT_STRAND = 8, 200, 20, 2


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
print(f"{nreads} reads of {READ} bp, {NREF} references of {REFLEN} bp, {n} listed pairs against {WIN} bp windows, "
      f"{int((stored_rev[i] == 0).sum())} of them forward", flush=True)
print(f"k_pileup.hip + k_calls.hip + wfa_pileup.hpp + wfa_calls.hpp sha256 {source_hash()}; medians of {REPS}", flush=True)


def genotype(R, A):
    """(gt, gq) of arrays of reference and alternate reads (int64)."""
    L = np.stack([ERR_Q * A, 3 * (R + A), ERR_Q * R], axis=1)
    low = np.sort(L, axis=1)
    return np.argmin(L, axis=1), np.minimum(99, low[:, 1] - low[:, 0])


def host_rule(p, G):
    """The genotype rows from sites() and the two tables of counts(): the strand filter, the genotypes and the forward counts in NumPy."""
    s = p.sites(G, min_depth=MIN_DEPTH, min_frac=PERMILLE / 1000)
    rows = np.stack([s[k] for k in p.SITE_COLUMNS], axis=1).astype(np.int64)
    total = np.concatenate([p.counts(r) for r in range(NREF)]).astype(np.int64)
    fwd = np.concatenate([p.counts(r, strand="+") for r in range(NREF)]).astype(np.int64)
    g = rows[:, 0] * REFLEN + rows[:, 1]
    c, f, r = total[g], fwd[g], rows[:, 2]
    k = np.arange(len(g))
    masked = c[:, :6].copy()
    masked[k, r] = -1
    alt = np.argmax(masked, axis=1)                       # (the smallest column among equals)
    A, depth = c[k, alt], c[:, :6].sum(axis=1)
    snv = (A >= 1) & (1000 * A >= PERMILLE * depth) & (f[k, alt] >= MIN_ALT_STRAND) & (A - f[k, alt] >= MIN_ALT_STRAND)
    ins = (c[:, 6] >= 1) & (1000 * c[:, 6] >= PERMILLE * depth) & (f[:, 6] >= MIN_ALT_STRAND) & (c[:, 6] - f[:, 6] >= MIN_ALT_STRAND)
    gt, gq = genotype(c[k, r], A)
    igt, igq = genotype(np.maximum(0, depth - c[:, 6]), c[:, 6])
    out = np.stack([rows[:, 0], rows[:, 1], r, np.where(snv, alt, -1), depth, c[k, r], np.where(snv, A, 0), c[:, 6],
                    np.where(snv, gt, -1), np.where(snv, gq, -1), np.where(ins, igt, -1), np.where(ins, igq, -1),
                    f[:, :6].sum(axis=1), f[k, r], np.where(snv, f[k, alt], 0), f[:, 6]], axis=1)
    return out[snv | ins].astype(np.int32)


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
wkw = dict(i=i, j=j, text_start=t_start, text_len=np.full(n, WIN, np.int32), reverse=stored_rev[i])
stranded = al.pileup(R, G, strands=True, **wkw)


def route_pileup(strands):
    al.pileup(R, G, strands=strands, **wkw).close()


GKW = dict(min_depth=MIN_DEPTH, min_frac=PERMILLE / 1000, err_q=ERR_Q, min_alt_strand=MIN_ALT_STRAND)
routes = {
    "(1) pileup()": lambda: route_pileup(False),
    "(2) pileup(strands=True)": lambda: route_pileup(True),
    "(3) genotypes(), every reference": lambda: stranded.genotypes(G, **GKW),
    "(4) sites() + counts() of both tables + the rule in NumPy": lambda: host_rule(stranded, G),
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
for what in ("pileup", "pileup stranded", "sites count", "sites scatter", "genotypes count", "genotypes scatter"):
    ms = err.ms(what)
    if ms:
        print(f"{what} kernel alone, HIP events: median {med(ms):.4f} ms per launch (min {min(ms):.4f}, max {max(ms):.4f}; {len(ms)} launches, "
              f"{sum(ms):.3f} ms in all)", flush=True)
plain_ms, stranded_ms = err.ms("pileup"), err.ms("pileup stranded")
if plain_ms and len(plain_ms) == len(stranded_ms):   # (a pileup() is one launch per batch of the list: the same batches both ways)
    print(f"stranded table kernel / plain table kernel, summed over the same batches and runs: {sum(stranded_ms) / sum(plain_ms):.4f}", flush=True)
t1, t2 = med(times["(1) pileup()"]), med(times["(2) pileup(strands=True)"])
print(f"strands cost (2) - (1) = {(t2 - t1) * 1e3:.2f} ms, (2) / (1) = {t2 / t1:.4f}; (3) / (4) = "
      f"{med(times['(3) genotypes(), every reference']) / med(times['(4) sites() + counts() of both tables + the rule in NumPy']):.5f}", flush=True)
# the routes agree
g = stranded.genotypes(G, **GKW)
dev_rows = np.stack([g[k] for k in stranded.GENOTYPE_COLUMNS], axis=1)
host_rows = host_rule(stranded, G)
print(f"device rows == host rows: {np.array_equal(dev_rows, host_rows)} ({len(dev_rows)} rows, {int((g['gt'] == 1).sum())} 0/1, "
      f"{int((g['gt'] == 2).sum())} 1/1)", flush=True)
stranded.close()
R.close()
G.close()
al.close()
