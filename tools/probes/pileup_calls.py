"""Probe of the calls and sites reductions of a pileup (Pileup.calls / sites).

Workload: the pileup of tools/probes/pileup_index.py — 8 references of 1 Mb (fixed seed), 16 384 reads of 150 bp cut from them at 2 %,
every second one stored reverse-complemented; 1 M listed pairs against 300 bp windows, piled up once.  On the open handles, in one
process, medians of REPS after a warm-up, with min and max:
 (1) sites() over every reference                      (2) calls() of every reference, one call each
 (3) today's route to the same answers: counts() of every reference, then the two rules in NumPy on the host (checked against (1), (2))
and the HIP-event times of the kernels alone (WFA_HIP_REDUCE_TIMING=1 makes the library print them).
Run it under `timeout`.  Usage: pileup_calls.py [--pairs N] [--reps R]"""
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
MIN_DEPTH, PERMILLE = 1, 500


def source_hash():
    h = hashlib.sha256()
    for name in ("k_calls.hip", "wfa_calls.hpp"):
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
    return LUT[np.r_[out, sub[:READ - len(out)]]].tobytes()


rng = np.random.default_rng(2027)
codes = [rng.integers(0, 4, REFLEN) for _ in range(NREF)]
refs = [LUT[c].tobytes().decode() for c in codes]
nreads = 16384
ref_of = rng.integers(0, NREF, nreads)
pos_of = rng.integers(200, REFLEN - 400, nreads)
stored_rev = (np.arange(nreads) % 2).astype(np.uint8)
reads = []
for k in range(nreads):
    s = copy_of(rng, codes[ref_of[k]][pos_of[k]:pos_of[k] + READ + 8])
    reads.append((s.translate(COMP)[::-1] if stored_rev[k] else s).decode())
i = np.repeat(np.arange(nreads), 64)
t_start = np.repeat(pos_of, 64) - 75 + np.tile(np.arange(-32, 32), nreads)
order = rng.permutation(len(i))[:NPAIRS]
i, t_start = i[order].astype(np.int32), t_start[order].astype(np.int32)
j = ref_of[i].astype(np.int32)
n = len(i)
print(f"{nreads} reads of {READ} bp, {NREF} references of {REFLEN} bp, {n} listed pairs against {WIN} bp windows", flush=True)
print(f"k_calls.hip + wfa_calls.hpp sha256 {source_hash()}; medians of {REPS}", flush=True)

REF_COLS = [c.astype(np.int64) for c in codes]   # (LUT's order A C G T is the column order)


def host_rules(counts, r):
    """The two rules in NumPy on the rows of one reference (its reference columns `r`): (call bytes, site rows without j)."""
    c = counts[:, :6].astype(np.int64)
    ins = counts[:, 6].astype(np.int64)
    depth = c.sum(axis=1)
    rows = np.arange(len(c))
    top = c.max(axis=1)
    code = np.where(c[rows, r] == top, r, c.argmax(axis=1))
    call = np.where(depth < MIN_DEPTH, 6, code | np.where(2 * ins > depth, 8, 0)).astype(np.uint8)
    masked = c.copy()
    masked[rows, r] = -1
    alt = masked.argmax(axis=1)
    A = c[rows, alt]
    snv = (A >= 1) & (1000 * A >= PERMILLE * depth)
    site = (depth >= MIN_DEPTH) & (snv | ((ins >= 1) & (1000 * ins >= PERMILLE * depth)))
    g = np.flatnonzero(site)
    out = np.stack([g, r[g], np.where(snv[g], alt[g], -1), depth[g], c[g, r[g]], np.where(snv[g], A[g], 0), ins[g]], axis=1)
    return call, out.astype(np.int32)


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
p = al.pileup(R, G, i=i, j=j, text_start=t_start, text_len=np.full(n, WIN, np.int32), reverse=stored_rev[i])


def route_host():
    return [host_rules(p.counts(r), REF_COLS[r]) for r in range(NREF)]


def route_calls():
    return [p.calls(G, r, min_depth=MIN_DEPTH) for r in range(NREF)]


routes = {
    "(1) sites(), every reference": lambda: p.sites(G, min_depth=MIN_DEPTH, min_frac=PERMILLE / 1000),
    "(2) calls(), 8 references": route_calls,
    "(3) counts() of 8 references + the rules in NumPy": route_host,
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
for what in ("calls", "sites count", "sites scatter"):
    ms = err.ms(what)
    print(f"{what} kernel(s) alone, HIP events: median {med(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}; {len(ms)} launches)", flush=True)
host = med(times["(3) counts() of 8 references + the rules in NumPy"])
print(f"(1) / (3) = {med(times['(1) sites(), every reference']) / host:.5f}; (2) / (3) = {med(times['(2) calls(), 8 references']) / host:.5f}",
      flush=True)
# the routes agree
s = p.sites(G, min_depth=MIN_DEPTH, min_frac=PERMILLE / 1000)
dev_rows = np.stack([s[k] for k in p.SITE_COLUMNS], axis=1)
dev_calls = route_calls()
hosted = route_host()
host_rows = np.concatenate([np.concatenate([np.full((len(rows), 1), r, np.int32), rows], axis=1) for r, (_, rows) in enumerate(hosted)])
same_calls = all(np.array_equal(d["code"] | (d["ins"].astype(np.uint8) << 3), h[0]) for d, h in zip(dev_calls, hosted))
print(f"device sites == host sites: {np.array_equal(dev_rows, host_rows)} ({len(dev_rows)} sites); device calls == host calls: {same_calls}", flush=True)
p.close()
R.close()
G.close()
al.close()
