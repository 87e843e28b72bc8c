"""Probe of the deletion log of a pileup (pileup(deletions=True), Pileup.deletions).

Workload: that of tools/probes/pileup_index.py / pileup_insertions.py — 8 references of 1 Mb (fixed seed), 16 384 reads of 150 bp cut
from them at 2 %, every second one stored reverse-complemented; 1 M listed pairs against 300 bp windows.  In one process, medians of
REPS after a warm-up, with min and max:
 (1) pileup() without tracking          (2) pileup(deletions=True)          — (2) - (1) is the cost of tracking
 (3) deletions() over every reference, on the open pileup of (2)
 (4) the route (3) replaces: align_windows with CIGARs (their run-length encoding comes back), then the records, the starts plane and
     the allele rule in NumPy / Python on the host, with the depth from counts() — checked against (3)
and the HIP-event times of the two record kernels and of the reduction alone (WFA_HIP_REDUCE_TIMING=1 makes the library print them).
Run it under `timeout`.  Usage: pileup_deletions.py [--pairs N] [--reps R]"""
import collections
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
MIN_DEPTH, PERMILLE = 8, 500


def source_hash():
    h = hashlib.sha256()
    for name in ("k_deletions.hip", "wfa_deletions.hpp", "k_pileup.hip"):
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
print(f"{nreads} reads of {READ} bp, {NREF} references of {REFLEN} bp, {n} listed pairs against {WIN} bp windows", flush=True)
print(f"k_deletions.hip + wfa_deletions.hpp + k_pileup.hip sha256 {source_hash()}; medians of {REPS}", flush=True)


def host_records(out):
    """The records of the listed pairs from the run-length encoding align_windows returns: (global row, length) per I run of an
    aligned core, 64 k pairs at a time."""
    seq = out["cigar_ops"]
    off, code, rlen = seq._off, seq._code.astype(np.int64), seq._len.astype(np.int64)
    ok = np.flatnonzero(out["status"] == 0)
    parts = []
    for lo in range(0, len(ok), 1 << 16):
        q = ok[lo:lo + (1 << 16)]
        cnt = off[q + 1] - off[q]
        pair = np.repeat(np.arange(len(q)), cnt)
        ridx = np.repeat(off[q], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        c, ln = code[ridx], rlen[ridx]
        first = np.r_[0, np.cumsum(cnt)[:-1]]
        on_h = np.where((c == 0) | (c == 1) | (c == 8), ln, 0)
        h0 = np.cumsum(on_h) - on_h
        h0 -= np.repeat(h0[first], cnt)
        k = np.arange(len(c))
        is_m = c == 0
        fm = np.full(len(q), len(c), np.int64)
        np.minimum.at(fm, pair[is_m], k[is_m])
        lm = np.full(len(q), -1, np.int64)
        np.maximum.at(lm, pair[is_m], k[is_m])
        sel = (c == 1) & (k >= fm[pair]) & (k <= lm[pair])
        rows = (j[q].astype(np.int64) * REFLEN + t_start[q])[pair[sel]] + h0[sel]
        parts.append(np.stack([rows, ln[sel]], axis=1))
    return np.concatenate(parts)


def host_rule(recs, tables):
    """The reported rows from the records and the tables of counts(): (j, pos, depth, S, count, len, alleles, 0)."""
    depth = np.concatenate(tables)[:, :6].astype(np.int64).sum(axis=1)
    S = np.bincount(recs[:, 0], minlength=len(depth)).astype(np.int64)
    chosen = np.flatnonzero((depth >= MIN_DEPTH) & (S >= 1) & (1000 * S >= PERMILLE * depth))
    recs = recs[np.isin(recs[:, 0], chosen)]
    at = collections.defaultdict(collections.Counter)
    for g, ln in recs.tolist():
        at[g][ln] += 1
    rows = []
    for g in chosen.tolist():
        ln, count = min(at[g].items(), key=lambda kv: (-kv[1], kv[0]))
        rows.append((g // REFLEN, g % REFLEN, depth[g], S[g], count, ln, len(at[g]), 0))
    return np.array(rows, np.int32).reshape(-1, 8)


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
tracked = al.pileup(R, G, deletions=True, **wkw)


def route_pileup(track):
    al.pileup(R, G, deletions=track, **wkw).close()


def route_host():
    out = al.align_windows(R, G, **wkw)
    return host_rule(host_records(out), [tracked.counts(r) for r in range(NREF)])


routes = {
    "(1) pileup()": lambda: route_pileup(False),
    "(2) pileup(deletions=True)": lambda: route_pileup(True),
    "(3) deletions(), every reference": lambda: tracked.deletions(G, min_depth=MIN_DEPTH, min_frac=PERMILLE / 1000),
    "(4) align_windows with CIGARs + records and rule on the host": route_host,
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
for what in ("pileup", "pileup deletion count", "pileup deletion scatter", "deletions count", "deletions reduce"):
    ms = err.ms(what)
    if ms:
        print(f"{what} kernel(s) alone, HIP events: median {med(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}; {len(ms)} launches)", flush=True)
t1, t2 = med(times["(1) pileup()"]), med(times["(2) pileup(deletions=True)"])
print(f"tracking costs (2) - (1) = {(t2 - t1) * 1e3:.2f} ms, (2) / (1) = {t2 / t1:.4f}; (3) / (4) = "
      f"{med(times['(3) deletions(), every reference']) / med(times['(4) align_windows with CIGARs + records and rule on the host']):.5f}", flush=True)
records, bases = tracked._pileup.deletion_stats()
print(f"the log: {records} records of {bases} deleted bases ({records * 16} bytes, and {4 * NREF * REFLEN} bytes of starts plane)", flush=True)
# the routes agree
s = tracked.deletions(G, min_depth=MIN_DEPTH, min_frac=PERMILLE / 1000)
dev_rows = np.stack([s[k] for k in tracked.DELETION_COLUMNS], axis=1)
host_rows = route_host()
print(f"device rows == host rows: {np.array_equal(dev_rows, host_rows)} ({len(dev_rows)} rows)", flush=True)
tracked.close()
R.close()
G.close()
al.close()
