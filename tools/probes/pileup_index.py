"""Probe of the two op-string reductions (align_windows(summary=True), WavefrontAligner.pileup).

Workload: the list of tools/probes/windows_index.py — 8 references of 1 Mb (fixed seed), 16 384 reads of 150 bp cut from them at 2 %,
every second one stored reverse-complemented; 1 M listed pairs, every read against 64 windows of 300 bp around its locus, shuffled;
gap-affine, ends-free with the text's ends free.  On open handles, in one process, medians of REPS after a warm-up:
 (1) align_windows, scope score                      (2) align_windows, scope full: today's route, the RLE of 1 M op strings comes back
 (3) align_windows(summary=True)                     (4) pileup()
 (5) route (2) plus a NumPy pileup built on the host from its run-length encoding (the columns of `Pileup`; checked against (4))
and the HIP-event times of the summary and pileup kernels alone (WFA_HIP_REDUCE_TIMING=1 makes the library print them).
Run it under `timeout`.  Usage: pileup_index.py [--pairs N] [--reps R]"""
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


def revcomp(b):
    return b.translate(COMP)[::-1]


rng = np.random.default_rng(2027)
codes = [rng.integers(0, 4, REFLEN) for _ in range(NREF)]
refs = [LUT[c].tobytes().decode() for c in codes]
nreads = 16384
ref_of = rng.integers(0, NREF, nreads)
pos_of = rng.integers(200, REFLEN - 400, nreads)
stored_rev = (np.arange(nreads) % 2).astype(np.uint8)
reads, fwd = [], []
for k in range(nreads):
    s = copy_of(rng, codes[ref_of[k]][pos_of[k]:pos_of[k] + READ + 8])
    fwd.append(s)
    reads.append((revcomp(s) if stored_rev[k] else s).decode())
i = np.repeat(np.arange(nreads), 64)
t_start = np.repeat(pos_of, 64) - 75 + np.tile(np.arange(-32, 32), nreads)
order = rng.permutation(len(i))[:NPAIRS]
i, t_start = i[order].astype(np.int32), t_start[order].astype(np.int32)
j = ref_of[i].astype(np.int32)
t_len = np.full(len(i), WIN, np.int32)
reverse = stored_rev[i]
n = len(i)
COL = np.full(256, 4, np.int64)
COL[[65, 67, 71, 84]] = [0, 1, 2, 3]
read_cols = COL[np.frombuffer(b"".join(fwd), np.uint8)].reshape(nreads, READ)   # the reads on the references' strand
print(f"{nreads} reads of {READ} bp, {NREF} references of {REFLEN} bp, {n} listed pairs against {WIN} bp windows, {reverse.mean():.2f} reversed",
      flush=True)


def host_pileup(out):
    """The table of `Pileup` from the run-length encoding align_windows returns, in NumPy, 64 k pairs at a time."""
    seq = out["cigar_ops"]
    off, code, rlen = seq._off, seq._code.astype(np.int64), seq._len.astype(np.int64)
    table = np.zeros((NREF * REFLEN, 8), np.int32).reshape(-1)
    ok = np.flatnonzero(out["status"] == 0)
    for lo in range(0, len(ok), 1 << 16):
        q = ok[lo:lo + (1 << 16)]
        cnt = (off[q + 1] - off[q])
        pair = np.repeat(np.arange(len(q)), cnt)                 # the chunk's runs: their pair, code, length
        ridx = np.repeat(off[q], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        c, ln = code[ridx], rlen[ridx]
        first = np.r_[0, np.cumsum(cnt)[:-1]]
        h = np.cumsum(np.where((c == 0) | (c == 1) | (c == 8), ln, 0))
        v = np.cumsum(np.where((c == 0) | (c == 2) | (c == 8), ln, 0))
        h0 = h - np.where((c == 0) | (c == 1) | (c == 8), ln, 0)
        v0 = v - np.where((c == 0) | (c == 2) | (c == 8), ln, 0)
        h0 -= np.repeat(h0[first], cnt)
        v0 -= np.repeat(v0[first], cnt)
        k = np.arange(len(c))
        is_m = c == 0
        fm = np.full(len(q), len(c), np.int64)
        np.minimum.at(fm, pair[is_m], k[is_m])
        lm = np.full(len(q), -1, np.int64)
        np.maximum.at(lm, pair[is_m], k[is_m])
        core = (k >= fm[pair]) & (k <= lm[pair])
        base = (j[q].astype(np.int64) * REFLEN + t_start[q])[pair] + h0      # the run's first row
        for sel, col in (((c == 1) & core, 5),):
            rows = np.repeat(base[sel], ln[sel]) + (np.arange(ln[sel].sum()) - np.repeat(np.cumsum(ln[sel]) - ln[sel], ln[sel]))
            np.add.at(table, rows * 8 + col, 1)
        np.add.at(table, base[(c == 2) & core] * 8 + 6, 1)
        sel = ((c == 0) | (c == 8)) & core
        within = np.arange(ln[sel].sum()) - np.repeat(np.cumsum(ln[sel]) - ln[sel], ln[sel])
        rows = np.repeat(base[sel], ln[sel]) + within
        letter = read_cols[np.repeat(i[q][pair[sel]], ln[sel]), np.repeat(v0[sel], ln[sel]) + within]
        np.add.at(table, rows * 8 + letter, 1)
        isx = np.repeat(c[sel] == 8, ln[sel])
        np.add.at(table, rows[isx] * 8 + 7, 1)
    return table.reshape(-1, 8)


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
wkw = dict(i=i, j=j, text_start=t_start, text_len=t_len, reverse=reverse)
score_al, full_al = WavefrontAligner(scope="score", **KW), WavefrontAligner(scope="full", **KW)
sets = {al: (al.sequence_set(reads), al.sequence_set(refs)) for al in (score_al, full_al)}
RS, GS = sets[score_al]
RF, GF = sets[full_al]
routes = {
    "(1) align_windows score": lambda: score_al.align_windows(RS, GS, **wkw),
    "(2) align_windows full (RLE)": lambda: full_al.align_windows(RF, GF, **wkw),
    "(3) align_windows summary=True": lambda: full_al.align_windows(RF, GF, summary=True, **wkw),
    "(4) pileup()": lambda: full_al.pileup(RF, GF, **wkw).close(),
    "(5) (2) + NumPy pileup on the host": lambda: host_pileup(full_al.align_windows(RF, GF, **wkw)),
}
times = {name: [] for name in routes}
with Stderr() as err:
    for name, fn in routes.items():
        if not name.startswith("(5)"):
            fn()                                            # warm-up: first-run allocations, pilots
    for _ in range(REPS):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
for name, t in times.items():
    print(f"{name}: median {med(t) * 1e3:.1f} ms (min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f}; {len(t)} runs)", flush=True)
for what in ("summary", "pileup"):
    ms = err.ms(what)
    print(f"{what} kernel alone, HIP events: median {med(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}; {len(ms)} launches of {n} pairs)", flush=True)
print(f"(3) / (2) = {med(times['(3) align_windows summary=True']) / med(times['(2) align_windows full (RLE)']):.3f}; "
      f"(4) / (5) = {med(times['(4) pileup()']) / med(times['(5) (2) + NumPy pileup on the host']):.4f}", flush=True)
# the two pileups agree
with full_al.pileup(RF, GF, **wkw) as p:
    dev = np.concatenate([p.counts(r) for r in range(NREF)])
host = host_pileup(full_al.align_windows(RF, GF, **wkw))
print(f"device pileup == host pileup: {np.array_equal(dev, host)}; counts {dev.sum(axis=0).tolist()}; mean depth {dev[:, :6].sum() / len(dev):.2f}", flush=True)
for al in (score_al, full_al):
    for s in sets[al]:
        s.close()
    al.close()
