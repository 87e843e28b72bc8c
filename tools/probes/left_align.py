"""Probe of left alignment (left_align=True of pileup / align_windows).

Workload: that of tools/probes/pileup_index.py / pileup_insertions.py — 8 references of 1 Mb (fixed seed), 16 384 reads of 150 bp cut
from them at 2 %, every second one stored reverse-complemented; 1 M listed pairs against 300 bp windows.  In one process, medians of
REPS after a warm-up, with min and max:
 (1) pileup()          (2) pileup(left_align=True)          — (2) - (1) is the cost of the rewrite
 (3) the route (2) replaces: align_windows with CIGARs (their run-length encoding comes back), then the host function over every pair,
     then a NumPy pileup — its table is checked against (2)
and the HIP-event times of the left-alignment kernel beside the pileup kernel's on the same batches (WFA_HIP_REDUCE_TIMING=1 makes the
library print them).
Run it under `timeout`.  Usage: left_align.py [--pairs N] [--reps R]"""
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

from pywfa_amd import WavefrontAligner, _native  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
NPAIRS = int(sys.argv[sys.argv.index("--pairs") + 1]) if "--pairs" in sys.argv else 1 << 20
LUT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
READ, WIN, NREF, REFLEN = 150, 300, 8, 1 << 20


def source_hash():
    h = hashlib.sha256()
    for name in ("k_leftalign.hip", "wfa_leftalign.hpp", "k_pileup.hip"):
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
ref_bytes = [LUT[c].tobytes() for c in codes]
nreads = 16384
ref_of = rng.integers(0, NREF, nreads)
pos_of = rng.integers(200, REFLEN - 400, nreads)
stored_rev = (np.arange(nreads) % 2).astype(np.uint8)
reads, forward = [], []
for k in range(nreads):
    s = LUT[copy_of(rng, codes[ref_of[k]][pos_of[k]:pos_of[k] + READ + 8])].tobytes()
    forward.append(s)                         # on the references' strand: the batch's pattern of a reversed window
    reads.append((s.translate(COMP)[::-1] if stored_rev[k] else s).decode())
i = np.repeat(np.arange(nreads), 64)
t_start = np.repeat(pos_of, 64) - 75 + np.tile(np.arange(-32, 32), nreads)
order = rng.permutation(len(i))[:NPAIRS]
i, t_start = i[order].astype(np.int32), t_start[order].astype(np.int32)
j = ref_of[i].astype(np.int32)
n = len(i)
print(f"{nreads} reads of {READ} bp, {NREF} references of {REFLEN} bp, {n} listed pairs against {WIN} bp windows", flush=True)
print(f"k_leftalign.hip + wfa_leftalign.hpp + k_pileup.hip sha256 {source_hash()}; medians of {REPS}", flush=True)


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
COL = np.full(256, 4, np.int64)
COL[list(b"ACGT")] = np.arange(4)


def route_host():
    """align_windows with CIGARs, wfa_hip_ops_left_align over every finished pair, the pileup rule in NumPy per pair."""
    out = al.align_windows(R, G, **wkw)
    table = np.zeros((NREF * REFLEN, 8), np.int32)
    moved = 0
    for q in np.flatnonzero(out["status"] == 0):
        ops = out["cigar_ops"][q]
        P = np.frombuffer(forward[i[q]], np.uint8)
        T = np.frombuffer(ref_bytes[j[q]], np.uint8)[t_start[q]:t_start[q] + WIN]
        ops, m, _ = _native.ops_left_align(ops, P, T)
        moved += m
        is_m = np.flatnonzero(ops == ord("M"))
        if not len(is_m):
            continue
        first, last = is_m[0], is_m[-1]
        on_v = (ops != ord("I")).astype(np.int64)
        on_h = (ops != ord("D")).astype(np.int64)
        v, h = np.cumsum(on_v) - on_v, np.cumsum(on_h) - on_h
        core = np.zeros(len(ops), bool)
        core[first:last + 1] = True
        row = j[q].astype(np.int64) * REFLEN + t_start[q] + h
        mx = core & ((ops == ord("M")) | (ops == ord("X")))
        np.add.at(table, (row[mx], COL[P[v[mx]]]), 1)
        np.add.at(table, (row[core & (ops == ord("X"))], 7), 1)
        np.add.at(table, (row[core & (ops == ord("I"))], 5), 1)
        d_start = core & (ops == ord("D")) & np.r_[True, ops[:-1] != ord("D")]
        np.add.at(table, (row[d_start], 6), 1)
    return table, moved


routes = {
    "(1) pileup()": lambda: al.pileup(R, G, **wkw).close(),
    "(2) pileup(left_align=True)": lambda: al.pileup(R, G, left_align=True, **wkw).close(),
    "(3) align_windows with CIGARs + the host function + a NumPy pileup": route_host,
}
times = {name: [] for name in routes}
with Stderr() as err:
    for name, fn in routes.items():
        if not name.startswith("(3)"):
            fn()                                            # warm-up
    for rep in range(REPS):
        for name, fn in routes.items():
            if name.startswith("(3)") and rep > 0:
                continue                                    # (a Python loop over every pair: once)
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
for name, t in times.items():
    print(f"{name}: median {med(t) * 1e3:.2f} ms (min {min(t) * 1e3:.2f}, max {max(t) * 1e3:.2f}; {len(t)} runs)", flush=True)
for what in ("left align", "pileup"):
    ms = err.ms(what)
    if ms:
        print(f"{what} kernel(s) alone, HIP events: median {med(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}; {len(ms)} launches)", flush=True)
t1, t2 = med(times["(1) pileup()"]), med(times["(2) pileup(left_align=True)"])
print(f"the rewrite costs (2) - (1) = {(t2 - t1) * 1e3:.2f} ms, (2) / (1) = {t2 / t1:.4f}", flush=True)
# the routes agree
host_table, moved = route_host()
with al.pileup(R, G, left_align=True, **wkw) as p:
    same = all(np.array_equal(p.counts(r), host_table[r * REFLEN:(r + 1) * REFLEN]) for r in range(NREF))
print(f"device table == host table: {same}; runs moved on the host route: {moved}", flush=True)
R.close()
G.close()
al.close()
