"""Probe of the placement of reads (WavefrontAligner.place_windows, wfa_hip_placer_*).

Workload: that of seed_index.py — 8 references of 1 Mb (fixed seed), 16 384 reads of 150 bp cut from random positions of them at 2 %,
every second one stored reverse-complemented; seeds(n=4) under the default parameters; gap-affine, ends-free with 10 free text bases
on either side, scope full.
(1) place_windows on the returned windows, from Python on open handles, medians of REPS.
(2) The route it replaces: align_windows(summary=True), then the same rule in NumPy (a lexsort by read), medians of REPS; the two
    routes' rows and flags are compared, exact equality.
(3) The placer's own part through the C ABI binding on one resident batch after its run: add (the record kernel, by wall clock) and
    run (count, scan, scatter and the place kernel, by HIP events: Placer.kernel_ms()), medians of REPS.
Usage: place_index.py [--reps N]"""
import hashlib
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pywfa_amd import WavefrontAligner  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
LUT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
READ, NREF, REFLEN = 150, 8, 1 << 20
INT32_MIN = -2**31
COLUMNS = ("hit", "score", "second", "mapq", "hits", "ties", "text_start", "text_end")


def copy_of(rng, f, div=0.02):
    """A copy of f (codes 0..3) with substitutions, deletions and insertions in equal parts at `div`, cut or padded to READ bases."""
    L = len(f)
    r = rng.random(L)
    sub = rng.integers(0, 4, L)
    first = np.where(r < div / 3, sub, f)
    cnt = np.where((r >= div / 3) & (r < 2 * div / 3), 0, np.where((r >= 2 * div / 3) & (r < div), 2, 1))
    vals = np.stack([first, sub], 1).ravel()
    keep = np.stack([cnt >= 1, cnt == 2], 1).ravel()
    out = vals[keep][:READ]
    return LUT[np.r_[out, sub[:READ - len(out)]]].tobytes()


def source_hash():
    h = hashlib.sha256()
    for name in ("k_place.hip", "wfa_place.hpp", "wfa_summary.hpp"):
        h.update(open(os.path.join(ROOT, "pywfa_amd", "csrc", name), "rb").read())
    return h.hexdigest()[:12]


def med(x):
    return float(np.median(x))


def numpy_place(nreads, i, j, rev, score, status, ts, te, min_score, full_gap):
    """The rule of include/wfa_hip.h ("placement") on host arrays: (rows, flags)."""
    n = len(i)
    rows = np.zeros((nreads, 8), np.int64)
    rows[:] = (-1, INT32_MIN, INT32_MIN, 0, 0, 0, 0, 0)
    flags = np.zeros(n, np.uint8)
    el = np.flatnonzero((status == 0) & (score >= min_score))
    if el.size == 0:
        return rows.astype(np.int32), flags
    order = el[np.lexsort((el, -score[el].astype(np.int64), i[el]))]       # by read, then score descending, then hit number
    ri = i[order]
    first = np.r_[True, ri[1:] != ri[:-1]]
    start = np.flatnonzero(first)
    p = order[start][np.cumsum(first) - 1]                                  # every eligible hit's primary
    ts64, te64 = ts.astype(np.int64), te.astype(np.int64)
    ov = np.minimum(te64[order], te64[p]) - np.maximum(ts64[order], ts64[p])
    same = (order != p) & (j[order] == j[p]) & (rev[order] == rev[p]) & (ov > 0) & (2 * ov >= np.minimum(te64[order] - ts64[order], te64[p] - ts64[p]))
    other = (order != p) & ~same
    flags[order] = np.where(order == p, 3, np.where(same, 2, 1))
    sc = score[order].astype(np.int64)
    second = np.maximum.reduceat(np.where(other, sc, np.int64(INT32_MIN) - 1), start)
    has = np.add.reduceat(other.astype(np.int64), start) > 0
    sp = score[order[start]].astype(np.int64)
    mapq = np.where(has, np.minimum(60, 60 * (sp - second) // full_gap), 60)
    r = ri[start]
    rows[r, 0] = order[start]
    rows[r, 1] = sp
    rows[r, 2] = np.where(has, second, INT32_MIN)
    rows[r, 3] = mapq
    rows[r, 4] = np.add.reduceat(np.ones(len(order), np.int64), start)
    rows[r, 5] = np.add.reduceat((other & (sc == score[p])).astype(np.int64), start)
    rows[r, 6] = ts[order[start]]
    rows[r, 7] = te[order[start]]
    return rows.astype(np.int32), flags


rng = np.random.default_rng(2027)
codes = [rng.integers(0, 4, REFLEN) for _ in range(NREF)]
refs = [LUT[c].tobytes().decode() for c in codes]
nreads = 16384
ref_of = rng.integers(0, NREF, nreads)
pos_of = rng.integers(200, REFLEN - 400, nreads)
stored_rev = (np.arange(nreads) % 2).astype(np.uint8)
reads = []
for q in range(nreads):
    s = copy_of(rng, codes[ref_of[q]][pos_of[q]:pos_of[q] + READ + 8])
    reads.append((s.translate(COMP)[::-1] if stored_rev[q] else s).decode())
print(f"{nreads} reads of {READ} bp, {NREF} references of {REFLEN} bp; k_place.hip + wfa_place.hpp + wfa_summary.hpp sha256 {source_hash()}", flush=True)

al = WavefrontAligner(span="ends-free", text_begin_free=10, text_end_free=10)
GAP = 24
with al.sequence_set(reads) as R, al.sequence_set(refs) as G:
    with al.seed_index(G) as idx:
        s = idx.seeds(R)
    keep = s["j"] >= 0
    i = np.nonzero(keep)[0].astype(np.int32)
    wins = dict(i=i, j=s["j"][keep], text_start=s["text_start"][keep], text_len=s["text_len"][keep], reverse=s["reverse"][keep].astype(np.uint8))
    print(f"{len(i)} windows of seeds(n=4); {int((np.bincount(i, minlength=nreads) > 1).sum())} reads with more than one", flush=True)

    res = al.place_windows(R, G, **wins)   # warm-up
    t_place = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        res = al.place_windows(R, G, **wins)
        t_place.append(time.perf_counter() - t0)
    rd = res["reads"]
    print(f"place_windows from Python on open handles: median {med(t_place) * 1e3:.2f} ms (min {min(t_place) * 1e3:.2f}, max "
          f"{max(t_place) * 1e3:.2f}); placed {int((rd['hit'] >= 0).sum())} reads, mapq 60: {int((rd['mapq'] == 60).sum())}, mapq 0 of the "
          f"placed: {int(((rd['mapq'] == 0) & (rd['hit'] >= 0)).sum())}, same-locus hits {int((res['flag'] == 2).sum())}", flush=True)
    right = (rd["hit"] >= 0) & (wins["j"][rd["hit"]] == ref_of) & (rd["text_start"] <= pos_of + 8) & (rd["text_end"] >= pos_of + READ - 8)
    print(f"primary at the true locus: {right.mean():.4f} of the reads", flush=True)

    al.align_windows(R, G, summary=True, **wins)   # warm-up
    t_host, t_rule = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        a = al.align_windows(R, G, summary=True, **wins)
        t1 = time.perf_counter()
        ts = wins["text_start"] + a["summary"]["locations"][:, 2]
        te = wins["text_start"] + a["summary"]["locations"][:, 3]
        rows, flags = numpy_place(nreads, wins["i"], wins["j"], wins["reverse"], a["score"], a["status"], ts, te, INT32_MIN, GAP)
        t2 = time.perf_counter()
        t_host.append(t2 - t0)
        t_rule.append(t2 - t1)
    same = np.array_equal(flags, res["flag"]) and all(np.array_equal(rows[:, c], rd[name]) for c, name in enumerate(COLUMNS))
    print(f"align_windows(summary=True) + the rule in NumPy: median {med(t_host) * 1e3:.2f} ms (min {min(t_host) * 1e3:.2f}, max "
          f"{max(t_host) * 1e3:.2f}), of which the NumPy rule {med(t_rule) * 1e3:.2f} ms; equal to place_windows: {same}; "
          f"place_windows / this route = {med(t_place) / med(t_host):.3f}", flush=True)

    nat = al._native
    rb = nat.batch_windows(R._set, G._set, wins["i"], wins["j"], None, None, wins["text_start"], wins["text_len"], wins["reverse"])
    rb.run()
    rb.sync()
    t_add, k_ms, t_run = [], [], []
    for _ in range(REPS + 1):
        pl = nat.placer(nreads)
        t0 = time.perf_counter()
        pl.add(rb, wins["i"], wins["j"], wins["text_start"], wins["reverse"])
        t1 = time.perf_counter()
        rows2, flags2 = pl.run(INT32_MIN, GAP)
        t2 = time.perf_counter()
        t_add.append(t1 - t0)
        t_run.append(t2 - t1)
        k_ms.append(pl.kernel_ms())
        pl.close()
    rb.close()
    t_add, k_ms, t_run = t_add[1:], k_ms[1:], t_run[1:]
    print(f"placer alone on {len(i)} hits: add (upload + record kernel, wall clock) median {med(t_add) * 1e3:.3f} ms; run kernels "
          f"(count, scan, scatter, place; HIP events) median {med(k_ms):.4f} ms (min {min(k_ms):.4f}, max {max(k_ms):.4f}); run from "
          f"Python median {med(t_run) * 1e3:.3f} ms; equal to place_windows: {np.array_equal(flags2, res['flag'])}", flush=True)
al.close()
