"""Probe of the SAM fields (sam=True of align_windows).

Workload: that of tools/probes/left_align.py / pileup_index.py — 8 references of 1 Mb (fixed seed), 16 384 reads of 150 bp cut from them
at 2 %, every second one stored reverse-complemented; 1 M listed pairs against 300 bp windows.  In one process, medians of REPS after a
warm-up, with min and max:
 (1) align_windows(sam=True): rows and the two blobs come back, no op string
 (2) the route it replaces: align_windows with CIGARs (their run-length encoding comes back), the windows cut out of the references on
     the host, then the host rule (_native.ops_sam) over every pair — once; its fields are checked against (1)
and the HIP-event time of the two SAM passes beside the RLE kernel's route on the same batches (the run-length encoding's own two
launches are timed from the host around ResidentBatch.rle(), which is what (2) pays for its strings).
Run it under `timeout`.  Usage: sam_index.py [--pairs N] [--reps R]"""
import hashlib
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pywfa_amd import WavefrontAligner, _native  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
NPAIRS = int(sys.argv[sys.argv.index("--pairs") + 1]) if "--pairs" in sys.argv else 1 << 20
LUT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
READ, WIN, NREF, REFLEN = 150, 300, 8, 1 << 20


def source_hash():
    h = hashlib.sha256()
    for name in ("k_sam.hip", "wfa_sam.hpp", "api_sam.hip"):
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
print(f"k_sam.hip + wfa_sam.hpp + api_sam.hip sha256 {source_hash()}; medians of {REPS}", flush=True)


def med(x):
    return float(np.median(x))


KW = dict(span="ends-free", text_begin_free=READ, text_end_free=READ)
al = WavefrontAligner(scope="full", **KW)
R, G = al.sequence_set(reads), al.sequence_set(refs)
wkw = dict(i=i, j=j, text_start=t_start, text_len=np.full(n, WIN, np.int32), reverse=stored_rev[i])


def route_host():
    """align_windows with CIGARs, the windows cut on the host, wfa_hip_ops_sam over every finished pair: (pos, CIGAR, MD) per pair and
    the seconds of the three steps."""
    t0 = time.perf_counter()
    out = al.align_windows(R, G, **wkw)
    t1 = time.perf_counter()
    windows = [ref_bytes[j[q]][t_start[q]:t_start[q] + WIN] for q in range(n)]
    t2 = time.perf_counter()
    fields = [None] * n
    for q in np.flatnonzero(out["status"] == 0):
        row, cigar, md = _native.ops_sam(out["cigar_ops"][q], windows[q], READ)
        fields[q] = (int(row[0]) + int(t_start[q]) if row[0] >= 0 else -1, cigar, md)
    t3 = time.perf_counter()
    return fields, (t1 - t0, t2 - t1, t3 - t2)


def kernels():
    """One windowed batch of the whole list: the HIP-event time of the two SAM passes, and the host's time around the run-length
    encoding (two launches of the RLE kernel and its downloads) and around sam() (two launches, the scans and its downloads)."""
    rb = al._native.batch_windows(R._set, G._set, i, j, None, None, t_start, np.full(n, WIN, np.int32), stored_rev[i])
    try:
        rb.run()
        rb.sync()
        sam_ms, sam_wall, rle_wall = [], [], []
        for rep in range(REPS + 1):
            t0 = time.perf_counter()
            rb.sam()
            t1 = time.perf_counter()
            rb.rle()
            t2 = time.perf_counter()
            if rep:
                sam_ms.append(rb.sam_kernel_ms())
                sam_wall.append((t1 - t0) * 1e3)
                rle_wall.append((t2 - t1) * 1e3)
        return sam_ms, sam_wall, rle_wall
    finally:
        rb.close()


al.align_windows(R, G, sam=True, **wkw)   # warm-up
times = []
for rep in range(REPS):
    t0 = time.perf_counter()
    dev = al.align_windows(R, G, sam=True, **wkw)
    times.append(time.perf_counter() - t0)
print(f"(1) align_windows(sam=True): median {med(times) * 1e3:.2f} ms (min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}; {len(times)} runs)", flush=True)
fields, (t_align, t_cut, t_rule) = route_host()
print(f"(2) the host route, once: align_windows with CIGARs {t_align * 1e3:.2f} ms + windows cut on the host {t_cut * 1e3:.2f} ms + "
      f"ops_sam per pair {t_rule * 1e3:.2f} ms = {(t_align + t_cut + t_rule) * 1e3:.2f} ms", flush=True)
sam_ms, sam_wall, rle_wall = kernels()
print(f"the two SAM passes alone, HIP events: median {med(sam_ms):.4f} ms (min {min(sam_ms):.4f}, max {max(sam_ms):.4f}; {len(sam_ms)} runs)", flush=True)
print(f"ResidentBatch.sam() on the host's clock: median {med(sam_wall):.2f} ms; ResidentBatch.rle(): median {med(rle_wall):.2f} ms", flush=True)
# the routes agree
s = dev["sam"]
same = all(f is None and s["pos"][q] == -1 or f is not None and (int(s["pos"][q]), s["cigar"][q].encode(), s["md"][q].encode()) == f
           for q, f in enumerate(fields))
print(f"device fields == host fields: {same}; mapped pairs: {int((s['pos'] >= 0).sum())} of {n}", flush=True)
R.close()
G.close()
al.close()
