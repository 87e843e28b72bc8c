"""Probe of the windowed batches (WavefrontAligner.align_windows, wfa_hip_batch_create_windows).

Workload: 8 references of 1 Mb (fixed seed), 16 384 reads of 150 bp cut from random positions of them at 2 %, every second one stored
reverse-complemented; 1 M listed pairs: every read against 64 windows of 300 bp of its reference around its locus (the locus 43 - 107
bases into the window), shuffled; gap-affine, ends-free with the text's ends free (150 each), scope score and scope full.
(1) Kernel time, same pairs: last_kernel() of the windowed batch against last_kernel() of an explicit resident batch holding the
    materialised pairs in the same order; the two alternate in one process, medians of REPS runs, the explicit batch's own spread.
(2) The generators' own times come from a separate run under the kernel tracer:
        rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o windows -- python3 tools/probes/windows_index.py --once
    (--once: score only, no repeats; in this order ONE indexed batch over whole sequences of the same lengths (150 bp patterns, 300 bp
    texts: wfa_pairs_gen_kernel), ONE windowed batch of the list with every pair forward and ONE with the list's strands
    (wfa_windows_gen_kernel, twice), so the trace holds exactly those three generator dispatches.)
(3) End to end from Python, on open handles: align_windows against cutting and reverse-complementing the strings on the host and
    calling wavefront_align_batch (the cutting is timed: it is what the caller does today); alternated, medians of REPS; and the
    bytes per pair each route sends over PCIe.
Usage: windows_index.py [--once] [--pairs N]"""
import hashlib
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pywfa_amd import WavefrontAligner, datagen  # noqa: E402

ONCE = "--once" in sys.argv
REPS = 1 if ONCE else 5
NPAIRS = int(sys.argv[sys.argv.index("--pairs") + 1]) if "--pairs" in sys.argv else 1 << 20
LUT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
READ, WIN, NREF, REFLEN = 150, 300, 8, 1 << 20


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


def revcomp(b):
    return b.translate(COMP)[::-1]


def source_hash():
    h = hashlib.sha256()
    for name in ("k_windows.hip", "wfa_cross.hpp"):
        h.update(open(os.path.join(ROOT, "pywfa_amd", "csrc", name), "rb").read())
    return h.hexdigest()[:12]


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
    reads.append((revcomp(s) if stored_rev[k] else s).decode())
i = np.repeat(np.arange(nreads), 64)
t_start = np.repeat(pos_of, 64) - 75 + np.tile(np.arange(-32, 32), nreads)
order = rng.permutation(len(i))[:NPAIRS]
i, t_start = i[order].astype(np.int32), t_start[order].astype(np.int32)
j = ref_of[i].astype(np.int32)
t_len = np.full(len(i), WIN, np.int32)
reverse = stored_rev[i]
n = len(i)
print(f"{nreads} reads of {READ} bp, {NREF} references of {REFLEN} bp, {n} listed pairs against {WIN} bp windows, {reverse.mean():.2f} reversed; "
      f"k_windows.hip + wfa_cross.hpp sha256 {source_hash()}", flush=True)


def cut_strings():
    """What the caller does without align_windows: every window as a Python string, the reversed reads complemented."""
    fwd = [revcomp(r.encode()).decode() for r in reads]
    pats = [fwd[a] if rv else reads[a] for a, rv in zip(i, reverse)]
    texts = [refs[b][s:s + WIN] for b, s in zip(j, t_start)]
    return pats, texts


def med(x):
    return float(np.median(x))


KW = dict(span="ends-free", text_begin_free=READ, text_end_free=READ)
slot_words = (READ + 15) // 16 + (WIN + 15) // 16
print(f"PCIe bytes per pair: align_windows {4 * 4 + 1} (i, j, text_start, text_len, reverse); wavefront_align_batch "
      f"{4 * slot_words + 4} host-packed (2-bit words and two 16-bit lengths; {READ + WIN} as bytes in a small batch)", flush=True)

if ONCE:
    al = WavefrontAligner(scope="score", **KW)
    whole = [refs[b][s:s + WIN] for b, s in zip(ref_of, pos_of - 75)]     # 16 384 whole sequences of the windows' length
    R, T, G = al.sequence_set(reads), al.sequence_set(whole), al.sequence_set(refs)
    jw = rng.integers(0, nreads, n).astype(np.int32)
    for make in (lambda: al._native.batch_indexed(R._set, T._set, i, jw),
                 lambda: al._native.batch_windows(R._set, G._set, i, j, None, None, t_start, t_len, None),
                 lambda: al._native.batch_windows(R._set, G._set, i, j, None, None, t_start, t_len, reverse)):
        rb = make()
        rb.close()
    for S in (R, T, G):
        S.close()
    al.close()
    sys.exit(0)

pats, texts = cut_strings()
explicit = datagen.from_strings(pats, texts, upper=True)
for scope in ("score", "full"):
    al = WavefrontAligner(scope=scope, **KW)
    al.align_windows(reads[:64], refs[:1], i=np.arange(64), j=np.zeros(64, np.int32), text_start=np.arange(64), text_len=np.full(64, WIN))
    al.wavefront_align_batch(texts[:2048], patterns=pats[:2048])   # (warm-up: first-run allocations, run-time kernels)
    # (1) kernel time, same pairs
    R, G = al.sequence_set(reads), al.sequence_set(refs)
    rb_w = al._native.batch_windows(R._set, G._set, i, j, None, None, t_start, t_len, reverse)
    rb_e = al.resident_batch(explicit)
    for rb in (rb_w, rb_e):   # warm-up
        rb.run()
        rb.sync()
    ms_w, ms_e = [], []
    for _ in range(REPS):
        for rb, ms in ((rb_e, ms_e), (rb_w, ms_w)):
            rb.run()
            rb.sync()
            ms.append(rb.last_kernel()[0])
    same = np.array_equal(rb_w.results(False)[0], rb_e.results(False)[0])
    rb_w.close()
    rb_e.close()
    print(f"[{scope}] kernel ms, {n} pairs: windowed median {med(ms_w):.3f} (min {min(ms_w):.3f}, max {max(ms_w):.3f}); explicit median "
          f"{med(ms_e):.3f} (min {min(ms_e):.3f}, max {max(ms_e):.3f}, spread {max(ms_e) - min(ms_e):.3f}); ratio "
          f"{med(ms_w) / med(ms_e):.4f}; difference of medians {med(ms_w) - med(ms_e):+.3f} ms; same scores: {same}", flush=True)
    # (3) end to end from Python, on open handles
    t_win, t_host, t_cut = [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        p2, t2 = cut_strings()
        t_cut.append(time.perf_counter() - t0)
        al.wavefront_align_batch(t2, patterns=p2)
        t_host.append(time.perf_counter() - t0)
        del p2, t2
        t0 = time.perf_counter()
        al.align_windows(R, G, i=i, j=j, text_start=t_start, text_len=t_len, reverse=reverse)
        t_win.append(time.perf_counter() - t0)
    R.close()
    G.close()
    print(f"[{scope}] end to end ms: align_windows on open handles median {med(t_win) * 1e3:.1f} (min {min(t_win) * 1e3:.1f}, max "
          f"{max(t_win) * 1e3:.1f}); strings cut on the host + wavefront_align_batch median {med(t_host) * 1e3:.1f} (min "
          f"{min(t_host) * 1e3:.1f}, max {max(t_host) * 1e3:.1f}, spread {(max(t_host) - min(t_host)) * 1e3:.1f}), of which cutting "
          f"the strings median {med(t_cut) * 1e3:.1f}", flush=True)
    al.close()
