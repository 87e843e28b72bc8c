"""Probe of the pairing of reads (WavefrontAligner.place_pairs, wfa_hip_placer_run_pairs).

Workload: 8 references of 1 Mb (fixed seed), 8 192 fragments of two 150 bp mates cut 300 - 600 bases apart (outer distance) from random
positions of them at 2 %, the right-hand mate stored reverse-complemented, every second fragment from the other strand; seeds(n=4)
under the default parameters; gap-affine, ends-free with 10 free text bases on either side, scope full.
(1) place_pairs on the returned windows, from Python on open handles, medians of REPS.
(2) The route it replaces: align_windows(summary=True), then the placement and pairing rules in NumPy (a lexsort by read, a cross join
    per fragment), medians of REPS; the two routes' pair rows and pair flags are compared, exact equality.
(3) The placer's own part through the C ABI binding on one resident batch after its run: run_pairs (count, scan, scatter, place and
    the pair kernel, by HIP events: Placer.kernel_ms()) beside run (the same without the pair kernel), medians of REPS.
Usage: pair_index.py [--reps N]"""
import hashlib
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
LUT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
READ, NREF, REFLEN = 150, 8, 1 << 20
PAIR_COLUMNS = ("hit1", "hit2", "proper", "score", "second", "mapq", "mapq1", "mapq2", "insert", "pairings", "ties", "overflow")


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


def numpy_pair(rows, flags, mates, i, j, rev, score, status, ts, te, min_score, full_gap, min_insert, max_insert, unpaired):
    """The rule of include/wfa_hip.h ("pairing") on host arrays, given the single-end rows and flags: (pair_rows, pair_flags).
    `mates`: int64 (F, 2).  Fragments over the cap of 65 536 pairings are marked and left out of the join."""
    F = len(mates)
    se1, se2 = rows[mates[:, 0]].astype(np.int64), rows[mates[:, 1]].astype(np.int64)
    out = np.zeros((F, 12), np.int64)
    out[:, 0], out[:, 1], out[:, 3], out[:, 4], out[:, 6], out[:, 7] = se1[:, 0], se2[:, 0], INT32_MIN, INT32_MIN, se1[:, 3], se2[:, 3]
    pair_flags = flags.copy()
    el = np.flatnonzero((status == 0) & (score >= min_score))
    order = el[np.argsort(i[el], kind="stable")]                 # eligible hits by read, ascending hit number within a read
    begin = np.searchsorted(i[order], np.arange(len(rows) + 1))
    e1, e2 = se1[:, 4], se2[:, 4]
    out[:, 11] = e1 * e2 > 65536
    cells = np.where(out[:, 11] == 1, 0, e1 * e2)
    total = int(cells.sum())
    if total == 0:
        return out.astype(np.int32), pair_flags
    fr = np.repeat(np.arange(F), cells)
    k = np.arange(total) - np.repeat(np.cumsum(cells) - cells, cells)
    h = order[begin[mates[fr, 0]] + k // e2[fr]]
    g = order[begin[mates[fr, 1]] + k % e2[fr]]
    ts64, te64, sc = ts.astype(np.int64), te.astype(np.int64), score.astype(np.int64)
    fwd_h = rev[h] == 0
    tsF, teF = np.where(fwd_h, ts64[h], ts64[g]), np.where(fwd_h, te64[h], te64[g])
    tsR, teR = np.where(fwd_h, ts64[g], ts64[h]), np.where(fwd_h, te64[g], te64[h])
    ins = teR - tsF
    ok = ((j[h] == j[g]) & (rev[h] != rev[g]) & (te64[h] > ts64[h]) & (te64[g] > ts64[g]) & (tsF <= tsR) & (teF <= teR)
          & (ins >= min_insert) & (ins <= max_insert))
    fr, h, g, ins = fr[ok], h[ok], g[ok], ins[ok]
    ps = sc[h] + sc[g]
    out[:, 9] = np.bincount(fr, minlength=F)
    if len(fr) == 0:
        return out.astype(np.int32), pair_flags
    by = np.lexsort((g, h, -ps, fr))
    fr, h, g, ins, ps = fr[by], h[by], g[by], ins[by], ps[by]
    first = np.r_[True, fr[1:] != fr[:-1]]
    start = np.flatnonzero(first)
    lead = start[np.cumsum(first) - 1]                           # every proper pairing's best one
    good = ps[lead] + unpaired >= se1[fr, 1] + se2[fr, 1]

    def at(x, c):                                                # x == c, or x at c's locus
        ov = np.minimum(te64[x], te64[c]) - np.maximum(ts64[x], ts64[c])
        return (x == c) | ((j[x] == j[c]) & (rev[x] == rev[c]) & (ov > 0) & (2 * ov >= np.minimum(te64[x] - ts64[x], te64[c] - ts64[c])))

    other = good & ~(at(h, h[lead]) & at(g, g[lead]))
    second = np.maximum.reduceat(np.where(other, ps, -2**40), start)
    has = np.add.reduceat(other.astype(np.int64), start) > 0
    ties = np.add.reduceat((other & (ps == ps[lead])).astype(np.int64), start)
    f, best, proper = fr[start], ps[start], good[start]
    mapq = np.where(has, np.minimum(60, 60 * (best - second) // full_gap), 60)
    f, ch, cg = f[proper], h[start][proper], g[start][proper]
    mapq, best, second, has, ties = mapq[proper], best[proper], second[proper], has[proper], ties[proper]
    out[f, 0], out[f, 1], out[f, 2], out[f, 3] = ch, cg, 1, np.clip(best, INT32_MIN + 1, INT32_MAX)
    out[f, 4] = np.where(has, np.clip(second, INT32_MIN + 1, INT32_MAX), INT32_MIN)
    out[f, 5] = mapq
    out[f, 6] = np.where(flags[ch] >= 2, np.maximum(mapq, se1[f, 3]), mapq)
    out[f, 7] = np.where(flags[cg] >= 2, np.maximum(mapq, se2[f, 3]), mapq)
    out[f, 8], out[f, 10] = ins[start][proper], ties
    for side, chosen in ((0, ch), (1, cg)):                      # the flags of the two groups of every proper fragment
        r = mates[f, side]
        n = begin[r + 1] - begin[r]
        x = order[np.repeat(begin[r], n) + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)]
        c = np.repeat(chosen, n)
        pair_flags[x] = np.where(x == c, 3, np.where(at(x, c), 2, 1))
    return out.astype(np.int32), pair_flags


def main():
    from pywfa_amd import WavefrontAligner

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    h = hashlib.sha256()
    for name in ("k_place.hip", "wfa_place.hpp", "wfa_summary.hpp"):
        h.update(open(os.path.join(ROOT, "pywfa_amd", "csrc", name), "rb").read())
    rng = np.random.default_rng(2028)
    codes = [rng.integers(0, 4, REFLEN) for _ in range(NREF)]
    refs = [LUT[c].tobytes().decode() for c in codes]
    nfrag = 8192
    reads = []
    for f in range(nfrag):
        r, outer = int(rng.integers(0, NREF)), int(rng.integers(300, 601))
        left = int(rng.integers(200, REFLEN - 1000))
        mates = [copy_of(rng, codes[r][left:left + READ + 8]), copy_of(rng, codes[r][left + outer - READ:left + outer + 8]).translate(COMP)[::-1]]
        reads += [m.decode() for m in (mates[::-1] if f % 2 else mates)]
    print(f"{nfrag} fragments of two {READ} bp mates, {NREF} references of {REFLEN} bp; k_place.hip + wfa_place.hpp + wfa_summary.hpp sha256 "
          f"{h.hexdigest()[:12]}", flush=True)
    al = WavefrontAligner(span="ends-free", text_begin_free=10, text_end_free=10)
    GAP, PAR = 24, dict(min_insert=0, max_insert=1000)
    with al.sequence_set(reads) as R, al.sequence_set(refs) as G:
        with al.seed_index(G) as idx:
            s = idx.seeds(R)
        keep = s["j"] >= 0
        i = np.nonzero(keep)[0].astype(np.int32)
        wins = dict(i=i, j=s["j"][keep], text_start=s["text_start"][keep], text_len=s["text_len"][keep], reverse=s["reverse"][keep].astype(np.uint8))
        print(f"{len(i)} windows of seeds(n=4)", flush=True)
        res = al.place_pairs(R, G, **PAR, **wins)   # warm-up
        t_pair = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res = al.place_pairs(R, G, **PAR, **wins)
            t_pair.append(time.perf_counter() - t0)
        pr = res["pairs"]
        print(f"place_pairs from Python on open handles: median {med(t_pair) * 1e3:.2f} ms (min {min(t_pair) * 1e3:.2f}, max "
              f"{max(t_pair) * 1e3:.2f}); proper {int(pr['proper'].sum())} of {nfrag}, mapq 60: {int((pr['mapq'] == 60).sum())}, overflow "
              f"{int(pr['overflow'].sum())}, flags changed by the pairing: {int((res['pair_flag'] != res['flag']).sum())}", flush=True)
        al.align_windows(R, G, summary=True, **wins)   # warm-up
        mates = np.arange(2 * nfrag, dtype=np.int64).reshape(-1, 2)
        t_host, t_rule = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            a = al.align_windows(R, G, summary=True, **wins)
            t1 = time.perf_counter()
            ts = wins["text_start"] + a["summary"]["locations"][:, 2]
            te = wins["text_start"] + a["summary"]["locations"][:, 3]
            rows, flags = numpy_place(2 * nfrag, wins["i"], wins["j"], wins["reverse"], a["score"], a["status"], ts, te, INT32_MIN, GAP)
            prow, pflag = numpy_pair(rows, flags, mates, wins["i"], wins["j"], wins["reverse"], a["score"], a["status"], ts, te, INT32_MIN,
                                     GAP, PAR["min_insert"], PAR["max_insert"], GAP)
            t2 = time.perf_counter()
            t_host.append(t2 - t0)
            t_rule.append(t2 - t1)
        same = np.array_equal(pflag, res["pair_flag"]) and all(np.array_equal(prow[:, c], pr[name]) for c, name in enumerate(PAIR_COLUMNS))
        print(f"align_windows(summary=True) + the two rules in NumPy: median {med(t_host) * 1e3:.2f} ms (min {min(t_host) * 1e3:.2f}, max "
              f"{max(t_host) * 1e3:.2f}), of which the NumPy rules {med(t_rule) * 1e3:.2f} ms; equal to place_pairs: {same}; "
              f"place_pairs / this route = {med(t_pair) / med(t_host):.3f}", flush=True)
        nat = al._native
        rb = nat.batch_windows(R._set, G._set, wins["i"], wins["j"], None, None, wins["text_start"], wins["text_len"], wins["reverse"])
        rb.run()
        rb.sync()
        k_run, k_pairs, t_pairs = [], [], []
        for _ in range(reps + 1):
            pl = nat.placer(2 * nfrag)
            pl.add(rb, wins["i"], wins["j"], wins["text_start"], wins["reverse"])
            pl.run(INT32_MIN, GAP)
            k_run.append(pl.kernel_ms())
            pl.clear()
            pl.add(rb, wins["i"], wins["j"], wins["text_start"], wins["reverse"])
            t0 = time.perf_counter()
            out = pl.run_pairs(nfrag, INT32_MIN, GAP, PAR["min_insert"], PAR["max_insert"], GAP)
            t_pairs.append(time.perf_counter() - t0)
            k_pairs.append(pl.kernel_ms())
            pl.close()
        rb.close()
        k_run, k_pairs, t_pairs = k_run[1:], k_pairs[1:], t_pairs[1:]
        print(f"placer alone on {len(i)} hits: run kernels (count, scan, scatter, place; HIP events) median {med(k_run):.4f} ms; run_pairs "
              f"kernels (the same and the flag copy and the pair kernel) median {med(k_pairs):.4f} ms (min {min(k_pairs):.4f}, max "
              f"{max(k_pairs):.4f}); run_pairs from Python median {med(t_pairs) * 1e3:.3f} ms; equal to place_pairs: "
              f"{np.array_equal(out[3], res['pair_flag'])}", flush=True)
    al.close()


if __name__ == "__main__":
    main()
