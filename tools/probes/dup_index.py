"""Probe of duplicate marking (WavefrontAligner.place_pairs(duplicates=True), wfa_hip_placer_duplicates).

Workload: that of pair_index.py — 8 references of 1 Mb (fixed seed), 8 192 fragments of two 150 bp mates cut 300 - 600 bases apart at
2 %, seeds(n=4) under the default parameters, gap-affine, ends-free with 10 free text bases on either side, scope full — with every
eighth fragment a copy of another: the same place, its own errors.
(1) place_pairs(duplicates=True) against place_pairs(), from Python on open handles, medians of REPS.
(2) The kernels by HIP events through the C ABI binding on one resident batch after its run: Placer.duplicates (group, place, pair,
    key, scan, scatter, resolve) beside Placer.run_pairs (the same without the last four), medians of REPS.
(3) The route it replaces: align_windows(summary=True), the placement and pairing rules in NumPy (pair_index.py) and the duplicate
    rule as a lexsort over the keys, medians of REPS; the two routes' rows are compared, exact equality.
Usage: dup_index.py [--reps N]"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), HERE]
import numpy as np  # noqa: E402

from pair_index import COMP, INT32_MIN, LUT, NREF, READ, REFLEN, copy_of, med, numpy_pair, numpy_place  # noqa: E402

MAX_BUCKET = 4096


def numpy_duplicates(rows, prow, mates, j, rev, ts, te):
    """The rule of include/wfa_hip.h ("duplicates") on host arrays, given the single-end rows and the pair rows: (read_rows,
    pair_rows).  Every b is taken to lie inside its text (the hits come from alignments)."""
    nreads, F = len(rows), len(mates)
    read_rows = np.zeros((nreads, 4), np.int64)
    read_rows[:, 0] = -1
    pair_rows = np.zeros((F, 4), np.int64)
    pair_rows[:, 0] = -1
    pf = np.flatnonzero(prow[:, 2] == 1)
    h, g = prow[pf, 0], prow[pf, 1]
    h_fwd = rev[h] == 0
    Fh, Rh = np.where(h_fwd, h, g), np.where(h_fwd, g, h)
    owned = np.zeros(nreads, bool)
    owned[mates[pf].ravel()] = True
    rr = np.flatnonzero(~owned & (rows[:, 0] >= 0) & (rows[:, 7] > rows[:, 6]))
    p = rows[rr, 0]
    rv = rev[p] != 0
    # one table of units: text, b, kind (1 / 2 pair units by `first`, 3 / 4 read units by strand), end, score, number
    uj = np.r_[j[Fh], j[p]].astype(np.int64)
    ub = np.r_[ts[Fh], np.where(rv, te[p] - 1, ts[p])].astype(np.int64)
    kind = np.r_[np.where(h_fwd, 1, 2), np.where(rv, 4, 3)]
    end = np.r_[te[Rh], np.zeros(len(rr), np.int64)].astype(np.int64)
    score = np.r_[prow[pf, 3], rows[rr, 1]].astype(np.int64)
    unit = np.r_[pf, rr]
    order = np.lexsort((unit, -score, end, kind, ub, uj))
    uj, ub, kind, end, unit = uj[order], ub[order], kind[order], end[order], unit[order]
    n = len(order)
    if n == 0:
        return read_rows.astype(np.int32), pair_rows.astype(np.int32)
    new_b = np.r_[True, (uj[1:] != uj[:-1]) | (ub[1:] != ub[:-1])]
    new_g = new_b | np.r_[True, (kind[1:] != kind[:-1]) | (end[1:] != end[:-1])]
    bstart, gstart = np.flatnonzero(new_b), np.flatnonzero(new_g)
    bsize = np.diff(np.r_[bstart, n])[np.cumsum(new_b) - 1]
    gsize = np.diff(np.r_[gstart, n])[np.cumsum(new_g) - 1]
    over = bsize > MAX_BUCKET
    rep = np.where(over, unit, unit[gstart][np.cumsum(new_g) - 1])
    out = np.stack([rep, np.where(over, 1, gsize), (rep != unit).astype(np.int64), over.astype(np.int64)], 1)
    is_pair = kind <= 2
    pair_rows[unit[is_pair]] = out[is_pair]
    read_rows[unit[~is_pair]] = out[~is_pair]
    for side in (0, 1):
        m = mates[unit[is_pair], side]
        read_rows[m, 2], read_rows[m, 3] = out[is_pair, 2], out[is_pair, 3]
    return read_rows.astype(np.int32), pair_rows.astype(np.int32)


def main():
    from pywfa_amd import WavefrontAligner

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    rng = np.random.default_rng(2028)
    codes = [rng.integers(0, 4, REFLEN) for _ in range(NREF)]
    refs = [LUT[c].tobytes().decode() for c in codes]
    nfrag = 8192
    reads, places = [], []
    for f in range(nfrag):
        if f % 8 == 7:
            r, left, outer = places[int(rng.integers(0, len(places)))]
        else:
            r, outer, left = int(rng.integers(0, NREF)), int(rng.integers(300, 601)), int(rng.integers(200, REFLEN - 1000))
        places.append((r, left, outer))
        mates = [copy_of(rng, codes[r][left:left + READ + 8]), copy_of(rng, codes[r][left + outer - READ:left + outer + 8]).translate(COMP)[::-1]]
        reads += [m.decode() for m in mates]
    print(f"{nfrag} fragments of two {READ} bp mates, every eighth a copy of another, {NREF} references of {REFLEN} bp", flush=True)
    al = WavefrontAligner(span="ends-free", text_begin_free=10, text_end_free=10)
    GAP, PAR = 24, dict(min_insert=0, max_insert=1000)
    with al.sequence_set(reads) as R, al.sequence_set(refs) as G:
        with al.seed_index(G) as idx:
            s = idx.seeds(R)
        keep = s["j"] >= 0
        i = np.nonzero(keep)[0].astype(np.int32)
        wins = dict(i=i, j=s["j"][keep], text_start=s["text_start"][keep], text_len=s["text_len"][keep], reverse=s["reverse"][keep].astype(np.uint8))
        print(f"{len(i)} windows of seeds(n=4)", flush=True)
        t = {False: [], True: []}
        for dup in (False, True):
            al.place_pairs(R, G, duplicates=dup, **PAR, **wins)   # warm-up
        for _ in range(reps):
            for dup in (False, True):
                t0 = time.perf_counter()
                res = al.place_pairs(R, G, duplicates=dup, **PAR, **wins)
                t[dup].append(time.perf_counter() - t0)
        pr, rd = res["pairs"], res["reads"]
        print(f"place_pairs(duplicates=True) from Python on open handles: median {med(t[True]) * 1e3:.2f} ms (min {min(t[True]) * 1e3:.2f}, max "
              f"{max(t[True]) * 1e3:.2f}); place_pairs(): median {med(t[False]) * 1e3:.2f} ms (min {min(t[False]) * 1e3:.2f}, max "
              f"{max(t[False]) * 1e3:.2f}); proper {int(pr['proper'].sum())} of {nfrag}, duplicate fragments {int(pr['dup'].sum())} (copies made: "
              f"{nfrag // 8}), duplicate reads {int(rd['dup'].sum())}, overflow {int(pr['dup_overflow'].sum())}", flush=True)
        nat = al._native
        rb = nat.batch_windows(R._set, G._set, wins["i"], wins["j"], None, None, wins["text_start"], wins["text_len"], wins["reverse"])
        rb.run()
        rb.sync()
        how = (INT32_MIN, GAP, PAR["min_insert"], PAR["max_insert"], GAP)
        k_pairs, k_dup, t_dup = [], [], []
        pl = nat.placer(2 * nfrag)
        pl.add(rb, wins["i"], wins["j"], wins["text_start"], wins["reverse"])
        for _ in range(reps + 1):
            pl.run_pairs(nfrag, *how)
            k_pairs.append(pl.kernel_ms())
            t0 = time.perf_counter()
            out = pl.duplicates(G._set, nfrag, *how)
            t_dup.append(time.perf_counter() - t0)
            k_dup.append(pl.kernel_ms())
        pl.close()
        rb.close()
        k_pairs, k_dup, t_dup = k_pairs[1:], k_dup[1:], t_dup[1:]
        print(f"placer alone on {len(i)} hits (the grouping kept from call to call): run_pairs kernels (HIP events) median {med(k_pairs):.4f} ms; duplicates "
              f"kernels (the same, the plane's memset, key, scan, scatter, resolve) median {med(k_dup):.4f} ms (min {min(k_dup):.4f}, max "
              f"{max(k_dup):.4f}); duplicates from Python median {med(t_dup) * 1e3:.3f} ms; equal to place_pairs: "
              f"{np.array_equal(out[1][:, 2], pr['dup']) and np.array_equal(out[0][:, 2], rd['dup'])}", flush=True)
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
            prow, _ = numpy_pair(rows, flags, mates, wins["i"], wins["j"], wins["reverse"], a["score"], a["status"], ts, te, INT32_MIN, GAP,
                                 PAR["min_insert"], PAR["max_insert"], GAP)
            t2 = time.perf_counter()
            rrows, frows = numpy_duplicates(rows, prow, mates, wins["j"], wins["reverse"], ts, te)
            t3 = time.perf_counter()
            t_host.append(t3 - t0)
            t_rule.append((t2 - t1, t3 - t2))
        same = all(np.array_equal(frows[:, c], pr[k]) and np.array_equal(rrows[:, c], rd[k]) for c, k in enumerate(("dup_rep", "dup_size", "dup", "dup_overflow")))
        print(f"align_windows(summary=True) + the three rules in NumPy: median {med(t_host) * 1e3:.2f} ms (min {min(t_host) * 1e3:.2f}, max "
              f"{max(t_host) * 1e3:.2f}), of which placement and pairing {med([x[0] for x in t_rule]) * 1e3:.2f} ms and the duplicate lexsort "
              f"{med([x[1] for x in t_rule]) * 1e3:.2f} ms; equal to place_pairs(duplicates=True): {same}; "
              f"place_pairs(duplicates=True) / this route = {med(t[True]) / med(t_host):.3f}", flush=True)
    al.close()


if __name__ == "__main__":
    main()
