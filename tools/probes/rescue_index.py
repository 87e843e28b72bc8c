"""Probe of mate rescue (WavefrontAligner.place_pairs(rescue=True), wfa_hip_placer_rescue).

Workload: that of pair_index.py — 8 references of 1 Mb (fixed seed), 8 192 fragments of two 150 bp mates cut 300 - 600 bases apart
(outer distance) at 2 %, seeds(n=4) under the default parameters, gap-affine, ends-free with 10 free text bases on either side, scope
full — with, for every fourth fragment, every window of mate 2 that overlaps its true place taken out of the list.  min_score -100,
min_insert 250, max_insert 650, rescue_pad 16.
(1) The placer's own part through the C ABI binding on one resident batch after its run: rescue (group, place, pair, decide, scan, emit,
    by HIP events: Placer.kernel_ms()) beside run_pairs (the same without the three rescue kernels), medians of REPS.
(2) place_pairs(rescue=True) from Python on open handles, median of REPS.
(3) The route it replaces: place_pairs, the rule in NumPy on its outputs, align_windows on the list with the free ends set by hand,
    place_pairs once more (over the listed windows only: one configuration cannot align both lists, so this route is timed in its own
    favour); median of REPS; its NumPy window list is compared with the device's of (2), exact equality.
(4) The share of the removed mates that come back proper at their true place.
Usage: rescue_index.py [--reps N]"""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from pair_index import COMP, LUT, NREF, PAIR_COLUMNS, READ, REFLEN, copy_of, med  # noqa: E402

INT32_MIN = -2**31
KEYS = ("i", "j", "text_start", "text_len", "reverse")


def numpy_rescue(res, wins, mates, read_len, text_len, min_insert, max_insert, pad, min_len, anchor_mapq):
    """The rule of include/wfa_hip.h ("rescue") on the outputs of place_pairs: the rows (i, j, text_start, text_len, reverse, fragment,
    anchor) in list order."""
    pr, rd = res["pairs"], res["reads"]
    lost = (pr["proper"] == 0) & (pr["pairings"] == 0) & (pr["overflow"] == 0)
    frag = np.arange(len(mates), dtype=np.int64)
    parts = []
    for m in (0, 1):
        r, o = mates[:, m], mates[:, 1 - m]
        a = rd["hit"][r].astype(np.int64)
        ts, te = rd["text_start"][r].astype(np.int64), rd["text_end"][r].astype(np.int64)
        ok = lost & (a >= 0) & (te > ts) & (rd["mapq"][r] >= anchor_mapq)
        at = np.where(a >= 0, a, 0)
        j, rev = wins["j"][at].astype(np.int64), (wins["reverse"][at] != 0).astype(np.int64)
        lo = np.where(rev == 0, ts + min_insert - read_len[o] - pad, te - max_insert - pad)
        hi = np.where(rev == 0, ts + max_insert + pad, te - min_insert + read_len[o] + pad)
        lo, hi = np.maximum(lo, 0), np.minimum(hi, text_len[j])
        ok &= hi - lo >= max(min_len, 1)
        parts.append(np.stack([o, j, lo, hi - lo, 1 - rev, frag, a, np.full(len(frag), m)], 1)[ok])
    rows = np.concatenate(parts)
    return rows[np.lexsort((rows[:, 7], rows[:, 5]))][:, :7]


def main():
    from pywfa_amd import WavefrontAligner

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    rng = np.random.default_rng(2028)
    codes = [rng.integers(0, 4, REFLEN) for _ in range(NREF)]
    refs = [LUT[c].tobytes().decode() for c in codes]
    nfrag = 8192
    reads, place2 = [], []
    for f in range(nfrag):
        r, outer = int(rng.integers(0, NREF)), int(rng.integers(300, 601))
        left = int(rng.integers(200, REFLEN - 1000))
        two = [copy_of(rng, codes[r][left:left + READ + 8]), copy_of(rng, codes[r][left + outer - READ:left + outer + 8]).translate(COMP)[::-1]]
        reads += [m.decode() for m in (two[::-1] if f % 2 else two)]
        place2.append((r, left if f % 2 else left + outer - READ))
    place2 = np.array(place2, np.int64)
    print(f"{nfrag} fragments of two {READ} bp mates, {NREF} references of {REFLEN} bp", flush=True)
    al = WavefrontAligner(span="ends-free", text_begin_free=10, text_end_free=10)
    GAP, PAD = 24, 16
    PAR = dict(min_score=-100, min_insert=250, max_insert=650)
    FREE = PAR["max_insert"] - PAR["min_insert"] + 2 * PAD
    read_len, text_len = np.full(2 * nfrag, READ, np.int64), np.full(NREF, REFLEN, np.int64)
    mates = np.arange(2 * nfrag, dtype=np.int64).reshape(-1, 2)
    with al.sequence_set(reads) as R, al.sequence_set(refs) as G:
        with al.seed_index(G) as idx:
            s = idx.seeds(R)
        keep = s["j"] >= 0
        i = np.nonzero(keep)[0].astype(np.int32)
        wins = dict(i=i, j=s["j"][keep], text_start=s["text_start"][keep], text_len=s["text_len"][keep], reverse=s["reverse"][keep].astype(np.uint8))
        # every fourth fragment loses the windows of mate 2 that overlap its true place
        f = wins["i"] // 2
        true2 = ((wins["i"] % 2 == 1) & (f % 4 == 0) & (wins["j"] == place2[f, 0]) & (wins["text_start"] < place2[f, 1] + READ)
                 & (wins["text_start"] + wins["text_len"] > place2[f, 1]))
        removed = np.unique(f[true2])
        wins = {k: v[~true2] for k, v in wins.items()}
        n0 = len(wins["i"])
        print(f"{n0} windows of seeds(n=4) after {int(true2.sum())} windows of {len(removed)} mates were removed", flush=True)

        nat = al._native
        rb = nat.batch_windows(R._set, G._set, wins["i"], wins["j"], None, None, wins["text_start"], wins["text_len"], wins["reverse"])
        rb.run()
        rb.sync()
        how = (PAR["min_score"], GAP, PAR["min_insert"], PAR["max_insert"], GAP)
        k_pairs, k_rescue = [], []
        for _ in range(reps + 1):
            pl = nat.placer(2 * nfrag)
            pl.add(rb, wins["i"], wins["j"], wins["text_start"], wins["reverse"])
            pl.run_pairs(nfrag, *how)
            k_pairs.append(pl.kernel_ms())
            pl.clear()
            pl.add(rb, wins["i"], wins["j"], wins["text_start"], wins["reverse"])
            count, _ = pl.rescue(R._set, G._set, nfrag, *how, pad=PAD, min_len=FREE)
            k_rescue.append(pl.kernel_ms())
            pl.close()
        rb.close()
        print(f"placer alone on {n0} hits: rescue kernels (group, place, pair, decide, scan, emit; HIP events) median {med(k_rescue[1:]):.4f} ms, "
              f"run_pairs kernels median {med(k_pairs[1:]):.4f} ms: the three rescue kernels about {med(k_rescue[1:]) - med(k_pairs[1:]):.4f} ms; "
              f"{count} windows", flush=True)

        res = al.place_pairs(R, G, rescue=True, rescue_pad=PAD, **PAR, **wins)   # warm-up
        t_new = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res = al.place_pairs(R, G, rescue=True, rescue_pad=PAD, **PAR, **wins)
            t_new.append(time.perf_counter() - t0)
        print(f"place_pairs(rescue=True) from Python on open handles: median {med(t_new) * 1e3:.2f} ms (min {min(t_new) * 1e3:.2f}, max "
              f"{max(t_new) * 1e3:.2f}); {len(res['rescue']['i'])} rescue windows", flush=True)

        t_old, t_plain = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            first = al.place_pairs(R, G, **PAR, **wins)
            t_plain.append(time.perf_counter() - t0)
            rows = numpy_rescue(first, wins, mates, read_len, text_len, PAR["min_insert"], PAR["max_insert"], PAD, FREE, 0)
            extra = dict(i=rows[:, 0].astype(np.int32), j=rows[:, 1].astype(np.int32), text_start=rows[:, 2].astype(np.int32),
                         text_len=rows[:, 3].astype(np.int32), reverse=rows[:, 4].astype(np.uint8))
            al.text_begin_free, al.text_end_free = FREE, FREE
            try:
                al.align_windows(R, G, **extra)
            finally:
                al.text_begin_free, al.text_end_free = 10, 10
            # (the second pairing has to align both lists again, the rescue windows under the wide free ends: two calls would be
            # needed for that; the listed windows alone are paired here, so this route is timed in its own favour)
            al.place_pairs(R, G, **PAR, **wins)
            t_old.append(time.perf_counter() - t0)
        same_list = all(np.array_equal(rows[:, c], res["rescue"][k]) for c, k in enumerate(("i", "j", "text_start", "text_len", "reverse", "fragment", "anchor")))
        print(f"the route it replaces (place_pairs, the rule in NumPy, align_windows with the free ends set by hand, place_pairs again): median "
              f"{med(t_old) * 1e3:.2f} ms (min {min(t_old) * 1e3:.2f}, max {max(t_old) * 1e3:.2f}); place_pairs alone median {med(t_plain) * 1e3:.2f} ms; "
              f"the NumPy list equals the device's: {same_list}; this stand-in pairs the listed windows only, so it bounds the full route from below", flush=True)

        pr, rd = res["pairs"], res["reads"]
        lost = first["pairs"]["proper"][removed] == 0
        r2 = 2 * removed + 1
        ov = np.minimum(rd["text_end"][r2], place2[removed, 1] + READ) - np.maximum(rd["text_start"][r2], place2[removed, 1])
        back = (pr["proper"][removed] == 1) & (pr["hit2"][removed] >= n0) & (rd["hit"][r2] == pr["hit2"][removed]) & (2 * ov >= READ)
        where = np.where(pr["hit2"][removed] >= n0, pr["hit2"][removed] - n0, 0)
        back &= res["rescue"]["j"][where] == place2[removed, 0]
        print(f"of {len(removed)} removed mates {int(lost.sum())} fragments were not proper without rescue; with rescue {int(back.sum())} are proper "
              f"with mate 2 at its true place ({100.0 * back.sum() / len(removed):.2f} %); rescued fragments in all: {int(pr['rescued'].sum())}; "
              f"pair columns: {', '.join(PAIR_COLUMNS[:3])}, ...", flush=True)
    al.close()


if __name__ == "__main__":
    main()
