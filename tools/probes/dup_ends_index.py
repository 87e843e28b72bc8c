"""Probe of duplicates on unclipped ends and of the representative by base quality (WavefrontAligner.place_pairs(duplicates=True,
dup_ends=, dup_qualities=), wfa_hip_placer_duplicates_ex).

Workload: that of dup_index.py — 8 references of 1 Mb (fixed seed), 8 192 fragments of two 150 bp mates cut 300 - 600 bases apart at
2 %, seeds(n=4) under the default parameters, gap-affine, ends-free with 10 free text bases on either side, scope full, every eighth
fragment a copy of another — with the copies made the way PCR makes them: BOTH 5' ENDS FIXED.  Each mate is taken from its 5' end on
its own strand, gets its own errors, and is trimmed at its 3' end; dup_index.py trims the reverse mate before the reverse complement,
which moves its 5' end, and no duplicate rule can recover that.
(1) The copies marked under dup_ends="core", "unclipped" and "unclipped" with qualities, of the copies made.
(2) place_pairs(duplicates=True) under each of the three from Python on open handles, medians of REPS.
(3) The kernels by HIP events through the C ABI binding on one resident batch after its run: Placer.duplicates under flags 0, 1 and 3,
    medians of REPS; WFA_HIP_REDUCE_TIMING=1 makes the library print the record kernel's time on stderr.
--errors subs: every error is a substitution (2 %), as sequencers that rarely make indels give them; the default is pair_index.copy_of's
mix of substitutions, deletions and insertions in equal parts, in which an indel next to a 5' end moves the unclipped end as a
substitution there moves the core's.
Usage: dup_ends_index.py [--reps N] [--errors mix|subs]"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), HERE]
os.environ["WFA_HIP_REDUCE_TIMING"] = "1"   # (read when an aligner is created)
import numpy as np  # noqa: E402

from pair_index import INT32_MIN, LUT, NREF, READ, REFLEN, copy_of, med  # noqa: E402


def subs_of(rng, f, div=0.02):
    """The first READ bases of f (codes 0..3) with substitutions at `div`."""
    f = f[:READ]
    hit = rng.random(READ) < div
    return LUT[np.where(hit, (f + rng.integers(1, 4, READ)) % 4, f)].tobytes()


def main():
    from pywfa_amd import WavefrontAligner

    errors = sys.argv[sys.argv.index("--errors") + 1] if "--errors" in sys.argv else "mix"
    make = {"mix": copy_of, "subs": subs_of}[errors]

    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    rng = np.random.default_rng(2028)
    codes = [rng.integers(0, 4, REFLEN) for _ in range(NREF)]
    refs = [LUT[c].tobytes().decode() for c in codes]
    nfrag = 8192
    reads, quals, places = [], [], []
    for f in range(nfrag):
        if f % 8 == 7:
            r, left, outer = places[int(rng.integers(0, len(places)))]
        else:
            r, outer, left = int(rng.integers(0, NREF)), int(rng.integers(300, 601)), int(rng.integers(200, REFLEN - 1000))
        places.append((r, left, outer))
        fwd = codes[r][left:left + READ + 8]                                  # from the fragment's left 5' end
        rev = (3 - codes[r][left + outer - READ - 8:left + outer])[::-1]      # from its right 5' end, on the other strand
        reads += [make(rng, fwd).decode(), make(rng, rev).decode()]           # (both trim behind READ bases: the 3' end)
        quals += [rng.integers(10, 41, READ).astype(np.uint8) for _ in range(2)]
    copies = np.arange(nfrag) % 8 == 7
    print(f"{nfrag} fragments of two {READ} bp mates, every eighth a copy of another with both 5' ends kept ({int(copies.sum())} copies), errors: {errors}, "
          f"{NREF} references of {REFLEN} bp", flush=True)
    al = WavefrontAligner(span="ends-free", text_begin_free=10, text_end_free=10)
    GAP, PAR = 24, dict(min_insert=0, max_insert=1000)
    with al.sequence_set(reads) as R, al.sequence_set(refs) as G, al.quality_set(R, quals) as Q:
        with al.seed_index(G) as idx:
            s = idx.seeds(R)
        keep = s["j"] >= 0
        i = np.nonzero(keep)[0].astype(np.int32)
        wins = dict(i=i, j=s["j"][keep], text_start=s["text_start"][keep], text_len=s["text_len"][keep], reverse=s["reverse"][keep].astype(np.uint8))
        print(f"{len(i)} windows of seeds(n=4)", flush=True)
        modes = (("core", dict()), ("unclipped", dict(dup_ends="unclipped")), ("unclipped + qualities", dict(dup_ends="unclipped", dup_qualities=Q)))
        t = {name: [] for name, _ in modes}
        res = {}
        for name, kw in modes:
            al.place_pairs(R, G, duplicates=True, **kw, **PAR, **wins)   # warm-up
        for _ in range(reps):
            for name, kw in modes:
                t0 = time.perf_counter()
                res[name] = al.place_pairs(R, G, duplicates=True, **kw, **PAR, **wins)
                t[name].append(time.perf_counter() - t0)
        for name, _ in modes:
            pr = res[name]["pairs"]
            # a copy and its source are one group: the group's later member or its earlier one is the duplicate
            grouped = int(((pr["dup_size"] >= 2) & copies).sum())
            print(f"dup_ends {name}: copies in a group of two or more {grouped} of {int(copies.sum())}; duplicate fragments {int(pr['dup'].sum())}, "
                  f"overflow {int(pr['dup_overflow'].sum())}, proper {int(pr['proper'].sum())}; place_pairs(duplicates=True) median "
                  f"{med(t[name]) * 1e3:.2f} ms (min {min(t[name]) * 1e3:.2f}, max {max(t[name]) * 1e3:.2f}), / core = {med(t[name]) / med(t['core']):.3f}",
                  flush=True)
        nat = al._native
        rb = nat.batch_windows(R._set, G._set, wins["i"], wins["j"], None, None, wins["text_start"], wins["text_len"], wins["reverse"])
        rb.run()
        rb.sync()
        how = (INT32_MIN, GAP, PAR["min_insert"], PAR["max_insert"], GAP)
        pl = nat.placer(2 * nfrag)
        for _ in range(reps):      # (the library prints "place record kernel" on stderr for each)
            pl.clear()
            pl.add(rb, wins["i"], wins["j"], wins["text_start"], wins["reverse"])
        lead, trail = pl.clips()
        print(f"clips of {len(lead)} hits: lead > 0 in {int((lead > 0).sum())}, trail > 0 in {int((trail > 0).sum())}, greatest {int(max(lead.max(), trail.max()))}", flush=True)
        for name, kw in (("flags 0", dict()), ("flags 1 (unclipped)", dict(unclipped=True)), ("flags 3 (unclipped, by quality)", dict(unclipped=True, qualities=Q._set))):
            k = []
            for _ in range(reps + 1):
                pl.duplicates(G._set, nfrag, *how, **kw)
                k.append(pl.kernel_ms())
            k = k[1:]
            print(f"placer alone on {len(i)} hits, duplicates kernels (HIP events) under {name}: median {med(k):.4f} ms (min {min(k):.4f}, max {max(k):.4f})", flush=True)
        pl.close()
        rb.close()
    al.close()


if __name__ == "__main__":
    main()
