"""Shared by the rescue tests (test_rescue_abi.py, test_rescue_gpu.py): the rule of include/wfa_hip.h ("rescue") restated in plain
Python from the header's text on top of pair_common.py_pair, and a generator of random cases — the hit lists of
pair_common.random_case with read lengths, text lengths (some shorter than the windows) and the three parameters of the rule — in
which every clause of the rule occurs."""
import numpy as np

from pair_common import fragments, py_pair, random_case

RESCUE_COLUMNS = ("i", "j", "text_start", "text_len", "reverse", "fragment", "anchor", "spare")
CLAUSES = ("forward", "reverse", "two", "no_hit", "pairings", "overflow", "empty", "clip_lo", "clip_hi", "dropped", "mapq", "made")


def py_rescue(hits, nreads, mates, par, read_len, text_len, pad, min_len, anchor_mapq, seen=None):
    """The window list of the rule: int32 of shape (count, 8).  `par`: the parameters of py_pair.  `seen`, a dict, counts how often
    each clause decided (CLAUSES)."""
    seen = seen if seen is not None else {}
    for k in CLAUSES:
        seen.setdefault(k, 0)
    rows, flags, pair_rows, pair_flags = py_pair(hits, nreads, mates, par["min_score"], par["full_gap"], par["min_insert"], par["max_insert"],
                                                 par["unpaired"])
    rev = hits["reverse"] if hits.get("reverse") is not None else [0] * len(hits["i"])
    lo_ins, hi_ins = par["min_insert"], par["max_insert"]
    out = []
    for f, (m1, m2) in enumerate(fragments(mates, nreads)):
        proper, pairings, overflow = (int(pair_rows[f][c]) for c in (2, 9, 11))
        if proper or pairings or overflow:
            seen["pairings"] += int(pairings > 0)
            seen["overflow"] += int(overflow)
            continue
        made = 0
        for m, o in ((m1, m2), (m2, m1)):
            a, mapq = int(rows[m][0]), int(rows[m][3])
            if a < 0:
                seen["no_hit"] += 1
                continue
            ts, te, j, r = int(hits["text_start"][a]), int(hits["text_end"][a]), int(hits["j"][a]), 1 if rev[a] else 0
            if te <= ts:
                seen["empty"] += 1
                continue
            if mapq < anchor_mapq:
                seen["mapq"] += 1
                continue
            if r == 0:
                lo, hi = ts + lo_ins - int(read_len[o]) - pad, ts + hi_ins + pad
            else:
                lo, hi = te - hi_ins - pad, te - lo_ins + int(read_len[o]) + pad
            clip_lo, clip_hi = lo < 0, hi > int(text_len[j])
            lo, hi = max(lo, 0), min(hi, int(text_len[j]))
            if hi - lo < max(min_len, 1):
                seen["dropped"] += 1
                continue
            seen["clip_lo"] += int(clip_lo)   # (the clips of windows that were made)
            seen["clip_hi"] += int(clip_hi)
            seen["reverse" if r else "forward"] += 1
            out.append((o, j, lo, hi - lo, 1 - r, f, a, 0))
            made += 1
        seen["two"] += int(made == 2)
        seen["made"] += made
    return np.array(out, np.int32).reshape(-1, 8)


def random_rescue_case(rng, max_hits=120):
    """(nreads, hits, mates, par, read_len, text_len, pad, min_len, anchor_mapq): a case of pair_common.random_case; reads of 0 .. 40
    bases; two texts whose lengths are drawn from 25 (shorter than most windows), 120, 260 and 3000; in one case of thirty the two reads
    of the first fragment get 257 and 256 more eligible hits, one more pairing than a fragment may have (overflow)."""
    nreads, hits, mates, par = random_case(rng, max_hits)
    frags = fragments(mates, nreads)
    if frags and rng.random() < 1 / 30:
        a, b = frags[0]
        extra = dict(i=[a] * 257 + [b] * 256, j=[0] * 513, reverse=[0] * 257 + [1] * 256, score=[0] * 513, status=[0] * 513,
                     text_start=[200] * 513, text_end=[230] * 513)
        hits = {k: np.concatenate([np.asarray(hits[k]), np.asarray(extra[k])]) for k in hits}
    read_len = rng.integers(0, 41, nreads).astype(np.int32)
    text_len = rng.choice([25, 120, 260, 3000], 2).astype(np.int32)
    return (nreads, hits, mates, par, read_len, text_len, int(rng.choice([0, 5, 16])), int(rng.choice([0, 30, 200])),
            int(rng.choice([0, 1, 60])))


def sized_case(rng, nfrag, kind="mixed", shuffled=False):
    """(nreads, hits, mates, read_len, text_len) with `nfrag` fragments for the device kernels: "all" — both mates placed, on
    different texts, so that every fragment is rescued twice; "none" — every fragment a proper pairing; "mixed" — per fragment one
    of: proper, both mates on different texts, one mate only (either one, either strand), one mate with an empty interval, one mate
    with an ineligible hit, one mate with two tied hits (mapq 0), no hit.  `shuffled`: the mates as an (F, 2) array over a permutation
    of the reads, three reads in no fragment; otherwise interleaved.  Hits in shuffled order."""
    nreads = 2 * nfrag + (3 if shuffled else 0)
    if shuffled:
        mates = rng.permutation(nreads)[:2 * nfrag].reshape(nfrag, 2).astype(np.int32)
    else:
        mates = nfrag
    frags = np.asarray(fragments(mates, nreads), np.int64).reshape(nfrag, 2)
    what = {"all": np.full(nfrag, 1), "none": np.full(nfrag, 0)}.get(kind)
    if what is None:
        what = rng.integers(0, 8, nfrag)
    rows = []   # (i, j, reverse, score, status, ts, te)
    for f in range(nfrag):
        a, b = (int(x) for x in frags[f])
        ts = int(rng.integers(0, 2600))
        k = int(what[f])
        side = int(rng.integers(0, 2))
        one = (a, b)[side]
        if k == 0:
            rows += [(a, 0, side, -4, 0, ts + 200 * side, ts + 200 * side + 100), (b, 0, 1 - side, -4, 0, ts + 200 * (1 - side), ts + 200 * (1 - side) + 100)]
        elif k == 1:
            rows += [(a, 0, side, -4, 0, ts + 200, ts + 300), (b, 1, int(rng.integers(0, 2)), -8, 0, 200 + ts // 4, 290 + ts // 4)]   # (far enough from the ends: no window is clipped away)
        elif k == 2:
            rows += [(one, int(rng.integers(0, 2)), int(rng.integers(0, 2)), -4, 0, ts, ts + 100)]
        elif k == 3:
            rows += [(one, 0, 0, -4, 0, ts, ts)]
        elif k == 4:
            rows += [(one, 0, 1, -4, 1, ts, ts + 100)]
        elif k == 5:
            rows += [(one, 0, 1, -4, 0, ts, ts + 100), (one, 1, 0, -4, 0, ts // 3, ts // 3 + 100)]
        elif k == 6:
            rows += [(one, 1, 0, -4, 0, 0, 60), (one, 1, 0, -9, 0, 2900, 3000)]
    rows = [rows[q] for q in rng.permutation(len(rows))]
    cols = list(zip(*rows)) if rows else [[]] * 7
    hits = {k: np.asarray(c, np.int32) for k, c in zip(("i", "j", "reverse", "score", "status", "text_start", "text_end"), cols)}
    return nreads, hits, mates, rng.integers(0, 41, nreads).astype(np.int32), np.array([3000, 1400], np.int32)


def rescue_corpus(seed=15):
    """pair_common.pair_corpus with, for every third fragment that is not a repeat fragment, the window at mate 2's true place taken
    out of the list (mate 2 keeps its random window only).  Returns refs, reads, the window list, truth and the fragments it was done
    to.  The seed is one under which the REFERENCE (the oracle and the restatements, test_rescue_abi.py) brings every such mate
    back: the references are 4 kb long, and under many seeds a fragment lies so near an end of its reference that its rescue window
    is clipped below F bases and, by the rule, not made."""
    from pair_common import pair_corpus
    from place_common import PAD
    refs, reads, W, truth = pair_corpus(seed)
    plain = [f for f, t in enumerate(truth) if not t[4]]
    dropped = plain[::3]
    keep = np.ones(len(W["i"]), bool)
    for f in dropped:
        r2, pos2 = truth[f][6]
        at = (W["i"] == 2 * f + 1) & (W["j"] == r2) & (W["t_start"] == max(0, pos2 - PAD))
        assert at.sum() == 1, f
        keep &= ~at
    return refs, reads, {k: v[keep] for k, v in W.items()}, truth, dropped


def window_list(found, read_len):
    """The window list (the arrays of test_windows_gpu.as_list) of rescue rows: the pattern window is the whole read."""
    found = np.asarray(found, np.int32).reshape(-1, 8)
    i = found[:, 0].astype(np.int64)
    return dict(i=i, j=found[:, 1].copy(), p_start=np.zeros(len(i), np.int32), p_len=np.asarray(read_len, np.int64)[i],
                t_start=found[:, 2].astype(np.int64), t_len=found[:, 3].copy(), reverse=found[:, 4].astype(np.uint8))


def join_hits(a, b):
    return {k: np.concatenate([np.asarray(a[k], np.int64), np.asarray(b[k], np.int64)]) for k in ("i", "j", "reverse", "score", "status", "text_start", "text_end")}
