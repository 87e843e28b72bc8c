"""Shared by the placement tests (test_place_abi.py, test_place_gpu.py): the rule of include/wfa_hip.h ("placement") restated in plain
Python from the header's text, the text interval of a batch's pair from an op string, and a corpus with an exact repeat, a near-repeat
and windows at the true locus, next to it, at the other copy and at a random place."""
import numpy as np

from reduce_common import core_of
from test_windows_gpu import LETTERS, as_list, mutate, revcomp

INT32_MIN = -2**31
KEYS = ("i", "j", "reverse", "score", "status", "text_start", "text_end")
COLUMNS = ("hit", "score", "second", "mapq", "hits", "ties", "text_start", "text_end")


def py_place(hits, nreads, min_score, full_gap):
    """(rows, flags) of the rule.  `hits`: a dict of equally long sequences under KEYS, in hit-number order (reverse may be None)."""
    n = len(hits["i"])
    rev = hits["reverse"] if hits.get("reverse") is not None else [0] * n
    H = [(int(hits["i"][h]), int(hits["j"][h]), 1 if rev[h] else 0, int(hits["score"][h]), int(hits["status"][h]),
          int(hits["text_start"][h]), int(hits["text_end"][h])) for h in range(n)]
    rows = np.zeros((nreads, 8), np.int32)
    flags = np.zeros(n, np.uint8)
    groups = [[] for _ in range(nreads)]
    for h, x in enumerate(H):
        groups[x[0]].append(h)
    for r, g in enumerate(groups):
        elig = [h for h in g if H[h][4] == 0 and H[h][3] >= min_score]
        if not elig:
            rows[r] = (-1, INT32_MIN, INT32_MIN, 0, 0, 0, 0, 0)
            continue
        p = min(elig, key=lambda h: (-H[h][3], h))
        _, jp, sp, score_p, _, ts_p, te_p = H[p]
        flags[p] = 3
        others = []
        for h in elig:
            if h == p:
                continue
            _, jh, sh, score_h, _, ts_h, te_h = H[h]
            ov = min(te_h, te_p) - max(ts_h, ts_p)
            same = jh == jp and sh == sp and ov > 0 and 2 * ov >= min(te_h - ts_h, te_p - ts_p)
            flags[h] = 2 if same else 1
            if not same:
                others.append(score_h)
        second = max(others) if others else INT32_MIN
        mapq = min(60, 60 * (score_p - second) // full_gap) if others else 60
        rows[r] = (p, score_p, second, mapq, len(elig), sum(1 for s in others if s == score_p), ts_p, te_p)
    return rows, flags


def interval_of(ops, plen, tlen, t_start, full=True):
    """[ts, te) of a batch's pair in coordinates of its text.  Scope full: t_start + columns 8 and 9 of the per-pair summary, i.e. the
    text bases in front of the first M and up to the last M (zeros for an empty pair or an empty op string; an op string without an M
    strips every text base from both ends).  Scope score: the window."""
    if not full:
        return t_start, t_start + tlen
    ops = bytes(ops)
    if not ops or not plen or not tlen:
        return t_start, t_start
    core = core_of(ops)
    if core is None:
        used = sum(1 for c in ops if c in b"XI")
        return t_start + used, t_start + tlen - used
    head = sum(1 for c in ops[:core[0]] if c in b"XI")
    tail = sum(1 for c in ops[core[1] + 1:] if c in b"XI")
    return t_start + head, t_start + tlen - tail


def hits_of(o, W, full=True):
    """The hit list of a window list from the oracle's results `o` of its materialised pairs."""
    n = len(W["i"])
    iv = [interval_of(o["cigars"][q] if full else b"", int(W["p_len"][q]), int(W["t_len"][q]), int(W["t_start"][q]), full) for q in range(n)]
    return dict(i=W["i"], j=W["j"], reverse=W["reverse"], score=np.asarray(o["score"]), status=np.asarray(o["status"]),
                text_start=[a for a, _ in iv], text_end=[b for _, b in iv])


def as_arrays(hits):
    out = {k: np.asarray(hits[k], np.int32) for k in KEYS if k != "reverse"}
    out["reverse"] = None if hits.get("reverse") is None else np.asarray(hits["reverse"], np.uint8)
    return out


EDGE = 8          # bases at either end of a read that are never mutated: its aligned core is then its whole locus
PAD, SHIFT = 10, 10


def corpus(seed=5, nreads=200, shuffle=True):
    """Three references of about 4 kb.  An exact 300-base repeat lies at refs[0][600:900] and refs[1][2500:2800]; a near-repeat at
    refs[1][800:1100] and, with two substitutions, at refs[2][1500:1800].  Reads of 150 bases: two in five from anywhere, one in
    five inside a copy of the exact repeat, one inside a copy of the near-repeat, one across an edge of a copy; mutated at 3 % away
    from their ends, every second one stored reverse-complemented.  Windows per read: its true locus padded by PAD, the same shifted
    right by SHIFT, the same offset at the other copy where the read touches a copy, and a random place — listed in shuffled order.
    Returns refs, reads, the window list and per read (reference, position, locus length, reversed, touches a copy)."""
    rng = np.random.default_rng(seed)
    bases = [rng.integers(0, 4, n) for n in (4000, 4200, 3800)]
    rep = rng.integers(0, 4, 300)
    bases[0][600:900] = rep
    bases[1][2500:2800] = rep
    near = rng.integers(0, 4, 300)
    bases[1][800:1100] = near
    bases[2][1500:1800] = near
    for at in (1600, 1700):
        bases[2][at] = (bases[2][at] + 1) % 4
    copies = [((0, 600), (1, 2500)), ((1, 2500), (0, 600)), ((1, 800), (2, 1500)), ((2, 1500), (1, 800))]
    refs = ["".join(LETTERS[b]) for b in bases]
    reads, origin, rows = [], [], []
    L = 150
    for k in range(nreads):
        kind = k % 5
        if kind < 2:
            r = int(rng.integers(0, 3))
            pos = int(rng.integers(0, len(bases[r]) - L + 1))
        else:
            (r, c0), _ = copies[int(rng.integers(0, 2)) + (2 if kind == 3 else 0)] if kind < 4 else copies[int(rng.integers(0, 4))]
            if kind < 4:
                pos = c0 + int(rng.integers(0, 300 - L + 1))
            else:
                pos = c0 - L + int(rng.integers(20, 100)) if rng.random() < 0.5 else c0 + 300 - int(rng.integers(20, 100))
        f = bases[r][pos:pos + L]
        s = "".join(LETTERS[np.r_[f[:EDGE], mutate(rng, f[EDGE:-EDGE], 0.03), f[-EDGE:]]])
        rev = k % 2 == 1
        reads.append(revcomp(s) if rev else s)
        other = [(r2, c2 + (pos - c1)) for (r1, c1), (r2, c2) in copies if r1 == r and pos < c1 + 300 and pos + L > c1]
        origin.append((r, pos, L, rev, bool(other)))
        places = [(r, pos - PAD), (r, pos - PAD + SHIFT)] + other[:1]
        rr = int(rng.integers(0, 3))
        places.append((rr, int(rng.integers(0, len(bases[rr]) - L))))
        for j, t0 in places:
            t0 = max(0, t0)
            t1 = min(len(refs[j]), t0 + L + 2 * PAD)
            rows.append((k, j, 0, len(s), t0, t1 - t0, int(rev)))
    if shuffle:
        rows = [rows[q] for q in rng.permutation(len(rows))]
    return refs, reads, as_list(rows), origin
