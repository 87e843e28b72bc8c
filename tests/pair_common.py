"""Shared by the pairing tests (test_pair_abi.py, test_pair_gpu.py): the rule of include/wfa_hip.h ("pairing") restated in plain Python
from the header's text on top of place_common.py_place, a generator of random hit lists in which every clause of the rule occurs, and
a paired corpus over the references of place_common.corpus: fragments of two 150-base mates, a fifth of them with mate 1 inside a copy
of the exact repeat and mate 2 in unique sequence."""
import numpy as np

from place_common import EDGE, INT32_MIN, PAD, corpus, py_place
from test_windows_gpu import LETTERS, as_list, mutate, revcomp

INT32_MAX = 2**31 - 1
PAIR_COLUMNS = ("hit1", "hit2", "proper", "score", "second", "mapq", "mapq1", "mapq2", "insert", "pairings", "ties", "overflow")
MAX_PAIRINGS = 65536
HIT_KEYS = ("i", "j", "reverse", "score", "status", "text_start", "text_end")


def saturate(v):
    return max(INT32_MIN + 1, min(INT32_MAX, v))


def fragments(mates, nreads):
    """The list of (mate1, mate2): `mates` an int (interleaved) or a sequence of pairs."""
    if isinstance(mates, (int, np.integer)):
        assert 2 * mates <= nreads
        return [(2 * f, 2 * f + 1) for f in range(int(mates))]
    return [(int(a), int(b)) for a, b in mates]


def py_pair(hits, nreads, mates, min_score, full_gap, min_insert, max_insert, unpaired):
    """(rows, flags, pair_rows, pair_flags) of the rule.  `hits` as for py_place."""
    rows, flags = py_place(hits, nreads, min_score, full_gap)
    n = len(hits["i"])
    rev = hits["reverse"] if hits.get("reverse") is not None else [0] * n
    H = [(int(hits["j"][h]), 1 if rev[h] else 0, int(hits["score"][h]), int(hits["text_start"][h]), int(hits["text_end"][h])) for h in range(n)]
    elig = [[] for _ in range(nreads)]
    for h in range(n):
        if int(hits["status"][h]) == 0 and H[h][2] >= min_score:
            elig[int(hits["i"][h])].append(h)

    def insert_of(h, g):
        """te_R - ts_F of a PROPER pairing, None of any other."""
        (jh, rh, _, tsh, teh), (jg, rg, _, tsg, teg) = H[h], H[g]
        if jh != jg or rh == rg or teh <= tsh or teg <= tsg:
            return None
        (tsF, teF), (tsR, teR) = ((tsh, teh), (tsg, teg)) if rh == 0 else ((tsg, teg), (tsh, teh))
        if not (tsF <= tsR and teF <= teR):
            return None
        return teR - tsF if min_insert <= teR - tsF <= max_insert else None

    def at_locus(h, p):
        (jh, rh, _, tsh, teh), (jp, rp, _, tsp, tep) = H[h], H[p]
        ov = min(teh, tep) - max(tsh, tsp)
        return h != p and jh == jp and rh == rp and ov > 0 and 2 * ov >= min(teh - tsh, tep - tsp)

    frags = fragments(mates, nreads)
    pair_rows = np.zeros((len(frags), 12), np.int32)
    pair_flags = flags.copy()
    for f, (a, b) in enumerate(frags):
        sa, sb = rows[a], rows[b]
        out = dict(hit1=sa[0], hit2=sb[0], proper=0, score=INT32_MIN, second=INT32_MIN, mapq=0, mapq1=sa[3], mapq2=sb[3], insert=0,
                   pairings=0, ties=0, overflow=0)
        if int(sa[4]) * int(sb[4]) > MAX_PAIRINGS:
            out["overflow"] = 1
        else:
            proper = [(H[h][2] + H[g][2], h, g) for h in elig[a] for g in elig[b] if insert_of(h, g) is not None]
            out["pairings"] = len(proper)
            if proper:
                ps, h, g = min(proper, key=lambda t: (-t[0], t[1], t[2]))
                if ps + unpaired >= int(sa[1]) + int(sb[1]):
                    others = [t[0] for t in proper
                              if not ((t[1] == h or at_locus(t[1], h)) and (t[2] == g or at_locus(t[2], g)))]
                    mapq = min(60, 60 * (ps - max(others)) // full_gap) if others else 60
                    out.update(hit1=h, hit2=g, proper=1, score=saturate(ps), second=saturate(max(others)) if others else INT32_MIN,
                               mapq=mapq, mapq1=max(mapq, sa[3]) if flags[h] >= 2 else mapq,
                               mapq2=max(mapq, sb[3]) if flags[g] >= 2 else mapq, insert=insert_of(h, g),
                               ties=sum(1 for s in others if s == ps))
                    for c, group in ((h, elig[a]), (g, elig[b])):
                        for x in group:
                            pair_flags[x] = 3 if x == c else 2 if at_locus(x, c) else 1
        pair_rows[f] = [out[k] for k in PAIR_COLUMNS]
    return rows, flags, pair_rows, pair_flags


def as_hit_arrays(hits):
    out = {k: np.asarray(hits[k], np.int32) for k in HIT_KEYS if k != "reverse"}
    out["reverse"] = None if hits.get("reverse") is None else np.asarray(hits["reverse"], np.uint8)
    return out


def random_case(rng, max_hits=400):
    """(nreads, hits, mates, parameters): 0 .. max_hits hits over a few reads, one or two texts, both strands (a read's hits mostly on one), scores from a small range,
    intervals of length 0, 20 and 30 that start 0, 5 or 10 bases into one of three places per text (hits of one place are mostly the
    same locus; two of the places are near enough for a pairing), so that orders, containments and inserts of every kind occur; the fragments
    interleaved (an int) or a shuffled (F, 2) array, some reads in no fragment."""
    nreads = int(rng.integers(2, 7))
    n = int(rng.integers(0, (9, 13, 13, 40, max_hits + 1)[int(rng.integers(0, 5))]))
    ts = np.array([0, 40, 200])[rng.integers(0, 3, n)] + 5 * rng.integers(0, 3, n)
    ln = rng.choice([0, 20, 20, 30], n)
    i = rng.integers(0, nreads, n)
    hits = dict(i=i, j=rng.integers(0, int(rng.integers(1, 3)), n), reverse=np.where(rng.random(n) < 0.75, i % 2, 1 - i % 2), score=-rng.integers(0, 9, n),
                status=(rng.random(n) < 0.15).astype(np.int32) * rng.integers(1, 3, n), text_start=ts, text_end=ts + ln)
    if rng.random() < 0.5:
        mates = int(rng.integers(0, nreads // 2 + 1))
    else:
        perm = rng.permutation(nreads)
        nfrag = int(rng.integers(0, nreads // 2 + 1))
        mates = perm[:2 * nfrag].reshape(nfrag, 2)
    par = dict(min_score=int(rng.choice([INT32_MIN, INT32_MIN, -6, -3])), full_gap=int(rng.choice([1, 3, 6, 24])),
               min_insert=int(rng.choice([0, 20, 40])), max_insert=int(rng.choice([40, 80, 1000])), unpaired=int(rng.choice([0, 0, 1, 2, 24])))
    return nreads, hits, mates, par


def pair_corpus(seed=11, nfrag=100):
    """Fragments over the three references of place_common.corpus (an exact 300-base repeat at refs[0][600:900] and
    refs[1][2500:2800]).  Fragment f is reads 2 f (mate 1) and 2 f + 1 (mate 2), 150 bases each, the outer distance from the left
    mate's first base to the right mate's last between 200 and 500; mutated at 3 % away from their ends.  For every fifth fragment mate 1 lies, with
    PAD bases on either side, inside a copy of the repeat and mate 2 in unique sequence next to that copy, on either side.  The
    fragment's forward mate is stored as it is, its reverse mate reverse-complemented; every second fragment is taken from the other strand (mate 1 is then the
    reverse mate).  Windows per read: its true locus padded by PAD, for mate 1 of a repeat fragment the same offset in the other
    copy, and a random place; in shuffled order.
    Returns refs, reads, the window list and per fragment (reference, left position, outer length, mate 1 is the right-hand mate,
    repeat fragment, (reference, position) of mate 1, of mate 2, and of mate 1's image in the other copy or None)."""
    refs, _, _, _ = corpus()
    rng = np.random.default_rng(seed)
    code = {c: k for k, c in enumerate(LETTERS)}
    bases = [np.array([code[c] for c in r]) for r in refs]
    copies = [((0, 600), (1, 2500)), ((1, 2500), (0, 600))]
    L = 150
    reads, rows, truth = [], [], []
    for f in range(nfrag):
        repeat = f % 5 == 0
        outer = int(rng.integers(200, 501))
        flip = f % 2 == 1                      # mate 1 is the right-hand (reverse-strand) mate
        if repeat:
            (r, c0), (r2, c2) = copies[int(rng.integers(0, 2))]
            m1 = c0 + PAD + int(rng.integers(0, 300 - L - 2 * PAD + 1))   # (its padded window lies inside the copy too)
            # mate 2 wholly outside the copy (and outside the near-repeat of refs[1][800:1100], far from here): right of it when mate 1
            # is the left-hand mate, left of it otherwise
            if not flip:
                outer = max(outer, c0 + 300 - m1 + L)
                left = m1
            else:
                outer = max(outer, m1 + L - c0 + L)
                left = m1 + L - outer
            image = (r2, c2 + (m1 - c0))
        else:
            r = int(rng.integers(0, 3))
            left = int(rng.integers(0, len(bases[r]) - outer + 1))
            image = None
        pos_l, pos_r = left, left + outer - L
        pos1, pos2 = (pos_r, pos_l) if flip else (pos_l, pos_r)
        for pos, right_hand in ((pos1, flip), (pos2, not flip)):
            b = bases[r][pos:pos + L]
            s = "".join(LETTERS[np.r_[b[:EDGE], mutate(rng, b[EDGE:-EDGE], 0.03), b[-EDGE:]]])
            reads.append(revcomp(s) if right_hand else s)
        truth.append((r, left, outer, flip, repeat, (r, pos1), (r, pos2), image))
        for k, pos, right_hand, also in ((2 * f, pos1, flip, image), (2 * f + 1, pos2, not flip, None)):
            places = [(r, pos - PAD)] + ([(also[0], also[1] - PAD)] if also else [])
            rr = int(rng.integers(0, 3))
            places.append((rr, int(rng.integers(0, len(bases[rr]) - L))))
            for j, t0 in places:
                t0 = max(0, t0)
                t1 = min(len(refs[j]), t0 + L + 2 * PAD)
                rows.append((k, j, 0, len(reads[k]), t0, t1 - t0, int(right_hand)))
    rows = [rows[q] for q in rng.permutation(len(rows))]
    return refs, reads, as_list(rows), truth
