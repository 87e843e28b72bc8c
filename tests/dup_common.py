"""Shared by the duplicate-marking tests (test_dup_abi.py, test_dup_gpu.py): the rule of include/wfa_hip.h ("duplicates") restated in
plain Python from the header's text on top of pair_common.py_pair, and a generator of random hit lists in which every clause of the
rule occurs."""
import numpy as np

from pair_common import INT32_MIN, fragments, py_pair

DUP_COLUMNS = ("rep", "size", "dup", "overflow")
MAX_BUCKET = 4096
HIT_KEYS = ("i", "j", "reverse", "score", "status", "text_start", "text_end")
CLAUSES = ("pair_group", "score_tie", "other_first", "other_end", "fwd_group", "rev_group_lens", "mixed_bucket", "nonproper_mate",
           "no_fragment", "no_hit", "empty", "outside", "rev_at_tlen", "pos0")


def py_duplicates(hits, nreads, mates, par, text_len, seen=None):
    """(read_rows, pair_rows) of the rule: int32 of shape (nreads, 4) and (F, 4).  `par`: the parameters of py_pair.  `seen`, a dict,
    counts how often each clause occurred (CLAUSES)."""
    seen = seen if seen is not None else {}
    for k in CLAUSES:
        seen.setdefault(k, 0)
    rows, _, pair_rows, _ = py_pair(hits, nreads, mates, par["min_score"], par["full_gap"], par["min_insert"], par["max_insert"], par["unpaired"])
    n = len(hits["i"])
    rev = hits["reverse"] if hits.get("reverse") is not None else [0] * n
    J, TS, TE = hits["j"], hits["text_start"], hits["text_end"]
    frags = fragments(mates, nreads)
    read_rows = np.tile(np.array([-1, 0, 0, 0], np.int32), (nreads, 1))
    frag_rows = np.tile(np.array([-1, 0, 0, 0], np.int32), (len(frags), 1))
    units = []    # (pair unit?, number, j, b, the rest of the key, score)
    owned, in_fragment = set(), set()
    for f, (m1, m2) in enumerate(frags):
        in_fragment |= {m1, m2}
        if int(pair_rows[f][2]) != 1:
            continue
        owned |= {m1, m2}
        h, g = int(pair_rows[f][0]), int(pair_rows[f][1])
        F, R, first = (h, g, 1) if not rev[h] else (g, h, 2)
        units.append((True, f, int(J[F]), int(TS[F]), (int(TE[R]), first), int(pair_rows[f][3])))
    for r in range(nreads):
        if r in owned:
            continue
        h = int(rows[r][0])
        if h < 0:
            seen["no_hit"] += 1
            continue
        if int(TE[h]) <= int(TS[h]):
            seen["empty"] += 1
            continue
        seen["nonproper_mate" if r in in_fragment else "no_fragment"] += 1
        rv = 1 if rev[h] else 0
        seen["rev_at_tlen"] += int(rv == 1 and int(TE[h]) == int(text_len[int(J[h])]))
        units.append((False, r, int(J[h]), int(TE[h]) - 1 if rv else int(TS[h]), (rv, int(TE[h]) - int(TS[h])), int(rows[r][1])))
    buckets = {}
    for u in units:
        buckets.setdefault((u[2], u[3]), []).append(u)
    for (j, b), members in buckets.items():
        outside = not 0 <= b < int(text_len[j])
        overflow = not outside and len(members) > MAX_BUCKET
        seen["outside"] += int(outside) * len(members)
        seen["pos0"] += int(b == 0) * len(members)
        seen["mixed_bucket"] += int(len({u[0] for u in members}) == 2)
        pair_keys = {u[4] for u in members if u[0]}
        seen["other_end"] += int(len({k[0] for k in pair_keys}) > 1)
        seen["other_first"] += int(any((te, 3 - first) in pair_keys for te, first in pair_keys))
        groups = {}
        for u in members:   # (a read unit's key is its strand alone: its length is kept for the clause counter)
            groups.setdefault((u[0], u[4] if u[0] else u[4][0]), []).append(u)
        for (is_pair, key), group in groups.items():
            best = min(group, key=lambda u: (-u[5], u[1]))
            if len(group) > 1 and not outside and not overflow:
                seen["pair_group" if is_pair else "rev_group_lens" if key == 1 and len({u[4][1] for u in group}) > 1 else "fwd_group"] += 1
                seen["score_tie"] += int(sum(1 for u in group if u[5] == best[5]) > 1)
            for u in group:
                alone = outside or overflow
                rep, size = (u[1], 1) if alone else (best[1], len(group))
                row = [rep, size, int(rep != u[1]), int(overflow)]
                if u[0]:
                    frag_rows[u[1]] = row
                    for m in frags[u[1]]:
                        read_rows[m] = [-1, 0, row[2], row[3]]
                else:
                    read_rows[u[1]] = row
    return read_rows, frag_rows


def random_dup_case(rng, max_reads=24):
    """(nreads, hits, mates, par, text_len): 2 .. max_reads reads with 0 .. 2 hits each on two texts whose lengths are drawn from 25,
    70 and 300.  A forward hit starts at 0, 10 or 40 and a reverse hit ends at 60, 70 or the end of its text, with 0, 20, 20 or 30
    bases, so that starts, ends and 5' ends collide all the time, reverse reads of different lengths share an end, a start can lie
    behind a 25-base text, and a reverse hit can end at the end of its text; a read's hits are mostly on the strand of its parity,
    swapped for three in ten of the read pairs (2 f, 2 f + 1), so that interleaved fragments are proper with either mate forward;
    scores from a small range, so that ties are frequent.  The fragments interleaved (an int) or a shuffled (F, 2) array, some
    reads in no fragment."""
    nreads = int(rng.integers(2, max_reads + 1))
    text_len = rng.choice([25, 70, 300], 2).astype(np.int32)
    i = np.repeat(np.arange(nreads), rng.choice([0, 1, 1, 1, 2], nreads))
    i = i[rng.permutation(len(i))]
    n = len(i)
    j = rng.integers(0, 2, n) if rng.random() < 0.3 else np.zeros(n, np.int64)
    flip = rng.random(nreads // 2 + 1) < 0.3          # reads 2 f and 2 f + 1 swap strands
    reverse = np.where(rng.random(n) < 0.9, (i + flip[i // 2]) % 2, rng.integers(0, 2, n))
    ln = rng.choice([0, 20, 20, 20, 30], n)
    te_r = np.where(rng.random(n) < 0.4, text_len[j], rng.choice([60, 70], n))
    ln = np.minimum(ln, te_r)
    ts = np.where(reverse == 1, te_r - ln, rng.choice([0, 10, 10, 40], n))
    hits = dict(i=i, j=j, reverse=reverse, score=-rng.integers(0, 3, n), status=(rng.random(n) < 0.05).astype(np.int32),
                text_start=ts, text_end=ts + ln)
    if rng.random() < 0.5:
        mates = int(rng.integers(0, nreads // 2 + 1))
    else:
        nfrag = int(rng.integers(0, nreads // 2 + 1))
        mates = rng.permutation(nreads)[:2 * nfrag].reshape(nfrag, 2)
    par = dict(min_score=int(rng.choice([INT32_MIN, INT32_MIN, -1])), full_gap=int(rng.choice([1, 6, 24])),
               min_insert=int(rng.choice([0, 20])), max_insert=int(rng.choice([80, 1000])), unpaired=int(rng.choice([0, 2, 24])))
    return nreads, hits, mates, par, text_len


def sized_dup_case(rng, nreads, text_len, spread=None):
    """(hits, mates) for the device kernels: `nreads` reads, interleaved fragments over the first 2 * (nreads // 3) of them and the rest
    in no fragment, on texts of the lengths `text_len`.  A fragment's mates lie 100 .. 160 bases apart with either mate forward, a
    single read on either strand, all 50 bases long; starts are drawn from `spread` places per text (None: every tenth base), so
    that groups of every size occur; a tenth of the reads have no hit, an ineligible one or an empty interval."""
    text_len = np.asarray(text_len, np.int64)
    nfrag = nreads // 3
    rows = []   # (i, j, reverse, score, status, ts, te)
    def start(j):
        room = max(1, int(text_len[j]) - 220)
        k = spread if spread else max(1, room // 10)
        return int(rng.integers(0, k)) * (room // k if room >= k else 1) % room
    for f in range(nfrag):
        j = int(rng.integers(0, len(text_len)))
        ts = start(j)
        side = int(rng.integers(0, 2))
        far = ts + int(rng.choice([100, 110, 160]))
        a = (2 * f, j, side, -int(rng.integers(0, 3)), 0, far if side else ts, (far if side else ts) + 50)
        b = (2 * f + 1, j, 1 - side, -int(rng.integers(0, 3)), 0, ts if side else far, (ts if side else far) + 50)
        kind = rng.random()
        if kind < 0.05:
            b = b[:4] + (1,) + b[5:]          # an ineligible mate: the other one is a read unit
        elif kind < 0.1:
            b = b[:6] + (b[5],)               # an empty interval
        rows += [a] if kind >= 0.97 else [a, b]
    for r in range(2 * nfrag, nreads):
        j = int(rng.integers(0, len(text_len)))
        ts = start(j)
        kind = rng.random()
        if kind < 0.04:
            continue
        ln = int(rng.choice([50, 50, 40]))
        rv = int(rng.integers(0, 2))
        ts = ts + 50 - ln if rv else ts        # (reverse reads of two lengths end at one base)
        rows.append((r, j, rv, -int(rng.integers(0, 3)), int(kind < 0.08), ts, ts + (0 if kind > 0.97 else ln)))
    rows = [rows[q] for q in rng.permutation(len(rows))]
    cols = list(zip(*rows)) if rows else [[]] * 7
    return {k: np.asarray(c, np.int32) for k, c in zip(HIT_KEYS, cols)}, nfrag


def as_arrays(hits):
    return [None if hits.get(k) is None else np.asarray(hits[k], np.uint8 if k == "reverse" else np.int32) for k in HIT_KEYS]
