"""Shared by the tests of duplicates on unclipped ends and of the representative by base quality (test_dup_ends_abi.py,
test_dup_ends_gpu.py): the "clips" paragraph and the two flags of "duplicates" (include/wfa_hip.h) restated in plain Python from the
header's text, on top of pair_common.py_pair and next to dup_common.py_duplicates, and a generator of random cases in which every new
clause occurs."""
import numpy as np

from dup_common import HIT_KEYS, MAX_BUCKET
from pair_common import INT32_MIN, fragments, py_pair

CLIP_MAX = 65535
INT32_MAX = 2**31 - 1
UNCLIPPED, BY_QUALITY = 1, 2
NEW_CLAUSES = ("only_unclipped", "only_core", "b_negative", "b_past_text", "rev_joined_by_trail", "pair_joined_by_lead_and_trail",
               "rep_differs", "quality_tie")


def py_clips(ops, plen, tlen):
    """(lead, trail) of one op string: the X and D ops in front of the first and behind the last M, saturated; 0, 0 without an M or for
    an empty pair."""
    ops = bytes(ops)
    if not ops or plen == 0 or tlen == 0 or b"M" not in ops:
        return 0, 0
    first, last = ops.index(b"M"), ops.rindex(b"M")
    lead = sum(1 for c in ops[:first] if c in b"XD")
    trail = sum(1 for c in ops[last + 1:] if c in b"XD")
    return min(lead, CLIP_MAX), min(trail, CLIP_MAX)


def py_qsum(quals, min_quality):
    return min(sum(int(q) for q in quals if int(q) >= min_quality), INT32_MAX)


def _units(hits, nreads, mates, par, lead, trail, unclipped, qsum):
    """The units of the rule as dicts: pair (bool), number, j, b, key (the rest of the key), score, and, for the clause counters, the
    score by alignment, the clips that entered the key and whether the key coordinates fit int32."""
    rows, _, pair_rows, _ = py_pair(hits, nreads, mates, par["min_score"], par["full_gap"], par["min_insert"], par["max_insert"], par["unpaired"])
    n = len(hits["i"])
    rev = hits["reverse"] if hits.get("reverse") is not None else [0] * n
    J, TS, TE = hits["j"], hits["text_start"], hits["text_end"]
    cl = (lambda c, h: min(int(c[h]), CLIP_MAX) if unclipped and c is not None else 0)
    us = lambda h: int(TS[h]) - cl(lead, h)
    ue = lambda h: int(TE[h]) + cl(trail, h)
    frags = fragments(mates, nreads)
    units, owned = [], set()
    for f, (m1, m2) in enumerate(frags):
        if int(pair_rows[f][2]) != 1:
            continue
        owned |= {m1, m2}
        h, g = int(pair_rows[f][0]), int(pair_rows[f][1])
        F, R, first = (h, g, 1) if not rev[h] else (g, h, 2)
        by_score = int(pair_rows[f][3])
        score = min(int(qsum[m1]) + int(qsum[m2]), INT32_MAX) if qsum is not None else by_score
        units.append(dict(pair=True, unit=f, j=int(J[F]), b=us(F), key=(ue(R), first), score=score, by_score=by_score,
                          clips=(cl(lead, F), cl(trail, R)), fits=ue(R) <= INT32_MAX))
    for r in range(nreads):
        if r in owned:
            continue
        h = int(rows[r][0])
        if h < 0 or int(TE[h]) <= int(TS[h]):
            continue
        rv = 1 if rev[h] else 0
        by_score = int(rows[r][1])
        units.append(dict(pair=False, unit=r, j=int(J[h]), b=ue(h) - 1 if rv else us(h), key=(rv,), score=int(qsum[r]) if qsum is not None else by_score,
                          by_score=by_score, clips=(cl(lead, h), cl(trail, h)), fits=True))
    return units, frags


def _groups(units, text_len):
    """[(members, alone, overflow)]: the groups of the units, bucket by bucket."""
    buckets = {}
    lone = []
    for u in units:
        if not u["fits"]:
            lone.append(([u], True, False))
        else:
            buckets.setdefault((u["j"], u["b"]), []).append(u)
    out = lone
    for (j, b), members in buckets.items():
        outside = not 0 <= b < int(text_len[j])
        overflow = not outside and len(members) > MAX_BUCKET
        groups = {}
        for u in members:
            groups.setdefault((u["pair"], u["key"]), []).append(u)
        out += [(g, outside or overflow, overflow) for g in groups.values()]
    return out


def py_duplicates_ex(hits, nreads, mates, par, text_len, lead=None, trail=None, flags=0, qsum=None, seen=None):
    """(read_rows, pair_rows) of the rule under `flags`; `qsum`: one int per read, used under BY_QUALITY.  `seen` counts the new clauses
    (NEW_CLAUSES)."""
    seen = seen if seen is not None else {}
    for k in NEW_CLAUSES:
        seen.setdefault(k, 0)
    unclipped, by_quality = bool(flags & UNCLIPPED), bool(flags & BY_QUALITY)
    units, frags = _units(hits, nreads, mates, par, lead, trail, unclipped, qsum if by_quality else None)
    groups = _groups(units, text_len)
    read_rows = np.tile(np.array([-1, 0, 0, 0], np.int32), (nreads, 1))
    frag_rows = np.tile(np.array([-1, 0, 0, 0], np.int32), (len(frags), 1))
    for group, alone, overflow in groups:
        best = min(group, key=lambda u: (-u["score"], u["unit"]))
        for u in group:
            rep, size = (u["unit"], 1) if alone else (best["unit"], len(group))
            row = [rep, size, int(rep != u["unit"]), int(overflow)]
            if u["pair"]:
                frag_rows[u["unit"]] = row
                for m in frags[u["unit"]]:
                    read_rows[m] = [-1, 0, row[2], row[3]]
            else:
                read_rows[u["unit"]] = row
        if by_quality and len(group) > 1 and not alone:
            seen["rep_differs"] += int(min(group, key=lambda u: (-u["by_score"], u["unit"]))["unit"] != best["unit"])
            seen["quality_tie"] += int(sum(1 for u in group if u["score"] == best["score"]) > 1)
    if unclipped:
        for u in units:
            seen["b_negative"] += int(u["fits"] and u["b"] < 0)
            seen["b_past_text"] += int(u["fits"] and u["b"] >= int(text_len[u["j"]]))
        name = lambda g: (g[0]["pair"], frozenset(u["unit"] for u in g))
        mine = {name(g): g for g, alone, _ in groups if len(g) > 1 and not alone}
        core = {name(g) for g, alone, _ in _groups(_units(hits, nreads, mates, par, lead, trail, False, None)[0], text_len) if len(g) > 1 and not alone}
        seen["only_core"] += len(core - set(mine))
        for k, g in mine.items():
            if k in core:
                continue
            seen["only_unclipped"] += 1
            if g[0]["pair"]:
                seen["pair_joined_by_lead_and_trail"] += int(any(u["clips"][0] > 0 for u in g) and any(u["clips"][1] > 0 for u in g))
            elif g[0]["key"] == (1,):
                seen["rev_joined_by_trail"] += int(any(u["clips"][1] > 0 for u in g))
    return read_rows, frag_rows


def random_ends_case(rng, max_reads=24):
    """(nreads, hits, mates, par, text_len, lead, trail, flags, qsum): the hit lists of dup_common.random_dup_case on texts of 25, 70
    and 250 bases (reads <= 64, texts <= 256 bases) with clips 0 .. 5.  A forward hit is moved up to 3 bases to the right and a
    reverse hit up to 3 to the left, and most of the time the clip is exactly that shift, so that the unclipped ends collide where the
    cores do not, and the other way round; a start at 0 with a lead lies in front of its text, a reverse hit that ends with its text
    and has a trail lies behind it; the choice is made per read pair, so that both ends of a fragment keep their unclipped place.  Quality sums from three values, so that ties are frequent and the order by quality differs from
    the order by score; every flag combination."""
    nreads = int(rng.integers(2, max_reads + 1))
    text_len = rng.choice([25, 70, 250], 2).astype(np.int32)
    i = np.repeat(np.arange(nreads), rng.choice([0, 1, 1, 1, 2], nreads))
    i = i[rng.permutation(len(i))]
    n = len(i)
    j = rng.integers(0, 2, n) if rng.random() < 0.3 else np.zeros(n, np.int64)
    flip = rng.random(nreads // 2 + 1) < 0.3          # reads 2 f and 2 f + 1 swap strands
    reverse = np.where(rng.random(n) < 0.9, (i + flip[i // 2]) % 2, rng.integers(0, 2, n))
    ln = rng.choice([0, 20, 20, 20, 30], n)
    te_r = np.where(rng.random(n) < 0.4, text_len[j], rng.choice([60, 70], n))
    ln = np.minimum(ln, te_r)
    ts = np.where(reverse == 1, te_r - ln, rng.choice([0, 10, 10, 40], n)).astype(np.int64)
    rv = reverse == 1
    shift = rng.choice([0, 0, 0, 1, 2, 3], n)
    shift = np.where(rv & (ts - shift < 0), 0, shift)
    ts = np.where(rv, ts - shift, ts + shift)
    same = (rng.random(nreads // 2 + 1) < 0.6)[i // 2] | (rng.random(n) < 0.3)   # (mostly both mates of an interleaved fragment)
    lead = np.where(~rv & same, shift, rng.choice([0, 0, 1, 2, 5], n))
    trail = np.where(rv & same, shift, rng.choice([0, 0, 1, 2, 5], n))
    hits = dict(i=i, j=j, reverse=reverse, score=-rng.integers(0, 3, n), status=(rng.random(n) < 0.05).astype(np.int32),
                text_start=ts, text_end=ts + ln)
    if rng.random() < 0.5:
        mates = int(rng.integers(0, nreads // 2 + 1))
    else:
        nfrag = int(rng.integers(0, nreads // 2 + 1))
        mates = rng.permutation(nreads)[:2 * nfrag].reshape(nfrag, 2)
    par = dict(min_score=int(rng.choice([INT32_MIN, INT32_MIN, -1])), full_gap=int(rng.choice([1, 6, 24])),
               min_insert=int(rng.choice([0, 20])), max_insert=int(rng.choice([80, 1000])), unpaired=int(rng.choice([0, 2, 24])))
    flags = int(rng.integers(0, 4))
    qsum = rng.choice([0, 600, 600, 1200], nreads).astype(np.int32)
    return nreads, hits, mates, par, text_len, lead.astype(np.int32), trail.astype(np.int32), flags, qsum


def sized_ends_case(rng, hits):
    """lead and trail for the hits of dup_common.sized_dup_case, and the hits moved by them the way random_ends_case moves them; one
    hit in fifty carries a clip at or above the cap."""
    n = len(hits["i"])
    ts, te, rv = hits["text_start"].astype(np.int64), hits["text_end"].astype(np.int64), np.asarray(hits["reverse"]) != 0
    shift = rng.choice([0, 0, 1, 2], n)
    shift = np.where(rv & (ts - shift < 0), 0, shift)
    ts, te = np.where(rv, ts - shift, ts + shift), np.where(rv, te - shift, te + shift)
    lead = np.where(~rv, shift, rng.integers(0, 3, n))
    trail = np.where(rv, shift, rng.integers(0, 3, n))
    big = rng.random(n) < 0.02
    lead = np.where(big, rng.choice([CLIP_MAX, CLIP_MAX + 1, 1 << 20], n), lead)
    trail = np.where(big, rng.choice([CLIP_MAX, CLIP_MAX + 1, 1 << 20], n), trail)
    out = {k: np.asarray(hits[k]) for k in HIT_KEYS}
    out.update(text_start=ts.astype(np.int32), text_end=te.astype(np.int32))
    return out, lead.astype(np.int32), trail.astype(np.int32)
