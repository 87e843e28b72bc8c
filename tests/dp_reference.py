"""A plain dynamic-programming aligner (test infrastructure): the optimum of the penalty model by the full O(plen x tlen)
recurrence, and a pricer of op strings.  It knows nothing of wavefronts, offsets, rings, int16 rows, trimming or breakpoints, so
an error that oracle/wfa_oracle.c and the kernels share does not reach it.

    dp_cost(batch, cfg)          optimal penalty per pair, int64
    price_ops(ops, p, t, cfg)    (ok, penalty) of one op string
    penalty_of_score(score, cfg) the penalty a reported score stands for (include/wfa_hip.h: indel and edit report +s, the
                                 other metrics report the classical score, which is -s with match == 0)

The model (cfg is a Config of oracle/loader.py or pywfa_amd/_native.py):
 * metrics: indel (no X; I and D cost 1), edit (X, I, D cost 1), gap-linear (X = mismatch, a gap of n costs n * gap_extension),
   gap-affine (o + n e) and gap-affine two-piece (min(o1 + n e1, o2 + n e2));
 * a cell matches when the two letters are equal or either one is the wildcard byte;
 * end-to-end: from (0, 0) to (plen, tlen);
 * ends-free: cells (v, 0), v <= pattern_begin_free, and (0, h), h <= text_begin_free, cost 0; the result is the minimum over the
   cells (v, tlen) with plen - v <= pattern_end_free and (plen, h) with tlen - h <= text_end_free.  The free-end sizes are read
   only when the span is ends-free;
 * match < 0 (gap-linear, gap-affine, two-piece): every matched base earns -match and the "penalty" is minus the maximal
   classical score.  End-to-end only: with free ends the reference minimises its internal score over end cells of different
   v + h, which is not the maximum of the classical score, and with free begins its own results are undefined
   (tests/test_oracle_vs_ref.py) — ValueError here.

Everything is int64.  The recurrence is batched over pairs and swept over anti-diagonals; the pairs of a batch are padded to a
common shape with letters that never match (and are no wildcard), which changes no cell inside a pair's own rectangle.
"""
import numpy as np

INDEL, EDIT, LINEAR, AFFINE, AFFINE2P = 0, 1, 2, 3, 4
INT32_MIN = -2147483648
INF = np.int64(1) << 40
_PAD_P, _PAD_T = 256, 257   # (int16 letters: outside the bytes, different from each other)


class Model:
    """The penalty model of a configuration: match (<= 0), x (None: no X op), the gap pieces [(o, e), ...], the four free-end sizes
    (pattern begin / end, text begin / end) and the wildcard byte (-1: none)."""

    def __init__(self, cfg):
        d = cfg.distance
        if d == INDEL:
            self.match, self.x, self.pieces = 0, None, [(0, 1)]
        elif d == EDIT:
            self.match, self.x, self.pieces = 0, 1, [(0, 1)]
        elif d == LINEAR:
            self.match, self.x, self.pieces = int(cfg.match), int(cfg.mismatch), [(0, int(cfg.gap_extension))]
        elif d == AFFINE:
            self.match, self.x, self.pieces = int(cfg.match), int(cfg.mismatch), [(int(cfg.gap_opening), int(cfg.gap_extension))]
        elif d == AFFINE2P:
            self.match, self.x = int(cfg.match), int(cfg.mismatch)
            self.pieces = [(int(cfg.gap_opening), int(cfg.gap_extension)), (int(cfg.gap_opening2), int(cfg.gap_extension2))]
        else:
            raise ValueError(f"distance {d}")
        self.free = (int(cfg.pattern_begin_free), int(cfg.pattern_end_free), int(cfg.text_begin_free), int(cfg.text_end_free)) \
            if cfg.span == 1 else (0, 0, 0, 0)
        self.wildcard = int(cfg.wildcard)
        self.distance = d
        if self.match < 0 and any(self.free):
            raise ValueError("match < 0 with free ends is outside the recurrence (it stays with the oracle)")

    def gap(self, n):
        """The price of gaps of n > 0 ops (array or int)."""
        n = np.asarray(n, np.int64)
        cost = None
        for o, e in self.pieces:
            c = o + e * n
            cost = c if cost is None else np.minimum(cost, c)
        return cost


def penalty_of_score(score, cfg):
    return int(score) if cfg.distance <= EDIT else -int(score)


def _letters(batch, i, which):
    off, ln = int(batch[which + "_off"][i]), int(batch[which + "_len"][i])
    return np.asarray(batch["seqs"][off:off + ln], np.uint8)


def dp_cost(batch, cfg):
    m = Model(cfg)
    n = len(batch["p_len"])
    if n == 0:
        return np.zeros(0, np.int64)
    plen = np.asarray(batch["p_len"], np.int64)
    tlen = np.asarray(batch["t_len"], np.int64)
    pbf, pef, tbf, tef = m.free
    if (plen < max(pbf, pef)).any() or (tlen < max(tbf, tef)).any():
        raise ValueError("free ends larger than a sequence")
    P, T = int(plen.max()), int(tlen.max())
    # row letters: pat[:, i] is the letter of matrix row i >= 1; column letters reversed: txt[:, T - j] is the letter of column
    # j >= 1, so that along an anti-diagonal (j = d - i) both are read with rising i
    pat = np.full((n, P + 1), _PAD_P, np.int16)
    txt = np.full((n, T + 1), _PAD_T, np.int16)
    for i in range(n):
        pat[i, 1:1 + plen[i]] = _letters(batch, i, "p")
        if tlen[i]:
            txt[i, T - tlen[i]:T] = _letters(batch, i, "t")[::-1]
    wild = m.wildcard >= 0
    if wild:
        pat_w, txt_w = pat == m.wildcard, txt == m.wildcard
    x_cost = INF if m.x is None else np.int64(m.x)
    match_cost = np.int64(m.match)
    npc = len(m.pieces)
    # three anti-diagonals of H and two of every gap matrix, indexed by row i + 1; column 0 stays INF (row -1)
    H = [np.full((n, P + 2), INF, np.int64) for _ in range(3)]
    D = [[np.full((n, P + 2), INF, np.int64) for _ in range(2)] for _ in range(npc)]   # gaps that consume the pattern
    I = [[np.full((n, P + 2), INF, np.int64) for _ in range(2)] for _ in range(npc)]   # gaps that consume the text
    last_row = np.full((n, T + 1), INF, np.int64)   # H(plen, j)
    last_col = np.full((n, P + 1), INF, np.int64)   # H(i, tlen)
    rows = np.arange(n)

    def record(h, d):
        j = d - plen
        sel = (j >= 0) & (j <= tlen)
        last_row[rows[sel], j[sel]] = h[rows[sel], plen[sel] + 1]
        i = d - tlen
        sel = (i >= 0) & (i <= plen)
        last_col[rows[sel], i[sel]] = h[rows[sel], i[sel] + 1]

    H[0][:, 1] = 0
    record(H[0], 0)
    for d in range(1, P + T + 1):
        lo, hi = max(0, d - T), min(d, P)
        h2, h1, h0 = H[(d - 2) % 3], H[(d - 1) % 3], H[d % 3]
        up, left, cur = slice(lo, hi + 1), slice(lo + 1, hi + 2), slice(lo + 1, hi + 2)
        if lo >= 1:
            # (rows below the sweep hold what the diagonal three back left there: they are never read again — up and the diagonal
            # move read rows >= lo - 1, which the two diagonals before this one own — but keep them INF all the same)
            h0[:, max(0, lo - 2):lo + 1] = INF
        eq = pat[:, lo:hi + 1] == txt[:, T - d + lo:T - d + hi + 1]
        if wild:
            eq |= pat_w[:, lo:hi + 1]
            eq |= txt_w[:, T - d + lo:T - d + hi + 1]
        best = h2[:, up] + np.where(eq, match_cost, x_cost)
        for k, (o, e) in enumerate(m.pieces):
            d1, d0 = D[k][(d - 1) % 2], D[k][d % 2]
            i1, i0 = I[k][(d - 1) % 2], I[k][d % 2]
            # (d1 / i1 are read before d0 / i0, which alias nothing: two buffers, and up / left of the previous diagonal only)
            dn = np.minimum(h1[:, up] + (o + e), d1[:, up] + e)
            inn = np.minimum(h1[:, left] + (o + e), i1[:, left] + e)
            if lo >= 1:
                d0[:, max(0, lo - 1):lo + 1] = INF
                i0[:, max(0, lo - 1):lo + 1] = INF
            d0[:, cur] = dn
            i0[:, cur] = inn
            np.minimum(best, dn, out=best)
            np.minimum(best, inn, out=best)
        h0[:, cur] = best
        if d <= P and d <= pbf:
            h0[:, d + 1] = 0
        if d <= T and d <= tbf:
            h0[:, 1] = 0
        record(h0, d)
    if cfg.span != 1:
        return last_row[rows, tlen]
    ci = np.arange(P + 1)[None, :]
    col_ok = (ci <= plen[:, None]) & (plen[:, None] - ci <= pef)
    cj = np.arange(T + 1)[None, :]
    row_ok = (cj <= tlen[:, None]) & (tlen[:, None] - cj <= tef)
    return np.minimum(np.where(col_ok, last_col, INF).min(axis=1), np.where(row_ok, last_row, INF).min(axis=1))


def _bytes(x):
    if isinstance(x, str):
        x = x.encode("ascii")
    return np.frombuffer(bytes(x), np.uint8) if not isinstance(x, np.ndarray) else x.astype(np.uint8, copy=False)


def price_ops(ops, p, t, cfg, want_gaps=False):
    """(ok, penalty) of the op string `ops` (chars M X I D) for pattern `p` against text `t`.  ok: M only on cells that match, X
    only on cells that do not (never under indel), D consumes the pattern, I the text, both consumed exactly — the library writes
    free ends as leading / trailing D / I runs.  penalty: every maximal gap run priced as one gap; of a leading D (I) run up to
    pattern_begin_free (text_begin_free) ops are free, of a trailing one up to pattern_end_free (text_end_free), both when one
    run is the whole string; what is left of such a run is charged as one gap.  penalty is None when not ok."""
    m = Model(cfg)
    ops, p, t = _bytes(ops), _bytes(p), _bytes(t)
    is_m, is_x, is_i, is_d = (ops == ord(c) for c in "MXID")
    if not (is_m | is_x | is_i | is_d).all():
        return False, None
    on_p, on_t = is_m | is_x | is_d, is_m | is_x | is_i
    if int(on_p.sum()) != len(p) or int(on_t.sum()) != len(t):
        return False, None
    v = np.cumsum(on_p) - on_p
    h = np.cumsum(on_t) - on_t
    sub = is_m | is_x
    a, b = p[v[sub]], t[h[sub]]
    eq = a == b
    if m.wildcard >= 0:
        eq |= (a == m.wildcard) | (b == m.wildcard)
    if (eq != is_m[sub]).any():
        return False, None
    if m.x is None and is_x.any():
        return False, None
    penalty = m.match * int(is_m.sum()) + (0 if m.x is None else m.x * int(is_x.sum()))
    if len(ops) == 0:
        return (True, penalty, np.zeros(0, np.int64)) if want_gaps else (True, penalty)
    start = np.concatenate(([0], np.flatnonzero(ops[1:] != ops[:-1]) + 1))
    length = np.diff(np.concatenate((start, [len(ops)]))).astype(np.int64)
    code = ops[start]
    pbf, pef, tbf, tef = m.free
    for at, d_free, i_free in ((0, pbf, tbf), (len(code) - 1, pef, tef)):
        allow = d_free if code[at] == ord("D") else i_free if code[at] == ord("I") else 0
        length[at] -= min(int(length[at]), allow)
    gaps = length[((code == ord("D")) | (code == ord("I"))) & (length > 0)]
    if gaps.size:
        penalty += int(m.gap(gaps).sum())
    if want_gaps:
        return True, penalty, gaps
    return True, penalty


def two_piece_slack(ops, p, t, cfg):
    """Every amount by which a wavefront walk of the valid op string `ops` can cost more than price_ops says under gap-affine
    two-piece: the model prices a gap by its cheaper piece, a walk pays the piece whose component it went through.  A set of
    ints holding 0."""
    m = Model(cfg)
    _, _, gaps = price_ops(ops, p, t, cfg, want_gaps=True)
    sums = {0}
    if len(m.pieces) == 2:
        (o1, e1), (o2, e2) = m.pieces
        for n in gaps:
            d = abs((o1 + e1 * int(n)) - (o2 + e2 * int(n)))
            sums |= {s + d for s in sums}
    return sums


def faults(cfg, p, t, cost, score, ops=None, unset_ok=False):
    """What is wrong with one completed result, given the recurrence's `cost` of the pair: a list of findings, empty when the
    score stands for that cost and the op string (if there is one) is an alignment of the pair at that price.  unset_ok: a score
    of INT32_MIN is no finding (BiWFA leaves it unset where the top level never splits)."""
    out = []
    if not (unset_ok and score == INT32_MIN) and penalty_of_score(score, cfg) != cost:
        out.append(f"score {score} stands for penalty {penalty_of_score(score, cfg)}, the optimum is {cost}")
    if ops is not None:
        ok, price = price_ops(ops, p, t, cfg)
        if not ok:
            out.append("the op string is no alignment of the pair")
        elif price != cost:
            out.append(f"the op string costs {price}, the optimum is {cost}")
    return out


def ops_of(cig, i):
    """Op string i of an (ops, begin, len) triple of the bindings."""
    ops, cbeg, clen = cig
    return ops[cbeg[i]:cbeg[i] + clen[i]].tobytes()
