"""What a lane stage with a band of 2 H diagonals (wfa_lane.hpp, NRP = H) keeps and what it hands on, on the host: the band rule in
closed form over oracle scores, and a banded gap-affine cost over many pairs at once (numpy) for the scores exactly at the bound.
Shared by tests/test_lane_width_model.py (CPU) and tests/test_lane_widths_gpu.py."""
import numpy as np

from pywfa_amd import datagen

INF = 1 << 28


def shape_of(x, o, e):
    """Penalties (mismatch, gap opening, gap extension) -> (g, X, OE, E), the kernels' penalty shape in units of the gcd."""
    g = int(np.gcd.reduce([x, o + e, e]))
    return g, x // g, (o + e) // g, e // g


def band(batch, H):
    """ak = tlen - plen, the band centre c = ceil(ak / 2), `bad` (the end diagonal lies outside k in [c - H, c + H))."""
    ak = np.asarray(batch["t_len"], dtype=np.int64) - np.asarray(batch["p_len"], dtype=np.int64)
    c = (ak + 1) >> 1
    return ak, c, (ak < 1 - 2 * H) | (ak > 2 * H - 1)


def deadline(ak, c, H, OE, E):
    """Bmin / g: a score is kept at step s <= min(2 (OE - E) + E (2c + 2H - ak), 2 (OE - E) + E (2H + 2 - 2c + ak))."""
    return np.minimum(2 * (OE - E) + E * (2 * c + 2 * H - ak), 2 * (OE - E) + E * (2 * H + 2 - 2 * c + ak))


def banded_costs(batch, idx, lo, hi, x, o, e):
    """Gap-affine (Gotoh) cost of the best alignment of each pair idx[i] whose cells stay on diagonals lo[i] <= h - v < hi[i] — the same
    recurrence as test_lane_narrow_gpu.banded_cost, all pairs at once, one numpy operation per row and band slot."""
    idx = np.asarray(idx, dtype=np.int64)
    lo = np.asarray(lo, dtype=np.int64)
    n = len(idx)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    wd = int(np.max(np.asarray(hi, dtype=np.int64) - lo))
    assert np.all(np.asarray(hi, dtype=np.int64) - lo == wd)
    pl = np.asarray(batch["p_len"], dtype=np.int64)[idx]
    tl = np.asarray(batch["t_len"], dtype=np.int64)[idx]
    pmax, tmax = int(pl.max()), int(tl.max())
    seqs = np.asarray(batch["seqs"])
    P = np.full((n, pmax + 1), 254, dtype=np.uint8)
    T = np.full((n, tmax + 1), 255, dtype=np.uint8)
    po = np.asarray(batch["p_off"], dtype=np.int64)[idx]
    to = np.asarray(batch["t_off"], dtype=np.int64)[idx]
    for i in range(n):   # (row i: the pair's bases, 1-based: column v holds base v - 1)
        P[i, 1:pl[i] + 1] = seqs[po[i]:po[i] + pl[i]]
        T[i, 1:tl[i] + 1] = seqs[to[i]:to[i] + tl[i]]
    rows = np.arange(n)
    # slot j of row v is the cell (v, h = v + lo + j); one slot of padding on either side stays INF
    Mp = np.full((n, wd + 2), INF, dtype=np.int64)
    Dp = np.full((n, wd + 2), INF, dtype=np.int64)
    out = np.full(n, INF, dtype=np.int64)
    for v in range(pmax + 1):
        Mc = np.full((n, wd + 2), INF, dtype=np.int64)
        Ic = np.full((n, wd + 2), INF, dtype=np.int64)
        Dc = np.full((n, wd + 2), INF, dtype=np.int64)
        for j in range(wd):
            h = v + lo + j
            ok = (h >= 0) & (h <= tl) & (v <= pl)
            ins = np.minimum(Mc[:, j] + o + e, Ic[:, j] + e)            # from (v, h - 1): slot j - 1 of this row
            dele = np.minimum(Mp[:, j + 2] + o + e, Dp[:, j + 2] + e)   # from (v - 1, h): slot j + 1 of the row above
            hc = np.clip(h, 0, tmax)
            sub = Mp[:, j + 1] + np.where(P[:, v] == T[rows, hc], 0, x) if v > 0 else np.full(n, INF, dtype=np.int64)
            sub = np.where(h >= 1, sub, INF)
            m = np.minimum(np.minimum(sub, ins), dele)
            m = np.where((h == 0) & (v == 0), 0, m)
            Mc[:, j + 1] = np.where(ok, np.minimum(m, INF), INF)
            Ic[:, j + 1] = np.where(ok & ~((h == 0) & (v == 0)), np.minimum(ins, INF), INF)
            Dc[:, j + 1] = np.where(ok & ~((h == 0) & (v == 0)), np.minimum(dele, INF), INF)
            out = np.where((v == pl) & (h == tl), Mc[:, j + 1], out)
        Mp, Dp = Mc, Dc
    return out


def handed_mask(batch, score, H, x, o, e, exact_ties=True):
    """True for the pairs a lane stage with 2 H diagonals hands on: the end diagonal outside the band, an oracle score beyond the
    deadline, or (exact_ties) one exactly at the deadline whose every optimal alignment leaves the band.  Without exact_ties a score
    at the deadline counts as kept (the closed form the pilot's count uses)."""
    g, X, OE, E = shape_of(x, o, e)
    ak, c, bad = band(batch, H)
    dl = deadline(ak, c, H, OE, E)
    steps = -np.asarray(score, dtype=np.int64) // g
    handed = bad | (steps > dl)
    if exact_ties:
        ties = np.flatnonzero(~bad & (steps == dl))
        cost = banded_costs(batch, ties, c[ties] - H, c[ties] + H, x, o, e)
        handed[ties[cost > g * steps[ties]]] = True
    return handed


def pair(batch, i):
    return datagen.pair_strings(batch, int(i))
