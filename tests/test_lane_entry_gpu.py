"""The plain score-only lane kernel (wfa_lane.hpp) enters every pair at score K = o + e: the refill follows diagonal 0 through
the cells below K and writes down the state the loop would hold there.  Constructed pairs around every edge of that entry
(run lengths at the 16- and 32-base probe boundaries, the chain ending at lim, pairs that finish inside the chain, the first gap
cells at and outside the band's edge) for every built-in penalty shape and one run-time shape, a ragged corpus, and the
hand-over count of the 16-diagonal stage: always exact equality with the CPU oracle."""
import functools
import re

import numpy as np
import pytest

import common
from oracle import loader
from pywfa_amd import datagen

pytestmark = pytest.mark.gpu

# (mismatch, gap_opening, gap_extension) -> the lane kernel's shape (X, OE, E) in units of g: the seven built-in shapes in the
# order of affine_shapes (csrc/wfa_shapes.hpp), then one that is instantiated at run time
SHAPES = {
    "s0_2_4_1": (4, 6, 2),
    "s1_2_3_1": (2, 2, 1),
    "s2_4_7_1": (4, 6, 1),
    "s3_3_5_1": (3, 4, 1),
    "s4_6_8_3": (6, 5, 3),
    "s5_5_3_3": (5, 0, 3),
    "s6_1_2_1": (1, 1, 1),
    "rtc_5_8_2": (5, 6, 2),
}
STAGES = ("0", "1", "01", "0189", "189")
ACGT = "ACGT"


def seq(rng, n):
    """n bases, no two neighbours equal (so that an inserted or deleted base always ends the run on diagonal 0 where it is)."""
    out, prev = [], -1
    for _ in range(n):
        b = int(rng.integers(0, 4))
        if b == prev:
            b = (b + 1 + int(rng.integers(0, 3))) & 3
        out.append(b)
        prev = b
    return "".join(ACGT[b] for b in out)


def other(base, rng, avoid=""):
    choice = [c for c in ACGT if c != base and c not in avoid]
    return choice[int(rng.integers(0, len(choice)))]


def subst(s, positions, rng):
    s = list(s)
    for i in positions:
        s[i] = other(s[i], rng)
    return "".join(s)


@functools.lru_cache(maxsize=None)
def edge_pairs():
    rng = np.random.default_rng(20250)
    pairs = []
    # identical reads
    for L in (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 512):
        p = seq(rng, L)
        pairs.append((p, p))
    # one mismatch at the first / last base and around the probe boundaries
    for L in (1, 16, 17, 32, 33, 150):
        p = seq(rng, L)
        for at in sorted({0, L - 1, 15, 16, 17, 31, 32, 33}):
            if at < L:
                pairs.append((p, subst(p, [at], rng)))
    # a mismatch only at the last base, further lengths
    for L in (2, 64, 65, 512):
        p = seq(rng, L)
        pairs.append((p, subst(p, [L - 1], rng)))
    # two mismatches, adjacent and 32 apart; NCH + 1 and more (NCH <= 2 for every shape here): the chain ends, the loop carries on
    p = seq(rng, 150)
    for pos in ((40, 41), (0, 1), (148, 149), (10, 42), (0, 32), (31, 63), (117, 149),
                (5, 50, 100), (5, 6, 7), (0, 75, 149), (15, 16, 17), (16, 32, 48, 64), (0, 1, 2, 3), (31, 32, 33, 149)):
        pairs.append((p, subst(p, pos, rng)))
    p = seq(rng, 33)
    pairs.append((p, subst(p, (0, 32), rng)))
    pairs.append((p, subst(p, (0, 16, 32), rng)))
    # tlen != plen: one an exact prefix of the other (diagonal 0 runs into lim before the end), and with a mismatch on the way
    for L in (0, 1, 17, 32, 150):
        for d in (1, 3, 7, 8, 15):
            t = seq(rng, L + d)
            pairs.append((t[:L], t))
            pairs.append((t, t[:L]))
            if L >= 17:
                pairs.append((subst(t[:L], [L // 2], rng), t))
                pairs.append((t, subst(t[:L], [L - 1], rng)))
    # empty pattern, empty text, both
    pairs += [("", seq(rng, 5)), (seq(rng, 5), ""), ("", ""), ("", "A"), ("C", ""), ("", seq(rng, 20)), (seq(rng, 20), "")]
    # one base inserted / deleted right where the first run of diagonal 0 ends: the first I / D cells
    for L in (40, 150):
        p = seq(rng, L)
        for r in (0, 1, 15, 16, 17, 31, 32, 33, L - 2, L - 1):
            ins = p[:r] + other(p[r], rng, avoid=p[r - 1] if r else "") + p[r:]
            dele = p[:r] + p[r + 1:]
            pairs += [(p, ins), (p, dele), (ins, p), (dele, p)]
            # the same behind one mismatch (the second cell of the chain)
            if r >= 8:
                pairs += [(subst(p, [3], rng), ins), (subst(p, [3], rng), dele)]
    # diagonal 0 in the band's edge slot (tlen - plen = -7 / 7 with 8 diagonals, -15 / 15 with 16; 8: just outside the narrow band):
    # a gap of that length right behind the first run, alone and with a single-base gap the other way further on
    for L in (60, 150):
        p = seq(rng, L)
        for d in (7, 8, 15):
            for r in (0, 9, 16, 32):
                g = seq(rng, d + 1)
                g = (g[1:] if g[0] == p[r] else g[:d])
                long_ = p[:r] + g + p[r:]
                pairs += [(p, long_), (long_, p)]
                # one more base on the long side and one on the short side: the same difference with two more gaps
                short2 = p[:r + 20] + p[r + 21:]
                pairs += [(short2, long_[:r + d + 30] + "A" + long_[r + d + 30:]), (long_[:r + d + 30] + "A" + long_[r + d + 30:], short2)]
    # twice, in two orders: more than a wave's 64 lanes, refills in the middle, every pair met at an early and a late score of its wave
    order = np.random.default_rng(3).permutation(len(pairs))
    pairs = pairs + [pairs[i] for i in order]
    return datagen.from_strings([p for p, _ in pairs], [t for _, t in pairs])


def config_kw(shape):
    x, o, e = SHAPES[shape]
    return dict(span="end-to-end", scope="score", mismatch=x, gap_opening=o, gap_extension=e)


@functools.lru_cache(maxsize=None)
def edge_oracle(shape):
    oc, _ = common.configs_pair(**config_kw(shape))
    return loader.run(loader.oracle(), oc, edge_pairs(), want_cigar=False)


def run_stages(monkeypatch, stages, batch, kw, timing=False):
    monkeypatch.setenv("WFA_HIP_FAST_STAGES", stages)
    if timing:
        monkeypatch.setenv("WFA_HIP_STAGE_TIMING", "1")
    else:
        monkeypatch.delenv("WFA_HIP_STAGE_TIMING", raising=False)
    _, nc = common.configs_pair(**kw)
    score, status, _ = common.gpu_run(nc, batch, False, True)
    return score, status


def check(o, score, status, batch, ctx):
    common.assert_same(o, score, status, None, batch, ctx)
    assert np.array_equal(status, o["status"]) and np.array_equal(score, o["score"]), ctx


# (a run-time shape has no 8-diagonal form: its stage lists go without the digit 0)
CASES = [(shape, stages) for shape in SHAPES if not shape.startswith("rtc") for stages in STAGES] + [("rtc_5_8_2", "1"), ("rtc_5_8_2", "189")]


@pytest.mark.parametrize("shape,stages", CASES)
def test_constructed_edges(gpu, monkeypatch, shape, stages):
    batch = edge_pairs()
    assert 300 <= len(batch["p_len"]) <= 1000
    score, status = run_stages(monkeypatch, stages, batch, config_kw(shape))
    check(edge_oracle(shape), score, status, batch, f"{shape} stages {stages}")


def ragged(n, seed):
    """Lengths 0 .. 512, |tlen - plen| 0 .. 9, 0 - 4 % divergence (substitutions and single-base indels)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    pats, txts = [], []
    for _ in range(n):
        L = int(rng.integers(0, 513))
        tlen = int(np.clip(L + int(rng.integers(-9, 10)), 0, 512))
        p = rng.integers(0, 4, L, dtype=np.uint8)
        t = p.copy()
        err = rng.uniform(0.0, 0.04)
        sub = rng.random(L) < err
        t[sub] = (t[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) & 3
        for _ in range(int(rng.binomial(L, err / 4))):
            at = int(rng.integers(0, len(t) + 1))
            if rng.random() < 0.5 or len(t) == 0:
                t = np.insert(t, at, np.uint8(rng.integers(0, 4)))
            else:
                t = np.delete(t, min(at, len(t) - 1))
        t = t[:tlen] if len(t) >= tlen else np.concatenate([t, rng.integers(0, 4, tlen - len(t), dtype=np.uint8)])
        pats.append(acgt[p].tobytes().decode())
        txts.append(acgt[t].tobytes().decode())
    return datagen.from_strings(pats, txts)


@functools.lru_cache(maxsize=None)
def ragged_with_oracle(n, seed):
    batch = ragged(n, seed)
    oc, _ = common.configs_pair(**config_kw("s0_2_4_1"))
    return batch, loader.run(loader.oracle(), oc, batch, want_cigar=False)


@pytest.mark.parametrize("stages", ["0189", "189", "0"])
@pytest.mark.parametrize("n", [70_000, 3_000])   # (> 65 536 pairs: both lane stages take their slices at run time; 3 000: fixed slices)
def test_ragged_corpus(gpu, monkeypatch, n, stages):
    batch, o = ragged_with_oracle(n, 31)
    score, status = run_stages(monkeypatch, stages, batch, config_kw("s0_2_4_1"))
    check(o, score, status, batch, f"ragged {n} stages {stages}")


G, X, OE, E = 2, 2, 4, 1   # gap-affine 0/4/6/2 in units of g = 2


def banded_cost(p, t, lo, hi, x=4, o=6, e=2):
    """Gap-affine (Gotoh) cost of the best alignment of p and t whose cells stay on diagonals lo <= h - v < hi."""
    INF = 1 << 30
    n, m = len(p), len(t)
    M, I, D = {(0, 0): 0}, {}, {}
    for v in range(n + 1):
        for h in range(max(0, v + lo), min(m, v + hi - 1) + 1):
            if v == 0 and h == 0:
                continue
            I[v, h] = min(M.get((v, h - 1), INF) + o + e, I.get((v, h - 1), INF) + e)
            D[v, h] = min(M.get((v - 1, h), INF) + o + e, D.get((v - 1, h), INF) + e)
            mm = M.get((v - 1, h - 1), INF) + (0 if p[v - 1:v] == t[h - 1:h] else x) if v and h else INF
            M[v, h] = min(mm, I[v, h], D[v, h])
    return M.get((n, m), INF)


def band_handed(batch, o, H):
    """Pairs a lane stage with a band of 2 H diagonals must hand on: |tlen - plen| outside the band, an optimum beyond the deadline
    Bmin / g = min(2 (OE - E) + E (2c + 2H - ak), 2 (OE - E) + E (2H + 2 - 2c + ak)), or one exactly at the deadline whose every
    optimal alignment leaves the band (the formula and the tie rule of the 8-diagonal stage's test, with H free)."""
    pl = np.asarray(batch["p_len"], dtype=np.int64)
    tl = np.asarray(batch["t_len"], dtype=np.int64)
    ak = tl - pl
    c = (ak + 1) >> 1
    dl = np.minimum(2 * (OE - E) + E * (2 * c + 2 * H - ak), 2 * (OE - E) + E * (2 * H + 2 - 2 * c + ak))
    steps = -np.asarray(o["score"], dtype=np.int64) // G
    bad = (ak < 1 - 2 * H) | (ak > 2 * H - 1)
    ties = 0
    for i in np.flatnonzero(~bad & (steps == dl)):
        p, t = datagen.pair_strings(batch, int(i))
        ties += banded_cost(p, t, int(c[i]) - H, int(c[i]) + H) > G * steps[i]
    return int(np.count_nonzero(bad | (steps > dl))) + int(ties)


def test_wide_stage_hands_on_exactly_what_the_bound_rejects(gpu, monkeypatch, capfd):
    batch, o = ragged_with_oracle(20_000, 47)
    capfd.readouterr()
    score, status = run_stages(monkeypatch, "1", batch, config_kw("s0_2_4_1"), timing=True)
    err = capfd.readouterr().err
    check(o, score, status, batch, "ragged 20000 stage 1")
    m = re.findall(r"stage \d+ \(variant 1\): [0-9.]+ ms, handed on (\d+) pairs", err)
    assert len(m) == 1, err
    assert int(m[0]) == band_handed(batch, o, 8)
