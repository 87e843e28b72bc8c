"""The 8-diagonal form of the lane kernel (wfa_lane.hpp, NRP = 4) as the first stage of the score-only cascade
(WFA_HIP_FAST_STAGES digit 0): the same results whatever the stage order, the oracle's, and a hand-over count that equals
the band argument's prediction exactly."""
import re

import numpy as np
import pytest

import common
from oracle import loader
from pywfa_amd import datagen

pytestmark = pytest.mark.gpu

# gap-affine 0/4/6/2 in units of g = gcd(x, o + e, e) = 2: x = 2, o + e = 4, e = 1 (the built-in shape 0)
G, X, OE, E = 2, 2, 4, 1


def c2_prefix(n):
    return datagen.generate(n, 150, 0.02, datagen.SEEDS["C2"])


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


def run_stages(monkeypatch, stages, batch, timing=False):
    monkeypatch.setenv("WFA_HIP_FAST_STAGES", stages)
    if timing:
        monkeypatch.setenv("WFA_HIP_STAGE_TIMING", "1")
    else:
        monkeypatch.delenv("WFA_HIP_STAGE_TIMING", raising=False)
    _, nc = common.configs_pair(span="end-to-end", scope="score")
    score, status, _ = common.gpu_run(nc, batch, False, True)
    return score, status


def oracle(batch):
    oc, _ = common.configs_pair(span="end-to-end", scope="score")
    return loader.run(loader.oracle(), oc, batch, want_cigar=False)


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


def narrow_handed(batch, o):
    """Pairs the 8-diagonal stage must hand on: |tlen - plen| outside [-7, 7], an optimum beyond its deadline (the lane kernel's
    Bmin with H = 4: a score is kept at step s <= min(2 (OE - E) + E (2c + 2H - ak), 2 (OE - E) + E (2H + 2 - 2c + ak))), or one exactly
    at the deadline whose every optimal alignment leaves the band (two gaps and nothing else: the bound is reached, not passed)."""
    pl = np.asarray(batch["p_len"], dtype=np.int64)
    tl = np.asarray(batch["t_len"], dtype=np.int64)
    ak = tl - pl
    c = (ak + 1) >> 1
    H = 4
    dl = np.minimum(2 * (OE - E) + E * (2 * c + 2 * H - ak), 2 * (OE - E) + E * (2 * H + 2 - 2 * c + ak))
    steps = -np.asarray(o["score"], dtype=np.int64) // G
    bad = (ak < 1 - 2 * H) | (ak > 2 * H - 1)
    ties = 0
    for i in np.flatnonzero(~bad & (steps == dl)):
        p, t = datagen.pair_strings(batch, int(i))
        ties += banded_cost(p, t, int(c[i]) - H, int(c[i]) + H) > G * steps[i]
    return int(np.count_nonzero(bad | (steps > dl))) + int(ties)


def stage_handed(text, variant):
    m = re.findall(r"stage \d+ \(variant %d\): [0-9.]+ ms, handed on (\d+) pairs" % variant, text)
    assert len(m) == 1, text
    return int(m[0])


def test_orders_agree_on_c2_prefix(gpu, monkeypatch):
    batch = c2_prefix(1_000_000)
    s0, st0 = run_stages(monkeypatch, "0189", batch)
    s1, st1 = run_stages(monkeypatch, "189", batch)
    assert np.array_equal(st0, st1) and np.array_equal(s0, s1)
    idx = np.arange(0, 1_000_000, 97)
    o = oracle(datagen.subset(batch, idx))
    assert np.array_equal(st0[idx], o["status"]) and np.array_equal(s0[idx], o["score"])


def test_orders_agree_on_ragged_corpus(gpu, monkeypatch):
    batch = ragged(70_000, 5)   # (> 65 536 pairs: both lane stages take their slices at run time)
    o = oracle(batch)
    for stages in ("0189", "189", "01", "0"):
        s, st = run_stages(monkeypatch, stages, batch)
        assert np.array_equal(st, o["status"]), stages
        assert np.array_equal(s, o["score"]), stages


@pytest.mark.parametrize("which", ["c2", "ragged"])
def test_narrow_stage_hands_on_exactly_what_the_bound_rejects(gpu, monkeypatch, capfd, which):
    batch = c2_prefix(100_000) if which == "c2" else ragged(20_000, 9)
    o = oracle(batch)
    capfd.readouterr()
    s, st = run_stages(monkeypatch, "0", batch, timing=True)
    err = capfd.readouterr().err
    assert np.array_equal(st, o["status"]) and np.array_equal(s, o["score"])
    assert stage_handed(err, 0) == narrow_handed(batch, o)
