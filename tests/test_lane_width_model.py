"""The share of C2 a first lane stage of 2 H diagonals keeps (wfa_lane.hpp, NRP = H), from the oracle's scores on the CPU: the band rule
|tlen - plen| <= 2 H - 1 and score / g <= Bmin(H), a score exactly at Bmin kept only if an optimal alignment stays inside the band.
H = 4 and H = 8 are the project's own figures (82.4 % and 98.0 %), reproduced within 0.2 points; H = 5 and H = 6 are what
the choice of the first stage's width rests on (H = 6 must keep at least 90 % for the width to be worth building)."""
import functools

import numpy as np
import pytest

import common
import lane_width_common as lw
from oracle import loader
from pywfa_amd import datagen

N = 200_000
X, O, E = 4, 6, 2   # C2's penalties 0/4/6/2


@functools.lru_cache(maxsize=None)
def c2_scores():
    batch = datagen.generate(N, 150, 0.02, datagen.SEEDS["C2"])
    oc, _ = common.configs_pair(span="end-to-end", scope="score")
    o = loader.run(loader.oracle(), oc, batch, want_cigar=False)
    assert not np.any(o["status"])
    return batch, np.asarray(o["score"], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def kept_share(H):
    batch, score = c2_scores()
    return 1.0 - np.count_nonzero(lw.handed_mask(batch, score, H, X, O, E)) / N


def test_vectorised_banded_cost_equals_the_scalar_one():
    """The numpy banded Gotoh against the scalar one of test_lane_narrow_gpu, on pairs at the H = 5 deadline and a few others."""
    import test_lane_narrow_gpu as narrow
    batch, score = c2_scores()
    g, _, OE, Eg = lw.shape_of(X, O, E)
    ak, c, bad = lw.band(batch, 5)
    ties = np.flatnonzero(~bad & (-score // g == lw.deadline(ak, c, 5, OE, Eg)))[:12]
    idx = np.concatenate([ties, np.arange(8)])
    for H in (4, 5):
        got = lw.banded_costs(batch, idx, c[idx] - H, c[idx] + H, X, O, E)
        for i, cost in zip(idx, got):
            p, t = lw.pair(batch, i)
            want = narrow.banded_cost(p, t, int(c[i]) - H, int(c[i]) + H)
            assert min(int(cost), lw.INF) == min(want, lw.INF) or (cost >= lw.INF and want >= lw.INF), (H, int(i), int(cost), want)


def test_documented_shares_are_reproduced(capsys):
    shares = {H: kept_share(H) for H in (4, 5, 6, 8)}
    batch, score = c2_scores()
    with capsys.disabled():
        print("\nC2, first %d pairs, mean score %.2f g-units; kept by the band rule: " % (N, float(np.mean(-score)) / 2)
              + ", ".join("H = %d: %.2f %%" % (H, 100 * s) for H, s in shares.items()))
    assert abs(100 * shares[4] - 82.4) <= 0.2, shares
    assert abs(100 * shares[8] - 98.0) <= 0.2, shares
    assert shares[4] < shares[5] < shares[6] < shares[8]


def test_twelve_diagonals_keep_nine_in_ten():
    """The estimate behind the wider first stage: H = 6 keeps at least 90 % of C2."""
    assert kept_share(6) >= 0.90, kept_share(6)


@pytest.mark.parametrize("H", [4, 5, 6])
def test_closed_form_count_never_hands_on_more_than_the_exact_rule(H, capsys):
    """What the pilot counts (a score at Bmin kept) differs from the exact rule only by the pairs at Bmin that leave the band: it
    hands on a subset.  (The difference is printed: it is the error of the pilot's estimate of the hand-over share.)"""
    batch, score = c2_scores()
    loose = lw.handed_mask(batch, score, H, X, O, E, exact_ties=False)
    exact = lw.handed_mask(batch, score, H, X, O, E)
    assert not np.any(loose & ~exact)
    with capsys.disabled():
        print("\nH = %d: handed on %d (exact), %d (a score at Bmin kept)" % (H, np.count_nonzero(exact), np.count_nonzero(loose)))
