"""The rule behind the lane kernel's Hamming finish (wfa_lane.hpp), tested on the CPU against the oracle: an end-to-end, match = 0,
gap-affine pair of equal lengths whose diagonal 0 holds m differences scores exactly -(m x) whenever m x <= 2 (o + e) — any other
alignment leaves diagonal 0 and comes back, so it opens an insertion and a deletion.  MH = floor(2 (o + e) / x) is the cap the
kernel uses; pairs beyond it (a text that is the pattern rotated by one base) show that the cap is needed."""
import functools

import numpy as np
import pytest

import common
from oracle import loader
from pywfa_amd import datagen

# (mismatch, gap_opening, gap_extension): the seven built-in shapes (2/4/1, 2/3/1, 4/7/1, 3/5/1, 6/8/3, 5/3/3, 1/2/1 as X/OE/E in units of
# their gcd) and the run-time shapes 5/8/2 and 2/6/1 (penalties 2/5/1: the three-cell shape of the lane tests)
SHAPES = {
    "s0_2_4_1": (4, 6, 2),
    "s1_2_3_1": (2, 2, 1),
    "s2_4_7_1": (4, 6, 1),
    "s3_3_5_1": (3, 4, 1),
    "s4_6_8_3": (6, 5, 3),
    "s5_5_3_3": (5, 0, 3),
    "s6_1_2_1": (1, 1, 1),
    "rtc_5_8_2": (5, 6, 2),
    "rtc_2_6_1": (2, 5, 1),
}
LENGTHS = (1, 16, 17, 33, 150, 512)
ACGT = "ACGT"


def mh(shape):
    x, o, e = SHAPES[shape]
    return (2 * (o + e)) // x


def config_kw(shape):
    x, o, e = SHAPES[shape]
    return dict(span="end-to-end", scope="score", mismatch=x, gap_opening=o, gap_extension=e)


def rand_seq(rng, n):
    return "".join(ACGT[b] for b in rng.integers(0, 4, n))


def substituted(rng, s, m):
    """s with exactly m substitutions at random places."""
    s = list(s)
    for i in rng.choice(len(s), size=m, replace=False):
        s[i] = ACGT[(ACGT.index(s[i]) + 1 + int(rng.integers(0, 3))) & 3]
    return "".join(s)


def hamming(p, t):
    return sum(a != b for a, b in zip(p, t))


@functools.lru_cache(maxsize=None)
def substitution_pairs(shape):
    """Six pairs per length and m = 0 .. MH + 2 (m <= length)."""
    rng = np.random.default_rng(7001 + sorted(SHAPES).index(shape))
    pats, txts, ms = [], [], []
    for n in LENGTHS:
        for m in range(0, min(n, mh(shape) + 2) + 1):
            for _ in range(6):
                p = rand_seq(rng, n)
                pats.append(p)
                txts.append(substituted(rng, p, m))
                ms.append(m)
    return pats, txts, np.asarray(ms)


def oracle_scores(shape, pats, txts):
    oc, _ = common.configs_pair(**config_kw(shape))
    o = loader.run(loader.oracle(), oc, datagen.from_strings(pats, txts), want_cigar=False)
    assert not np.any(o["status"])
    return np.asarray(o["score"], dtype=np.int64)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_at_most_mh_substitutions_score_m_x(shape):
    x, o, e = SHAPES[shape]
    pats, txts, ms = substitution_pairs(shape)
    assert all(hamming(p, t) == m for p, t, m in zip(pats, txts, ms))
    score = oracle_scores(shape, pats, txts)
    within = ms <= mh(shape)
    assert within.any() and (~within).any()
    assert np.array_equal(score[within], -(ms[within] * x)), shape
    # equality m x == 2 (o + e) belongs to the rule where the shape allows it (both alignments give the same score)
    if mh(shape) * x == 2 * (o + e):
        assert np.any(ms[within] * x == 2 * (o + e))
    # beyond the cap the diagonal is only an upper bound on the cost
    assert np.all(score[~within] >= -(ms[~within] * x))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_rotated_text_needs_the_cap(shape):
    """The text is the pattern rotated by one base: diagonal 0 differs almost everywhere, one deletion and one insertion cost
    2 (o + e).  Such a pair must lie beyond MH — finishing it at m x would be wrong."""
    x, o, e = SHAPES[shape]
    rng = np.random.default_rng(7100)
    pats, txts = [], []
    for n in (16, 17, 33, 150, 512):
        p = rand_seq(rng, n)
        pats.append(p)
        txts.append(p[1:] + p[:1])
    score = oracle_scores(shape, pats, txts)
    for p, t, s in zip(pats, txts, score):
        m = hamming(p, t)
        assert s == -2 * (o + e), (shape, len(p), s)
        assert m > mh(shape) and -(m * x) < s, (shape, len(p), m)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_one_difference_beyond_the_cap_can_be_wrong(shape):
    """A base inserted at a and one deleted MH bases on: equal lengths, exactly MH + 1 differences on diagonal 0, and the two gaps
    cost 2 (o + e) < (MH + 1) x — the cap cannot be one larger."""
    x, o, e = SHAPES[shape]
    m = mh(shape) + 1
    rng = np.random.default_rng(7200)
    pats, txts = [], []
    for n in (33, 150):
        for a in (0, 5, n - m - 1):
            b = [int(rng.integers(0, 4))]
            while len(b) < n:   # no two neighbours equal: the shifted stretch differs everywhere
                b.append((b[-1] + 1 + int(rng.integers(0, 3))) & 3)
            p = "".join(ACGT[c] for c in b)
            t = p[:a] + ACGT[(b[a] + 1) & 3] + p[a:a + m - 1] + p[a + m:]
            assert len(t) == n and hamming(p, t) == m
            pats.append(p)
            txts.append(t)
    score = oracle_scores(shape, pats, txts)
    assert np.all(score == -2 * (o + e)) and 2 * (o + e) < m * x, (shape, score)


def test_share_of_c2_the_rule_finishes(capsys):
    """Counted, asserted against nothing: the share of the first 200 000 pairs of the C2 stream with tlen == plen and at most 4
    differences on diagonal 0 (what the window pass finishes), and the share the chain alone ended (fewer than 2)."""
    n = 200_000
    b = datagen.generate(n, 150, 0.02, datagen.SEEDS["C2"])
    eq = np.flatnonzero(b["t_len"] == b["p_len"])
    idx = np.arange(150, dtype=np.int64)
    p = b["seqs"][b["p_off"][eq, None] + idx]
    t = b["seqs"][b["t_off"][eq, None] + idx]
    m = (p != t).sum(axis=1)
    with capsys.disabled():
        print(f"\nC2, first {n} pairs: tlen == plen {len(eq) / n:.4%}; and m <= 4: {np.count_nonzero(m <= 4) / n:.4%}; "
              f"and m <= 1: {np.count_nonzero(m <= 1) / n:.4%}; m = 2 .. 4: {np.count_nonzero((m >= 2) & (m <= 4)) / n:.4%}")
