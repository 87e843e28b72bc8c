"""The window pass of the plain score-only lane kernel (wfa_lane.hpp) finishes every equal-length pair with at most MH = floor(2 OE / X)
differences on diagonal 0 — score -(m X) g — and moves the pairs that are left to the front of their window, so that a finished
pair takes no lane and no place in a refill.  Constructed pairs put 0 .. MH + 2 differences at base 0, at both sides of every word
and 32-base round boundary and at the last base, for every built-in shape, the run-time shape 5/8/2 and a shape with three cells
(2/6/1 as X/OE/E, i.e. penalties 2/5/1: no window pass, unchanged); pairs a gapped alignment serves better, and pairs of unequal lengths whose diagonal 0 looks
clean, must not be finished.  Batches of finished and unfinished pairs in every arrangement (all, none, alternating windows, head,
tail, mixed) move the window bookkeeping through every edge: a window, a slice and a whole list that finish, partial last windows,
run-time and fixed slices, the second lane stage reading a device-side count.  WFA_HIP_LANE_WINFIN=0 and =1 give the same scores,
statuses and hand-over counts.  Always exact equality with the CPU oracle."""
import functools

import numpy as np
import pytest

import common
import test_lane_entry_gpu as tle
import test_lane_narrow_gpu as tln
from oracle import loader
from pywfa_amd import datagen

pytestmark = pytest.mark.gpu

# (mismatch, gap_opening, gap_extension); names are X_OE_E in units of the gcd: penalties 2/5/1 are the shape 2/6/1, three cells
SHAPES = dict(tle.SHAPES, rtc_2_6_1=(2, 5, 1))
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 512)
M_MAX = 8   # MH + 2 of the shape with the largest MH (2/6/1: 6; 2/4/1 and 1/2/1: 4)


def config_kw(shape):
    x, o, e = SHAPES[shape]
    return dict(span="end-to-end", scope="score", mismatch=x, gap_opening=o, gap_extension=e)


def mh(shape):
    x, o, e = SHAPES[shape]
    return (2 * (o + e)) // x


@functools.lru_cache(maxsize=None)
def constructed():
    rng = np.random.default_rng(5201)
    pats, txts = [], []
    for n in LENGTHS:
        p = tle.seq(rng, n)
        # base 0, both sides of every word boundary (every second one a round boundary), the last base
        cand = sorted({0, n - 1} | {b for k in range(16, n, 16) for b in (k - 1, k)})
        for m in range(0, min(M_MAX, len(cand)) + 1):
            sets = {tuple(cand[:m]), tuple(cand[len(cand) - m:])}
            if m == 1:
                sets |= {(c,) for c in cand}
            for _ in range(4):
                sets.add(tuple(sorted(cand[i] for i in rng.choice(len(cand), size=m, replace=False))))
            for at in sorted(sets):
                pats.append(p)
                txts.append(tle.subst(p, at, rng))
    # the text is the pattern rotated by one base: diagonal 0 differs everywhere, a deletion and an insertion cost 2 OE
    for n in (16, 17, 33, 150, 512):
        p = tle.seq(rng, n)
        pats.append(p)
        txts.append(p[1:] + p[:1])
    # a base inserted at a and one deleted m - 1 bases on: equal lengths, exactly m differences on diagonal 0 (no two neighbours of
    # the pattern are equal), and two gaps cost 2 OE whatever m is — the pairs just beyond MH on which a larger cap would be wrong
    for n in (33, 150):
        p = tle.seq(rng, n)
        for a in (0, 15, n - M_MAX - 1):
            for m in range(2, M_MAX + 1):
                t = p[:a] + tle.other(p[a], rng) + p[a:a + m - 1] + p[a + m:]
                assert len(t) == n and sum(x != y for x, y in zip(p, t)) == m
                pats.append(p)
                txts.append(t)
    # tlen - plen = +-1 with no, one or two differences on diagonal 0 below L: never finished in the window pass
    for n in (17, 33, 65, 150):
        p = tle.seq(rng, n)
        for at in ((), (0,), (n // 2,), (3, n - 2)):
            q = tle.subst(p, at, rng)
            longer = q + tle.other(q[-1], rng)
            pats += [p, longer, p, q[:-1]]
            txts += [longer, p, q[:-1], p]
    return datagen.from_strings(pats, txts)


@functools.lru_cache(maxsize=None)
def constructed_oracle(shape):
    oc, _ = common.configs_pair(**config_kw(shape))
    return loader.run(loader.oracle(), oc, constructed(), want_cigar=False)


# (a run-time shape has no 8-diagonal form)
CASES = [(shape, stages) for shape in tle.SHAPES if not shape.startswith("rtc") for stages in ("0", "1")] + \
        [("rtc_5_8_2", "1"), ("rtc_2_6_1", "1")]


@pytest.mark.parametrize("shape,stages", CASES)
def test_constructed_pairs(gpu, monkeypatch, shape, stages):
    batch = constructed()
    assert 300 <= len(batch["p_len"]) <= 1500
    o = constructed_oracle(shape)
    # the corpus holds what it should: pairs the rule covers (their score is the diagonal's), pairs beyond it
    pl, tl = np.asarray(batch["p_len"]), np.asarray(batch["t_len"])
    x = SHAPES[shape][0]
    steps = -np.asarray(o["score"], dtype=np.int64)
    assert np.count_nonzero((pl == tl) & (steps <= mh(shape) * x)) >= 100 and np.count_nonzero((pl == tl) & (steps > mh(shape) * x)) >= 40
    score, status = tle.run_stages(monkeypatch, stages, batch, config_kw(shape))
    tle.check(o, score, status, batch, f"{shape} stages {stages}")


# ---- bookkeeping: position i of a batch holds the i-th pair of a list of pairs the window pass finishes, or of a list it does not
N_BIG = 70_001   # the smallest size used that gets run-time slices (65 536 pairs and up)
SIZES = (1, 63, 64, 65, 128, 129, N_BIG)
ARRANGEMENTS = ("all", "none", "alternate", "head", "tail", "mixed")
N_POOL = 4099    # pairs of either kind (position i holds pair i mod N_POOL of its kind; a prime: no period of 64)


@functools.lru_cache(maxsize=None)
def pool():
    """2 x N_POOL pairs of 32 - 64 bases for the shape 2/4/1 (MH = 4), with the oracle's results: first those the window pass finishes
    (equal lengths, 0 .. 4 substitutions), then those it must leave (a base inserted or deleted, or 6 .. 8 substitutions; every
    997th with |tlen - plen| = 12: no lane stage of the first kind can take it)."""
    rng = np.random.default_rng(5309)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def subs(t, m):
        at = rng.choice(len(t), size=m, replace=False)
        t[at] = (t[at] + rng.integers(1, 4, m, dtype=np.uint8)) & 3

    pats, txts, covered = [], [], []
    for kind in (0, 1):
        for i in range(N_POOL):
            p = rng.integers(0, 4, int(rng.integers(32, 65)), dtype=np.uint8)
            t = p.copy()
            if kind == 0:
                subs(t, int(rng.integers(0, 5)))
            elif i % 997 == 500:
                t = np.concatenate([t, rng.integers(0, 4, 12, dtype=np.uint8)]) if i & 1 else t[:-12]
            else:
                how = int(rng.integers(0, 3))
                if how == 0:
                    subs(t, int(rng.integers(6, 9)))
                else:
                    subs(t, int(rng.integers(0, 3)))
                    t = np.insert(t, int(rng.integers(0, len(t) + 1)), np.uint8(rng.integers(0, 4))) if how == 1 else \
                        np.delete(t, int(rng.integers(0, len(t))))
            covered.append(len(t) == len(p) and int(np.count_nonzero(t != p)) <= 4)
            pats.append(acgt[p].tobytes().decode())
            txts.append(acgt[t].tobytes().decode())
    batch = datagen.from_strings(pats, txts)
    oc, _ = common.configs_pair(**tle.config_kw("s0_2_4_1"))
    o = loader.run(loader.oracle(), oc, batch, want_cigar=False)
    # the two halves are what they are meant to be: the rule (equal lengths, at most MH = 4 differences) covers the first and not the second
    assert all(covered[:N_POOL]) and not any(covered[N_POOL:])
    return batch, o


def arrangement(kind, n):
    """Which positions of a batch of n pairs hold a pair the window pass finishes."""
    i = np.arange(n)
    if kind == "all":
        return np.ones(n, dtype=bool)
    if kind == "none":
        return np.zeros(n, dtype=bool)
    if kind == "alternate":
        return (i // 64) % 2 == 0
    if kind == "head":
        return i < (n + 1) // 2
    if kind == "tail":
        return i >= n // 2
    return np.random.default_rng(n).random(n) < 0.5


def arranged(kind, n):
    batch, o = pool()
    idx = np.where(arrangement(kind, n), 0, N_POOL) + np.arange(n) % N_POOL
    return datagen.subset(batch, idx), {"score": np.asarray(o["score"])[idx], "status": np.asarray(o["status"])[idx]}


@pytest.mark.parametrize("stages", ["01", "0189", "189", "1"])
@pytest.mark.parametrize("kind", ARRANGEMENTS)
def test_bookkeeping_small_batches(gpu, monkeypatch, kind, stages):
    for n in SIZES[:-1]:
        batch, o = arranged(kind, n)
        score, status = tle.run_stages(monkeypatch, stages, batch, tle.config_kw("s0_2_4_1"))
        tle.check(o, score, status, batch, f"{kind}, {n} pairs, stages {stages}")


@pytest.mark.parametrize("dyn", [100, 192, 0])
@pytest.mark.parametrize("kind", ARRANGEMENTS)
def test_bookkeeping_slices(gpu, monkeypatch, kind, dyn):
    batch, o = arranged(kind, N_BIG)
    monkeypatch.setenv("WFA_HIP_LANE_DYN", str(dyn))
    for stages in ("01", "0189", "189", "1"):
        score, status = tle.run_stages(monkeypatch, stages, batch, tle.config_kw("s0_2_4_1"))
        tle.check(o, score, status, batch, f"{kind}, {N_BIG} pairs, slices of {dyn}, stages {stages}")


N_GEOMETRY = 70_001   # run-time slices need 65 536 pairs; 70 001 = 700 slices of 100 + 1 = 364 slices of 192 + 113


@functools.lru_cache(maxsize=None)
def ragged_short():
    """The ragged corpus of test_lane_window_entry_gpu, built here again: 70 001 pairs of 32 - 64 bp, 0 - 6 % substitutions, tlen - plen
    in [-3, 3]; every 997th pair with |tlen - plen| in 8 .. 20 (neither lane stage, or only the second, can take it).  With the
    oracle's results for 0/4/6/2."""
    rng = np.random.default_rng(8111)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    pats, txts = [], []
    for i in range(N_GEOMETRY):
        n = int(rng.integers(32, 65))
        d = int(rng.integers(-3, 4))
        if i % 997 == 500:
            d = int(rng.integers(8, 21)) * (1 if rng.random() < 0.5 else -1)
        m = min(max(n + d, 12), 64 + 20)
        p = rng.integers(0, 4, n, dtype=np.uint8)
        t = np.concatenate([p, rng.integers(0, 4, max(0, m - n), dtype=np.uint8)])[:m]
        sub = rng.random(m) < rng.uniform(0.0, 0.06)
        t[sub] = (t[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) & 3
        pats.append(acgt[p].tobytes().decode())
        txts.append(acgt[t].tobytes().decode())
    batch = datagen.from_strings(pats, txts)
    oc, _ = common.configs_pair(**tle.config_kw("s0_2_4_1"))
    return batch, loader.run(loader.oracle(), oc, batch, want_cigar=False)


def test_switch_off_gives_the_same(gpu, monkeypatch, capfd):
    """Scores, statuses and the hand-over counts of both widths do not depend on the switch — a pair finished in the window pass was
    never handed on before either — and the counts are what the band bounds reject."""
    batch, o = ragged_short()
    pl, tl = np.asarray(batch["p_len"]), np.asarray(batch["t_len"])
    assert np.count_nonzero((pl == tl) & (-np.asarray(o["score"]) <= 16)) >= 2000   # (pairs the window pass finishes)
    seen = []
    for winfin in ("0", "1"):
        monkeypatch.setenv("WFA_HIP_LANE_WINFIN", winfin)
        capfd.readouterr()
        score, status = tle.run_stages(monkeypatch, "01", batch, tle.config_kw("s0_2_4_1"), timing=True)
        err = capfd.readouterr().err
        tle.check(o, score, status, batch, f"ragged {N_GEOMETRY}, stages 01, WFA_HIP_LANE_WINFIN={winfin}")
        seen.append((score, status, tln.stage_handed(err, 0), tln.stage_handed(err, 1)))
    assert np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1])
    assert seen[0][2:] == seen[1][2:]
    assert seen[1][2:] == (tle.band_handed(batch, o, 4), tle.band_handed(batch, o, 8))
