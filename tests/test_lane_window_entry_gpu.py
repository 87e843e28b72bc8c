"""The plain score-only lane kernel (wfa_lane.hpp) follows a pair's entry chain — the cells of diagonal 0 below score K = o + e —
once per 64-pair metadata window, lane i for pair i straight from global memory, and the refill that takes the pair picks the cells
up (cell 0 from the window's ln, cell 1 from LDS).  Constructed pairs put the first, second and third difference of diagonal 0 at
every word and round boundary of that walk and at the end of the shorter sequence, for every built-in shape, the run-time shape
5/8/2, and a run-time shape with three cells below K (2/5/1), which keeps the walk inside the refill; a corpus of 70 001 short
pairs moves the windows through run-time slices that end mid-window, slices that are no multiple of 64 and a last slice of under
64 pairs, with pairs the stage cannot take inside ordinary windows, through both ways a window finds its pairs (the batch order,
and the work list with a device-side count of the stage behind the first).  Always exact equality with the CPU oracle, and both
lane stages hand on exactly what their band bounds reject.

Not covered: a read over 512 bases inside a window (ln == 0xffffffff).  No host path produces one: every planner leaves the
register stages out of a batch whose longest read exceeds 512 bases, for list-built and indexed batches alike, so a test with such
a read would pass without running the kernel."""
import functools
import itertools

import numpy as np
import pytest

import common
import test_lane_entry_gpu as tle
import test_lane_narrow_gpu as tln
from oracle import loader
from pywfa_amd import datagen

pytestmark = pytest.mark.gpu

AT = (0, 1, 15, 16, 17, 31, 32, 47, 48)
LENGTHS = (1, 15, 16, 17, 33, 150)
DELTAS = (0, 1, -1, 7, -7, 8, -8)   # tlen - plen (8: outside the 8-diagonal band)


@functools.lru_cache(maxsize=None)
def constructed():
    """The shorter sequence a prefix of the longer one (diagonal 0 matches up to L = min(plen, tlen)), then substitutions at one, two
    and three of the positions AT, L - 2, L - 1 — and none."""
    rng = np.random.default_rng(4117)
    pats, txts = [], []
    for n, d in itertools.product(LENGTHS, DELTAS):
        plen, tlen = n, n + d
        if tlen < 0:
            continue
        L = min(plen, tlen)
        pos = sorted({a for a in AT + (L - 2, L - 1) if 0 <= a < L})
        sets = [()] + [(a,) for a in pos] + list(itertools.combinations(pos, 2))
        # three: every run of three neighbours in the list, and the two ends with each position between
        sets += [tuple(pos[i:i + 3]) for i in range(len(pos) - 2)] + [(pos[0], a, pos[-1]) for a in pos[1:-1]]
        long_ = tle.seq(rng, max(plen, tlen))
        for at in dict.fromkeys(sets):
            short = tle.subst(long_[:L], at, rng)
            p, t = (short, long_) if plen <= tlen else (long_, short)
            pats.append(p)
            txts.append(t)
    return datagen.from_strings(pats, txts)


# (mismatch, gap_opening, gap_extension) of the shapes of test_lane_entry_gpu, and one with X = 2, OE = 6: three cells below K
SHAPES = dict(tle.SHAPES, rtc_2_5_1=(2, 5, 1))


def config_kw(shape):
    x, o, e = SHAPES[shape]
    return dict(span="end-to-end", scope="score", mismatch=x, gap_opening=o, gap_extension=e)


@functools.lru_cache(maxsize=None)
def constructed_oracle(shape):
    oc, _ = common.configs_pair(**config_kw(shape))
    return loader.run(loader.oracle(), oc, constructed(), want_cigar=False)


# (a run-time shape has no 8-diagonal form: its stage orders are those without the digit 0)
CASES = [(shape, stages) for shape in tle.SHAPES if not shape.startswith("rtc") for stages in ("0", "1", "01", "0189")] + \
        [("rtc_5_8_2", "1"), ("rtc_5_8_2", "189"), ("rtc_2_5_1", "1"), ("rtc_2_5_1", "189")]


@pytest.mark.parametrize("shape,stages", CASES)
def test_constructed_differences(gpu, monkeypatch, shape, stages):
    batch = constructed()
    assert 1000 <= len(batch["p_len"]) <= 4000
    score, status = tle.run_stages(monkeypatch, stages, batch, config_kw(shape))
    tle.check(constructed_oracle(shape), score, status, batch, f"{shape} stages {stages}")


N_GEOMETRY = 70_001   # run-time slices need 65 536 pairs; 70 001 = 700 slices of 100 + 1 = 364 slices of 192 + 113


def geometry_strings():
    """32 - 64 bp, 0 - 6 % substitutions, tlen - plen in [-3, 3]; every 997th pair with |tlen - plen| in 8 .. 20 (neither lane stage,
    or only the second, can take it)."""
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
    return pats, txts


@functools.lru_cache(maxsize=None)
def geometry():
    batch = datagen.from_strings(*geometry_strings())
    oc, _ = common.configs_pair(**tle.config_kw("s0_2_4_1"))
    return batch, loader.run(loader.oracle(), oc, batch, want_cigar=False)


@pytest.mark.parametrize("dyn", [100, 192, 0])
def test_window_geometry(gpu, monkeypatch, capfd, dyn):
    batch, o = geometry()
    monkeypatch.setenv("WFA_HIP_LANE_DYN", str(dyn))
    capfd.readouterr()
    score, status = tle.run_stages(monkeypatch, "01", batch, tle.config_kw("s0_2_4_1"), timing=True)
    err = capfd.readouterr().err
    tle.check(o, score, status, batch, f"geometry, slices of {dyn}, stages 01")
    # the 8-diagonal stage reads the batch in order, the 16-diagonal stage the list the first one left, its length on the device: each
    # hands on what its band bound rejects (what 16 diagonals reject, 8 reject too, so the second count is the whole batch's at H = 8)
    assert tln.stage_handed(err, 0) == tle.band_handed(batch, o, 4)
    assert tln.stage_handed(err, 1) == tle.band_handed(batch, o, 8)

