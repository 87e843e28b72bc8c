"""The 10- and 12-diagonal forms of the lane kernel's first stage (wfa_lane.hpp, NRP = 5 and 6; WFA_HIP_LANE_NARROW_NRP with stage
digit 0): the checks of tests/test_lane_narrow_gpu.py for both widths.  The hand-over count equals the band argument's prediction
exactly; constructed pairs sit on every edge of the band (|tlen - plen| at and beyond 2 H - 1, odd and even, scores at Bmin - 1, Bmin
and Bmin + 1, the end diagonal and diagonal 0 in the outermost slots and the last register, reads of 1 .. 512 bases) for all seven
built-in shapes; the whole cascade gives the oracle's results whatever the width; run-time and fixed slices; and the pilot's choice
of the width on a batch where it is clear."""
import functools
import re

import numpy as np
import pytest

import common
import lane_width_common as lw
import test_lane_entry_gpu as tle
import test_lane_narrow_gpu as tln
import test_lane_window_entry_gpu as tlw
from oracle import loader
from pywfa_amd import datagen

pytestmark = pytest.mark.gpu

WIDTHS = (5, 6)
BUILTIN = [s for s in tle.SHAPES if not s.startswith("rtc")]


def run_width(monkeypatch, nrp, stages, batch, kw, timing=False):
    if nrp is None:
        monkeypatch.delenv("WFA_HIP_LANE_NARROW_NRP", raising=False)
    else:
        monkeypatch.setenv("WFA_HIP_LANE_NARROW_NRP", str(nrp))
    return tle.run_stages(monkeypatch, stages, batch, kw, timing=timing)


def oracle(batch, shape="s0_2_4_1"):
    oc, _ = common.configs_pair(**tle.config_kw(shape))
    return loader.run(loader.oracle(), oc, batch, want_cigar=False)


# ---- the hand-over count on a ragged corpus

@functools.lru_cache(maxsize=None)
def ragged_short():
    """About 20 000 pairs of 30 - 150 bp at 1 - 4 % (substitutions and single-base indels), |tlen - plen| up to 13."""
    rng = np.random.default_rng(615)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    pats, txts = [], []
    for _ in range(20_000):
        L = int(rng.integers(30, 151))
        p = rng.integers(0, 4, L, dtype=np.uint8)
        t = p.copy()
        err = rng.uniform(0.01, 0.04)
        sub = rng.random(L) < err
        t[sub] = (t[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) & 3
        for _ in range(int(rng.binomial(L, err / 3))):
            at = int(rng.integers(0, len(t) + 1))
            if rng.random() < 0.5:
                t = np.insert(t, at, np.uint8(rng.integers(0, 4)))
            else:
                t = np.delete(t, min(at, len(t) - 1))
        if rng.random() < 0.1:   # a longer end gap: the end diagonal near and beyond the band's edge
            d = int(rng.integers(5, 14))
            t = np.concatenate([t, rng.integers(0, 4, d, dtype=np.uint8)]) if rng.random() < 0.5 else t[:max(1, len(t) - d)]
        pats.append(acgt[p].tobytes().decode())
        txts.append(acgt[t].tobytes().decode())
    batch = datagen.from_strings(pats, txts)
    return batch, oracle(batch)


@pytest.mark.parametrize("nrp", WIDTHS)
def test_hand_over_count_is_exact(gpu, monkeypatch, capfd, nrp):
    batch, o = ragged_short()
    want = lw.handed_mask(batch, o["score"], nrp, *tle.SHAPES["s0_2_4_1"])
    ak, c, bad = lw.band(batch, nrp)
    steps = -np.asarray(o["score"], dtype=np.int64) // 2
    dl = lw.deadline(ak, c, nrp, 4, 1)
    # the corpus holds every reason to hand a pair on, and pairs at the bound that stay
    assert bad.any() and (~bad & (steps > dl)).any() and (~bad & (steps == dl) & want).any() and (~bad & (steps == dl) & ~want).any()
    capfd.readouterr()
    score, status = run_width(monkeypatch, nrp, "01", batch, tle.config_kw("s0_2_4_1"), timing=True)
    err = capfd.readouterr().err
    tle.check(o, score, status, batch, f"ragged, width {nrp}")
    assert tln.stage_handed(err, 0) == int(np.count_nonzero(want))
    assert tln.stage_handed(err, 1) == tle.band_handed(batch, o, 8)


# ---- constructed pairs at the band's edges, every built-in shape

@functools.lru_cache(maxsize=None)
def edge_grid():
    """150 bp; tlen - plen = -13 .. 13 as one gap behind base 60 (so: +-(2 H - 1) and +-2 H of both widths, odd and even, the end
    diagonal in the outermost slot on either side, diagonal 0 in the last register), 0 .. 10 spaced substitutions, and none or
    one further insertion and deletion of one or two bases behind base 100: scores on both sides of every width's bound."""
    rng = np.random.default_rng(5606)
    pats, txts = [], []
    for ak in range(-13, 14):
        for nsub in range(0, 11):
            for a, b in ((0, 0), (1, 1), (2, 1), (1, 2)):
                p = tle.seq(rng, 150)
                t = tle.subst(p, [5 + 9 * i if i < 6 else 110 + 7 * (i - 6) for i in range(nsub)], rng)
                d = ak - (a - b)
                t = t[:100] + tle.seq(rng, a) + t[100:130] + t[130 + b:]
                t = t[:60] + tle.seq(rng, d) + t[60:] if d >= 0 else t[:60] + t[60 - d:]
                assert len(t) - len(p) == ak
                pats.append(p)
                txts.append(t)
    return datagen.from_strings(pats, txts)


@functools.lru_cache(maxsize=None)
def grid_oracle(shape):
    return oracle(edge_grid(), shape)


@pytest.mark.parametrize("nrp", WIDTHS)
@pytest.mark.parametrize("shape", BUILTIN)
def test_constructed_band_edges(gpu, monkeypatch, capfd, shape, nrp):
    batch, o = edge_grid(), grid_oracle(shape)
    x, op, e = tle.SHAPES[shape]
    g, X, OE, E = lw.shape_of(x, op, e)
    H = nrp
    ak, c, bad = lw.band(batch, H)
    steps = -np.asarray(o["score"], dtype=np.int64) // g
    dl = lw.deadline(ak, c, H, OE, E)
    want = lw.handed_mask(batch, o["score"], H, x, op, e)
    # what the grid must hold for this shape and width (from the oracle's scores, before anything runs on the GPU)
    # scores next to the bound on either side.  With X and OE - E both even every score has the parity of E (tlen - plen) — substitutions
    # and gap openings add even amounts, the gap lengths add up to tlen - plen mod 2 — and so has Bmin = 2 (OE - E) + E (2 H [+ 1 for an
    # odd difference]): Bmin +- 1 cannot occur for 2/3/1 and 4/7/1, and the nearest scores are Bmin +- 2
    near = 2 if (X % 2 == 0 and (OE - E) % 2 == 0) else 1
    for d in (-near, 0, near):
        assert (~bad & (steps - dl == d)).any(), (shape, H, d)
    for edge in (2 * H - 1, 1 - 2 * H):          # the end diagonal in the outermost slot, kept and handed on
        assert ((ak == edge) & ~want).any() and ((ak == edge) & want).any(), (shape, H, edge)
    for out in (2 * H, -2 * H):
        assert ((ak == out) & bad).any()
    for last in (2 - 2 * H, 3 - 2 * H):           # diagonal 0 in the last register (slot 2 H - 1, slot 2 H - 2), kept
        assert ((ak == last) & ~want).any(), (shape, H, last)
    capfd.readouterr()
    score, status = run_width(monkeypatch, nrp, "01", batch, tle.config_kw(shape), timing=True)
    err = capfd.readouterr().err
    tle.check(o, score, status, batch, f"{shape} width {nrp}: grid")
    assert tln.stage_handed(err, 0) == int(np.count_nonzero(want)), (shape, nrp)
    # reads of 0, 1, 15, 16, 17 .. 512 bases and the entry's own edges (the corpus of test_lane_entry_gpu)
    score, status = run_width(monkeypatch, nrp, "01", tle.edge_pairs(), tle.config_kw(shape))
    tle.check(tle.edge_oracle(shape), score, status, tle.edge_pairs(), f"{shape} width {nrp}: entry edges")


# ---- the whole cascade, every width

@functools.lru_cache(maxsize=None)
def c2_prefix():
    batch = tln.c2_prefix(100_000)   # (> 65 536 pairs: run-time slices)
    return batch, oracle(batch)


def test_cascade_agrees_across_widths(gpu, monkeypatch):
    batch, o = c2_prefix()
    for nrp, stages in ((4, "0189"), (5, "0189"), (6, "0189"), (None, "189")):
        score, status = run_width(monkeypatch, nrp, stages, batch, tle.config_kw("s0_2_4_1"))
        assert np.array_equal(status, o["status"]) and np.array_equal(score, o["score"]), (nrp, stages)


# ---- slices taken at run time and fixed slices

@functools.lru_cache(maxsize=None)
def geometry_handed(H):
    batch, o = tlw.geometry()
    return int(np.count_nonzero(lw.handed_mask(batch, o["score"], H, *tle.SHAPES["s0_2_4_1"])))


@pytest.mark.parametrize("dyn", [100, 192, 0])
@pytest.mark.parametrize("nrp", WIDTHS)
def test_run_time_slices(gpu, monkeypatch, capfd, nrp, dyn):
    batch, o = tlw.geometry()
    monkeypatch.setenv("WFA_HIP_LANE_DYN", str(dyn))
    capfd.readouterr()
    score, status = run_width(monkeypatch, nrp, "01", batch, tle.config_kw("s0_2_4_1"), timing=True)
    err = capfd.readouterr().err
    tle.check(o, score, status, batch, f"geometry, width {nrp}, slices of {dyn}")
    assert tln.stage_handed(err, 0) == geometry_handed(nrp)
    assert tln.stage_handed(err, 1) == geometry_handed(8)


# ---- the pilot's choice

def pilot_line(err):
    m = re.findall(r"pilot: 8 / 10 / 12 diagonals \(lane form\) hand on (\d+) / (\d+) / (\d+) of (\d+); first lane stage: (\d+) diagonals", err)
    return [tuple(int(v) for v in t) for t in m]


def test_pilot_takes_eight_diagonals_at_half_a_percent(gpu, monkeypatch, capfd):
    """0.5 %: every width hands on next to nothing (CPU: 0.17 / 0.05 / 0.01 % of 70 000 pairs), so the cheapest stage per pair wins —
    the narrowest — whatever the model's constants."""
    batch = datagen.generate(70_000, 150, 0.005, datagen.SEEDS["C2"])
    o = oracle(batch)
    loose = [np.count_nonzero(lw.handed_mask(batch, o["score"], H, 4, 6, 2, exact_ties=False)) / 70_000 for H in (4, 5, 6)]
    assert loose[0] < 0.005
    monkeypatch.delenv("WFA_HIP_FAST_STAGES", raising=False)
    monkeypatch.delenv("WFA_HIP_LANE_NARROW_NRP", raising=False)
    monkeypatch.setenv("WFA_HIP_STAGE_TIMING", "1")
    _, nc = common.configs_pair(**tle.config_kw("s0_2_4_1"))
    capfd.readouterr()
    score, status, _ = common.gpu_run(nc, batch, False, True)
    err = capfd.readouterr().err
    assert np.array_equal(status, o["status"]) and np.array_equal(score, o["score"])
    lines = pilot_line(err)
    assert len(lines) >= 1, err
    h4, h5, h6, np_, diag = lines[0]
    assert diag == 8, lines
    # the sample's counts against the batch's shares: 8 192 draws, four standard deviations of a share below 0.5 % (0.3 points)
    for h, s in zip((h4, h5, h6), loose):
        assert abs(h / np_ - s) <= 0.003, (lines, loose)
    assert h4 >= h5 >= h6
    assert re.search(r"stage 0 \(variant 0\)", err), err


def test_pilot_takes_no_narrow_stage_at_three_percent(gpu, monkeypatch, capfd):
    """3 %: 12 diagonals hand on 24 % of the pairs (CPU), beyond the 20 % a narrow stage may hand on, and 16 diagonals 11 %, beyond
    the 8 % at which they go first: no lane stage of any narrow width."""
    batch = datagen.generate(70_000, 150, 0.03, datagen.SEEDS["C2"])
    o = oracle(batch)
    loose6 = np.count_nonzero(lw.handed_mask(batch, o["score"], 6, 4, 6, 2, exact_ties=False)) / 70_000
    assert loose6 > 0.22   # (four standard deviations of the sample's share, 1.9 points, above 20 %)
    monkeypatch.delenv("WFA_HIP_FAST_STAGES", raising=False)
    monkeypatch.delenv("WFA_HIP_LANE_NARROW_NRP", raising=False)
    monkeypatch.setenv("WFA_HIP_STAGE_TIMING", "1")
    _, nc = common.configs_pair(**tle.config_kw("s0_2_4_1"))
    capfd.readouterr()
    score, status, _ = common.gpu_run(nc, batch, False, True)
    err = capfd.readouterr().err
    assert np.array_equal(status, o["status"]) and np.array_equal(score, o["score"])
    assert all(t[4] == 16 for t in pilot_line(err)), err
    assert re.search(r"stage 0 \(variant", err) and not re.search(r"stage \d+ \(variant 0\)", err), err
