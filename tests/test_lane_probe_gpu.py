"""The extension probes of the plain score-only lane kernel (wfa_lane.hpp, both widths): constructed pairs at the word and round
boundaries of the probes and at the limits of a slot.  A probe compares 16 bases (two packed words per sequence), a run that goes on
is parked and continued 32 bases per round, a second run of the same lane in the same step is finished on the spot; what can go
wrong there goes wrong at 16-base word boundaries of the pattern and of the text (independently: a run on an off-diagonal starts
and ends at different places in the two), at the end of a slot (offset == lim) and where two runs meet — not at 150 bp x 10 M.
So: every length 1 .. 70, and for each equal pairs, a substitution at every position of the first three words and at the end, gaps of
one to three bases at the word boundaries, pairs with two long runs in one step, and every tlen - plen in -15 .. 15 (beyond +-7
the 8-diagonal form must hand the pair on; a pair with two gaps passes the deadline of either form).  Scores and statuses are
compared with the CPU oracle, exactly, for the seven built-in penalty shapes and a run-time shape, for four stage orders, with more
than 64 pairs per wave and as 65 pairs (a second wave with one lane); the number of pairs a single lane stage hands on is compared
with the band argument's prediction."""
import functools

import numpy as np
import pytest

import common
import test_lane_entry_gpu as entry
import test_lane_narrow_gpu as narrow
from oracle import loader
from pywfa_amd import datagen

pytestmark = pytest.mark.gpu

SHAPES = entry.SHAPES
ORDERS = ("0", "1", "01", "0189")
RTC_ORDERS = ("1", "189")      # (a run-time shape has no 8-diagonal form: the same orders without the digit 0)
GAP_AT = (0, 15, 16, 17, 31, 32, 33)
ACGT = "ACGT"


def rot(unit, n, shift=0):
    return "".join(unit[(i + shift) % len(unit)] for i in range(n))


@functools.lru_cache(maxsize=None)
def corpus_strings():
    rng = np.random.default_rng(7150)
    pairs = []
    for L in range(1, 71):
        p = entry.seq(rng, L)
        pairs.append((p, p))
        # one substitution: every position of words 0 - 2, and the last base
        for at in sorted(set(range(min(L, 48))) | {L - 1}):
            pairs.append((p, entry.subst(p, [at], rng)))
        # a gap of 1 - 3 bases at the word boundaries: the run behind it lies on diagonal +-1 .. +-3 and starts at a different place
        # of a word in the pattern and in the text
        for at in sorted({a for a in GAP_AT if a < L} | {L - 1}):
            for g in (1, 2, 3):
                ins = entry.seq(rng, g + 1)
                ins = ins[1:] if ins[0] == p[at] else ins[:g]
                longer = p[:at] + ins + p[at:]
                pairs += [(p, longer), (longer, p)]
                if at + g <= L:
                    shorter = p[:at] + p[at + g:]
                    pairs += [(p, shorter), (shorter, p)]
        # two runs that go on in the same step of one pair.  Period 2 shifted by one base (period 4: by two): diagonal 0 matches nowhere
        # and diagonals +1 and -1 (+2 and -2) both match to the end, from the same score; the same behind a common prefix and in front
        # of a common suffix.  Then the issue's example: a tandem repeat of period 1 - 3 with one unit more on one side
        if L >= 18:
            for unit, sh in (("AC", 1), ("GT", 1), ("ACGT", 2), ("AGCT", 2)):
                a, b = rot(unit, L), rot(unit, L, sh)
                pairs += [(a, b), (b, a)]
                f = entry.seq(rng, 3)
                pairs += [(f + a[:L - 3], f + b[:L - 3]), (a[:L - 3] + f, b[:L - 3] + f), (a, b[:L - 1]), (a[:L - 1], b)]
            for unit in ("A", "AC", "ACG"):
                span = min(L - 2, 44) // len(unit) * len(unit)
                fl = entry.seq(rng, L - span)
                fa, fb = fl[:(L - span) // 2], fl[(L - span) // 2:]
                a = fa + rot(unit, span) + fb
                b = fa + rot(unit, span + len(unit)) + fb
                c = fa + rot(unit, span)[:span // 2] + "T" + rot(unit, span)[span // 2 + 1:] + fb
                pairs += [(a, b), (b, a), (c, b), (b, c)]
        # every tlen - plen in -15 .. 15: one gap at the front, at the first word boundary or in the middle, and the same difference as two gaps with a substitution between them
        for d in range(-15, 16):
            if L + d < 0:
                continue
            for at in sorted({0, min(16, L), L // 2}):
                if d >= 0:
                    t = p[:at] + entry.seq(rng, d) + p[at:]
                else:
                    lo = min(at, L + d)          # (the gap of -d bases ends inside the pattern)
                    t = p[:lo] + p[lo - d:]
                assert len(t) == L + d
                pairs.append((p, t))
                if L >= 12 and len(t) >= 10:
                    t2 = t[:2] + t[3:len(t) - 3] + entry.other(t[-3], rng) + t[-3:]   # one base out near the front, one in near the end
                    t2 = entry.subst(t2, [len(t2) // 2], rng)
                    pairs.append((p, t2))
    return pairs


@functools.lru_cache(maxsize=None)
def corpus():
    """The list in a fixed shuffled order: every wave holds 64 pairs of different lengths, so parked runs of different lengths share
    their rounds, and every refill mixes the cases."""
    pairs = corpus_strings()
    order = np.random.default_rng(11).permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    return datagen.from_strings([p for p, _ in pairs], [t for _, t in pairs])


@functools.lru_cache(maxsize=None)
def corpus65():
    """65 pairs: a wave of 64 and a second wave with one lane.  Every 1/65th of the shuffled list, so all the cases are met."""
    n = len(corpus()["p_len"])
    return datagen.subset(corpus(), np.arange(65) * (n // 65))


@functools.lru_cache(maxsize=None)
def oracle_for(shape, small):
    oc, _ = common.configs_pair(**entry.config_kw(shape))
    batch = corpus65() if small else corpus()
    o = loader.run(loader.oracle(), oc, batch, want_cigar=False)
    # the coverage rule: a pair the oracle cannot score is an error, never a case left out
    assert len(o["score"]) == len(batch["p_len"]) and np.all(np.asarray(o["status"]) == 0), f"{shape}: the oracle did not score every pair"
    return o


def test_corpus_is_what_the_header_says():
    pairs = corpus_strings()
    assert 20_000 <= len(pairs) <= 60_000, len(pairs)
    pl = np.array([len(p) for p, _ in pairs]); tl = np.array([len(t) for _, t in pairs])
    assert set(range(1, 71)) <= set(pl.tolist())
    for d in range(-15, 16):
        assert np.count_nonzero(tl - pl == d) >= 50, d
    assert corpus_strings() is corpus_strings() and len(corpus65()["p_len"]) == 65


CASES = [(s, o) for s in SHAPES if not s.startswith("rtc") for o in ORDERS] + [("rtc_5_8_2", o) for o in RTC_ORDERS]


@pytest.mark.parametrize("shape,stages", CASES)
def test_probe_corpus(gpu, monkeypatch, shape, stages):
    for small in (False, True):
        batch = corpus65() if small else corpus()
        o = oracle_for(shape, small)
        score, status = entry.run_stages(monkeypatch, stages, batch, entry.config_kw(shape))
        assert len(score) == len(batch["p_len"])
        entry.check(o, score, status, batch, f"{shape} stages {stages} ({len(score)} pairs)")


@pytest.mark.parametrize("stages", ["0", "1"])
def test_single_stage_hands_on_what_the_band_rejects(gpu, monkeypatch, capfd, stages):
    """The hand-over set of either width is unchanged: gap-affine 0/4/6/2 (the shape the helpers of the two stages' own tests are
    written for), the count of pairs left to the later stages against the band prediction."""
    batch, o = corpus(), oracle_for("s0_2_4_1", False)
    capfd.readouterr()
    score, status = entry.run_stages(monkeypatch, stages, batch, entry.config_kw("s0_2_4_1"), timing=True)
    err = capfd.readouterr().err
    entry.check(o, score, status, batch, f"stage {stages} alone")
    want = narrow.narrow_handed(batch, o) if stages == "0" else entry.band_handed(batch, o, 8)
    got = narrow.stage_handed(err, int(stages))
    print(f"stage {stages}: handed on {got}, band prediction {want}")
    assert got == want
