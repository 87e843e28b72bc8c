"""The plain recurrence of tests/dp_reference.py: hand-worked answers, the oracle against it, and proof that its op-string checker
notices what it is there to notice.  CPU only."""
import re

import numpy as np
import pytest

import common
import corpus_common
import dp_reference as dp
from oracle import loader
from pywfa_amd import datagen
from test_parity_gpu import GRID

METRICS = ["indel", "levenshtein", "linear", "affine", "affine2p"]


def cost1(p, t, **kw):
    return int(dp.dp_cost(datagen.from_strings([p], [t]), loader.make_config(**kw))[0])


def price(ops, p, t, **kw):
    return dp.price_ops(ops, p, t, loader.make_config(**kw))


# ------------------------------------------------------------------------------------------ answers worked out by hand
def test_empty_against_empty():
    for d in METRICS:
        for span in ("end-to-end", "ends-free"):
            assert cost1("", "", distance=d, span=span) == 0
            assert price(b"", "", "", distance=d, span=span) == (True, 0)


@pytest.mark.parametrize("distance,n,want", [("indel", 5, 5), ("levenshtein", 5, 5), ("linear", 5, 10), ("affine", 5, 16), ("affine2p", 5, 16),
                                             ("affine2p", 30, 54)])   # (pywfa's defaults 4 / 6 / 2 / 24 / 1; 30: 24 + 30 < 6 + 60)
def test_empty_against_n_bases(distance, n, want):
    s = "ACGTT" * (n // 5)
    assert cost1("", s, distance=distance, span="end-to-end") == want
    assert cost1(s, "", distance=distance, span="end-to-end") == want
    assert price("I" * n, "", s, distance=distance, span="end-to-end") == (True, want)
    assert price("D" * n, s, "", distance=distance, span="end-to-end") == (True, want)
    assert price("D" * n, "", s, distance=distance, span="end-to-end")[0] is False
    # the same bases inside the free ends cost nothing: begin and end allowances of one run add
    assert cost1("", s, distance=distance, text_begin_free=2, text_end_free=n - 2) == 0
    assert price("I" * n, "", s, distance=distance, text_begin_free=2, text_end_free=n - 2) == (True, 0)
    one_less = {"indel": 1, "levenshtein": 1, "linear": 2, "affine": 8, "affine2p": 8}[distance]
    assert cost1("", s, distance=distance, text_begin_free=2, text_end_free=n - 3) == one_less
    assert price("I" * n, "", s, distance=distance, text_begin_free=2, text_end_free=n - 3) == (True, one_less)


@pytest.mark.parametrize("distance,want", [("indel", 8), ("levenshtein", 4), ("linear", 16), ("affine", 16), ("affine2p", 16)])
def test_no_common_base(distance, want):
    """AAAA / CCCC: four mismatches (4 x 4) against two gaps of four (indel: the only way; gap-affine 2 x 14)."""
    assert cost1("AAAA", "CCCC", distance=distance, span="end-to-end") == want
    ops = "DDDDIIII" if distance == "indel" else "XXXX"
    assert price(ops, "AAAA", "CCCC", distance=distance, span="end-to-end") == (True, want)
    assert price("MMMM", "AAAA", "CCCC", distance=distance, span="end-to-end")[0] is False
    assert price("XXXX", "AAAA", "CCCC", distance="indel", span="end-to-end")[0] is False
    assert cost1("AAAA", "CCCC", distance="affine", mismatch=8, span="end-to-end") == 28


def test_one_long_two_piece_gap_beats_two_short_ones():
    """L C^12 T C^12 R against L T R: keeping the T matched takes two gaps of 12, 2 x min(6 + 24, 24 + 12) = 60; one gap of 24
    and the left-over C against the T as a mismatch costs min(6 + 48, 24 + 24) + 4 = 52 — the second piece is what makes it win
    by that much (one piece: 58 against 60)."""
    L, R = "AGGAAGAGGA", "GAAGGAGAAG"
    p, t = L + "C" * 12 + "T" + "C" * 12 + R, L + "T" + R
    kw = dict(distance="affine2p", span="end-to-end")
    assert cost1(p, t, **kw) == 52
    assert price("M" * 10 + "D" * 24 + "X" + "M" * 10, p, t, **kw) == (True, 52)
    assert price("M" * 10 + "D" * 12 + "M" + "D" * 12 + "M" * 10, p, t, **kw) == (True, 60)
    assert cost1(p, t, distance="affine", span="end-to-end") == 58


def test_free_begin_worth_taking_on_one_side_only():
    s = "ACGTACGGTCAG"
    p, t = "TTT" + s, s
    assert cost1(p, t, pattern_begin_free=3, text_begin_free=3) == 0
    assert price("DDD" + "M" * 12, p, t, pattern_begin_free=3, text_begin_free=3) == (True, 0)
    assert cost1(p, t, pattern_begin_free=0, text_begin_free=3) == 12          # the text's free begin is of no use: one gap of 3
    assert price("DDD" + "M" * 12, p, t, pattern_begin_free=0, text_begin_free=3) == (True, 12)
    assert cost1(p, t, pattern_begin_free=2, text_begin_free=3) == 8           # two free, the third a gap of 1
    assert price("DDD" + "M" * 12, p, t, pattern_begin_free=2, text_begin_free=3) == (True, 8)
    assert cost1(p, t, span="end-to-end", pattern_begin_free=3) == 12          # free ends are read under ends-free only
    assert cost1(t, p, pattern_end_free=9, text_begin_free=3) == 0


def test_wildcard_saves_a_mismatch():
    p, t = "ACGTNACGT", "ACGTCACGT"
    assert cost1(p, t, wildcard="N") == 0 and cost1(p, t) == 4
    assert price("M" * 9, p, t, wildcard="N") == (True, 0)
    assert price("M" * 9, p, t)[0] is False
    assert price("MMMMXMMMM", p, t) == (True, 4)
    assert price("MMMMXMMMM", p, t, wildcard="N")[0] is False     # X where the model counts a match
    assert cost1(t, p, wildcard="N") == 0                         # the wildcard on either side


def test_match_bonus_is_the_classical_score():
    """match = -1, 4 / 6 / 2: eleven matches, one mismatch, one gap of two: 11 - 4 - 10 = -3; the reported score is -penalty."""
    p, t = "ACGTAGGTCAGG", "ACGTACGTCAGGTT"
    kw = dict(match=-1, span="end-to-end")
    assert price("MMMMMXMMMMMMII", p, t, **kw) == (True, -11 + 4 + 10)
    assert cost1(p, t, **kw) == 3
    assert dp.penalty_of_score(-3, loader.make_config(**kw)) == 3 and dp.penalty_of_score(7, loader.make_config(distance="indel")) == 7
    with pytest.raises(ValueError):
        cost1(p, t, match=-1, text_end_free=2)


# ------------------------------------------------------------------------------------------ the oracle against the recurrence
def exact_grid():
    """Every exact configuration family of the parity grid that the recurrence covers — no heuristic, no step limit, and not
    match < 0 with free ends — with BiWFA in both scopes."""
    out = []
    for kw in GRID:
        if kw.get("heuristic") or kw.get("max_steps"):
            continue
        free = any(kw.get(k, 0) for k in ("pattern_begin_free", "pattern_end_free", "text_begin_free", "text_end_free"))
        if kw.get("match", 0) < 0 and kw.get("span", "ends-free") == "ends-free" and free:
            continue
        out.append(kw)
        if kw.get("memory_mode") == "biwfa":
            out.append(dict(kw, scope="full"))
    return out


EXACT = exact_grid()
_corpora = {}


def corpus(name):
    if name not in _corpora:
        import validate_oracle as vo
        _corpora[name] = {"60bp_15pct": lambda: datagen.generate(200, 60, 0.15, 7060), "150bp_20pct": lambda: datagen.generate(80, 150, 0.2, 7150),
                          "special_mini": lambda: corpus_common.special_mini(vo.corpus_special(seed=99))}[name]()
    return _corpora[name]


def fit_free(batch, kw, keep=0):
    """The pairs of `batch` whose sequences hold the free ends of `kw` (the library refuses the others), repeated from the front up
    to `keep` pairs so that a batch stays on the path its size selects."""
    p_need = max(kw.get("pattern_begin_free", 0), kw.get("pattern_end_free", 0))
    t_need = max(kw.get("text_begin_free", 0), kw.get("text_end_free", 0))
    if kw.get("span", "ends-free") != "ends-free" or (p_need == 0 and t_need == 0):
        return batch
    idx = np.flatnonzero((batch["p_len"] >= p_need) & (batch["t_len"] >= t_need))
    if len(idx) < keep:
        idx = np.concatenate([idx, idx[:keep - len(idx)]])
    return datagen.subset(batch, idx)


def assert_optimal(cfg, batch, cost, score, status, cigars, ctx, unset_ok=False):
    """Every pair completed, its score stands for the recurrence's cost, its op string (if any) is an alignment of that price."""
    assert (np.asarray(status) == 0).all(), (ctx, "status", np.flatnonzero(np.asarray(status) != 0)[:5])
    for i in range(len(cost)):
        p, t = datagen.pair_strings(batch, i)
        faults = dp.faults(cfg, p, t, int(cost[i]), int(score[i]), None if cigars is None else cigars[i], unset_ok)
        assert not faults, f"{ctx}: pair {i}: {faults}\nP={p[:200]}\nT={t[:200]}"


@pytest.mark.parametrize("name", ["60bp_15pct", "150bp_20pct", "special_mini"])
@pytest.mark.parametrize("cfg_idx", range(len(EXACT)))
def test_oracle_is_optimal(cfg_idx, name):
    kw = EXACT[cfg_idx]
    batch = fit_free(corpus(name), kw)
    assert len(batch["p_len"]) >= 30
    cfg = loader.make_config(**kw)
    o = loader.run(loader.oracle(), cfg, batch)
    cost = dp.dp_cost(batch, cfg)
    # (BiWFA with CIGARs leaves the score unset where the top level never splits, SURVEY.md Appendix B Q6: the op string is priced)
    assert_optimal(cfg, batch, cost, o["score"], o["status"], o["cigars"], f"{name} {kw}",
                   unset_ok=(kw.get("memory_mode") == "biwfa" and cfg.scope == 1))


def test_exact_grid_holds_every_family():
    d = [loader.make_config(**kw) for kw in EXACT]
    assert {c.distance for c in d} == {0, 1, 2, 3, 4}
    frees = {(c.pattern_begin_free, c.pattern_end_free, c.text_begin_free, c.text_end_free) for c in d if c.span == 1}
    assert {(0, 0, 0, 0), (8, 7, 3, 2), (20, 0, 0, 9)} <= frees
    assert {c.memory_mode for c in d} == {0, 1, 2, 3} and {c.scope for c in d if c.memory_mode == 3} == {0, 1}
    assert any(c.match < 0 for c in d) and any(c.wildcard == ord("N") for c in d) and any(c.span == 0 for c in d)
    assert any((c.mismatch, c.gap_opening, c.gap_extension) == (5, 0, 3) for c in d)


# ------------------------------------------------------------------------------------------ the checker checks
CORRUPT_KW = dict(distance="affine", span="ends-free", pattern_begin_free=8)


def corruption_corpus():
    """Twenty pairs whose oracle results hold everything the corruptions need: eight junk bases in front of the pattern (a leading D
    run that uses the whole free begin), substitutions, and three inserted bases next to one of them (an I run beside an X)."""
    rng = np.random.default_rng(2024)
    acgt = "ACGT"
    pats, txts = [], []
    for _ in range(20):
        k = 30
        s = "".join(rng.choice(list(acgt), size=60))
        s = s[:k - 1] + 3 * s[k] + s[k + 2:]
        t = list(s)
        for pos in (12, 50):
            t[pos] = acgt[(acgt.index(t[pos]) + 1 + int(rng.integers(0, 3))) % 4]
        t[k] = acgt[(acgt.index(s[k]) + 2) % 4]
        # (the inserted letter differs from s[k - 1] = s[k] = s[k + 1] and from what replaced s[k]: the run cannot slide away from the X)
        ins = 3 * acgt[(acgt.index(s[k]) + 1) % 4]
        junk = "".join(acgt[(acgt.index(s[0]) + 1 + int(rng.integers(0, 3))) % 4] for _ in range(8))
        pats.append(junk + s); txts.append("".join(t[:k]) + ins + "".join(t[k:]))
    return datagen.from_strings(pats, txts)


def test_the_checker_flags_corrupted_results():
    batch = corruption_corpus()
    cfg = loader.make_config(**CORRUPT_KW)
    o = loader.run(loader.oracle(), cfg, batch)
    cost = dp.dp_cost(batch, cfg)
    assert_optimal(cfg, batch, cost, o["score"], o["status"], o["cigars"], "corruption corpus, untouched")
    n_moved = n_priced = 0
    for i in range(20):
        p, t = datagen.pair_strings(batch, i)
        ops, score, c = o["cigars"][i].decode(), int(o["score"][i]), int(cost[i])
        assert not dp.faults(cfg, p, t, c, score, ops)
        # one M turned to X at a matching base
        k = ops.index("M", len(ops) // 2)
        assert dp.faults(cfg, p, t, c, score, ops[:k] + "X" + ops[k + 1:]), (i, "M -> X")
        assert dp.price_ops(ops[:k] + "X" + ops[k + 1:], p, t, cfg)[0] is False, (i, "M -> X is no alignment, whatever it costs")
        # one X dropped
        k = ops.index("X")
        assert dp.faults(cfg, p, t, c, score, ops[:k] + ops[k + 1:]), (i, "X dropped")
        # a score off by one extension, either way
        assert dp.faults(cfg, p, t, c, score - cfg.gap_extension, ops) and dp.faults(cfg, p, t, c, score + cfg.gap_extension, ops), (i, "score")
        # an I run moved across a mismatch: III X -> II X I (X III -> I X II), one more gap opening where the X stays a mismatch
        m = re.search("I{2,}X|XI{2,}", ops)
        if m:
            n_moved += 1
            run = m.group(0)
            moved = run[1:-1] + "XI" if run[0] == "I" else "IX" + run[2:]
            bad = ops[:m.start()] + moved + ops[m.end():]
            assert len(bad) == len(ops) and dp.faults(cfg, p, t, c, score, bad), (i, "I run moved")
            ok, pr = dp.price_ops(bad, p, t, cfg)
            if ok:
                n_priced += 1
                assert pr == c + cfg.gap_opening, (i, pr, c)
        # a free-end run one longer than its limit, priced as free: one more junk base, one more D, the same score
        lead = len(ops) - len(ops.lstrip("D"))
        assert lead == 8, (i, ops)
        p1 = "G" + p if p[0] != "G" else "C" + p
        c1 = int(dp.dp_cost(datagen.from_strings([p1], [t]), cfg)[0])
        assert dp.faults(cfg, p1, t, c1, score, "D" + ops), (i, "free run of 9")
        ok, pr = dp.price_ops("D" + ops, p1, t, cfg)
        assert ok and pr == c + cfg.gap_opening + cfg.gap_extension
    assert n_moved == 20 and n_priced == 20, (n_moved, n_priced)   # (by construction of the corpus)
