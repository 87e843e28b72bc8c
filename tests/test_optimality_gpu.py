"""The HIP path against the plain recurrence of tests/dp_reference.py: the reported score is the optimum of the penalty model and
the op string is an alignment of that cost.  The recurrence shares nothing with the wavefront algorithm, so this holds where the
oracle and the kernels could be wrong together.  The recurrence's cost depends on the corpus, the penalties, the span and the
wildcard only — not on scope, memory mode, heuristic, route or entry point — and is computed once per such key."""
import numpy as np
import pytest

import common
import corpus_common
import dp_reference as dp
from oracle import loader
from pywfa_amd import _native, datagen
from test_dp_reference import assert_optimal, fit_free

pytestmark = pytest.mark.gpu

# the smallest corpora that still reach each kernel family (batches above 128 pairs take the staged path)
BUILDERS = {
    "mini": lambda: corpus_common.special_mini(__import__("validate_oracle").corpus_special(seed=99)),   # single-launch path
    "lane": lambda: datagen.generate(300, 150, 0.04, 6150),                                             # lane / segment cascade
    "banded": lambda: corpus_common.ragged_batch(140, 300, 0.10, 6300),                                 # banded / slim
    "tile": lambda: corpus_common.ragged_batch(140, 600, 0.10, 6600),                                   # tile, small geometry
    "wide": lambda: corpus_common.ragged_batch(140, 1300, 0.08, 7300),                                  # wide / tile / BiWFA splitting
    # the step limits 10 and 60: costs of about 6, 30 and 130 in one batch, so that pairs fall on both sides of either limit
    "steps": lambda: datagen.from_strings(*zip(*[datagen.pair_strings(b, i) for b in (datagen.generate(120, 150, 0.01, 6151), datagen.generate(120, 150, 0.05, 6152),
                                                                                      datagen.generate(60, 300, 0.10, 6153)) for i in range(len(b["p_len"]))])),
}
_corpora, _costs = {}, {}


def corpus(name, kw):
    if name not in _corpora:
        _corpora[name] = BUILDERS[name]()
    return fit_free(_corpora[name], kw, keep=len(_corpora[name]["p_len"]) if name != "mini" else 0)


def cost_of(name, kw):
    """(batch, config pair, recurrence cost) of a configuration on a corpus; the cost cached per (corpus, penalties, span, wildcard)."""
    batch = corpus(name, kw)
    oc, nc = common.configs_pair(**kw)
    m = dp.Model(oc)
    key = (name, m.distance, m.match, m.x, tuple(m.pieces), m.free, m.wildcard)
    if key not in _costs:
        _costs[key] = dp.dp_cost(batch, oc)
        _costs[key].setflags(write=False)
    return batch, oc, nc, _costs[key]


def run(nc, batch, full, resident, want_no_fallback=False):
    if not want_no_fallback:
        return common.gpu_run(nc, batch, full, resident)
    al = _native.Aligner(nc)
    try:
        rb = al.batch(batch)
        rb.run(); rb.sync()
        score, status, cig = rb.results(full)
        assert rb.fallback_pairs() == 0   # (the kernel family this test means took every pair: a reroute would make it a test of the general kernel)
        rb.close()
    finally:
        al.close()
    return score, status, ([dp.ops_of(cig, i) for i in range(len(score))] if full else None)


F0, F1, F2 = dict(), dict(pattern_begin_free=8, pattern_end_free=7, text_begin_free=3, text_end_free=2), dict(pattern_begin_free=20, text_end_free=9)
EXACT = [dict(distance=d, **f) for d in ("indel", "levenshtein", "linear", "affine", "affine2p") for f in (dict(span="end-to-end"), F0, F1, F2)]
EXACT += [
    dict(mismatch=2, gap_opening=3, gap_extension=1), dict(mismatch=5, gap_opening=0, gap_extension=3, span="end-to-end"),
    dict(mismatch=2, gap_opening=3, gap_extension=1, **F1), dict(mismatch=5, gap_opening=0, gap_extension=3, **F2),
    dict(distance="affine2p", mismatch=3, gap_opening=4, gap_extension=2, gap_opening2=12, gap_extension2=1),
    dict(distance="affine2p", mismatch=3, gap_opening=4, gap_extension=2, gap_opening2=12, gap_extension2=1, **F1),
    dict(match=-1, span="end-to-end"), dict(distance="affine2p", match=-1, span="end-to-end"), dict(distance="linear", match=-1, span="end-to-end"),
    dict(wildcard="N"), dict(wildcard="N", distance="affine2p", **F1), dict(wildcard="N", distance="levenshtein", span="end-to-end"),
    dict(memory_mode="medium"), dict(memory_mode="medium", **F1), dict(memory_mode="low", distance="affine2p", span="end-to-end"),
    dict(memory_mode="low", **F2),
    dict(memory_mode="biwfa", span="end-to-end"), dict(memory_mode="biwfa", distance="affine2p"), dict(memory_mode="biwfa", distance="levenshtein", span="end-to-end"),
    dict(memory_mode="biwfa", mismatch=2, gap_opening=3, gap_extension=1), dict(memory_mode="biwfa", match=-1, span="end-to-end"),
    dict(memory_mode="biwfa", wildcard="N"),
]


def check(name, kw, routes, monkeypatch, ctx):
    """Both scopes of `kw` on corpus `name` through every route (environment, resident, no fallback allowed)."""
    for scope in ("score", "full"):
        batch, oc, nc, cost = cost_of(name, dict(kw, scope=scope))
        for env, resident, strict in routes:
            for k_, v_ in env.items():
                monkeypatch.setenv(k_, v_)
            score, status, cigars = run(nc, batch, scope == "full", resident, strict)
            for k_ in env:
                monkeypatch.delenv(k_)
            assert_optimal(oc, batch, cost, score, status, cigars, f"{ctx} {name} {kw} {scope} {env} resident={resident}",
                           unset_ok=(kw.get("memory_mode") == "biwfa" and scope == "full"))


@pytest.mark.parametrize("cfg_idx", range(len(EXACT)))
def test_single_launch_path_is_optimal(gpu, cfg_idx, monkeypatch):
    """The 64 edge-case pairs (empty, length 1, unrelated, repeats, N, long gaps, windows) in one non-resident call: the single-launch
    path; and the batch machinery on the same pairs."""
    check("mini", EXACT[cfg_idx], [({}, False, False), ({"WFA_HIP_NO_TINY": "1"}, cfg_idx % 2 == 0, False)], monkeypatch, "single launch")


@pytest.mark.parametrize("cfg_idx", range(len(EXACT)))
def test_lane_and_segment_cascade_is_optimal(gpu, cfg_idx, monkeypatch):
    """300 pairs of 150 bases at 4 %: the staged path of short reads (lane kernel, segments, what they hand on)."""
    check("lane", EXACT[cfg_idx], [({}, True, False), ({"WFA_HIP_NO_TINY": "1"}, False, False)], monkeypatch, "lane cascade")


@pytest.mark.parametrize("stages", ["0189", "689", "245", "2", "98"])
def test_stage_orders_are_optimal(gpu, stages, monkeypatch):
    for kw in (dict(span="end-to-end"), dict(span="end-to-end", mismatch=2, gap_opening=3, gap_extension=1)):
        check("lane", kw, [({"WFA_HIP_FAST_STAGES": stages}, True, False)], monkeypatch, "stage order")
        check("banded", kw, [({"WFA_HIP_FAST_STAGES": stages}, True, False)], monkeypatch, "stage order")


LONG = [dict(span="end-to-end"), dict(**F2), dict(distance="affine2p", span="end-to-end"), dict(distance="affine2p", **F1),
        dict(mismatch=2, gap_opening=3, gap_extension=1, span="end-to-end"), dict(mismatch=5, gap_opening=0, gap_extension=3),
        dict(distance="affine2p", mismatch=3, gap_opening=4, gap_extension=2, gap_opening2=12, gap_extension2=1, span="end-to-end"),
        dict(distance="levenshtein", span="end-to-end"), dict(distance="linear", **F1), dict(distance="indel"),
        dict(match=-1, span="end-to-end"), dict(memory_mode="medium", span="end-to-end"), dict(memory_mode="low", **F2),
        dict(memory_mode="biwfa", span="end-to-end"), dict(memory_mode="biwfa", distance="affine2p")]


@pytest.mark.parametrize("slim", ["1", "0"])
@pytest.mark.parametrize("cfg_idx", range(len(LONG)))
def test_banded_and_slim_kernels_are_optimal(gpu, cfg_idx, slim, monkeypatch):
    """140 ragged pairs of 300 bases at 10 %: what the register cascade hands on and the banded stages (slim step or not) take."""
    check("banded", LONG[cfg_idx], [({"WFA_HIP_BAND_SLIM": slim}, cfg_idx % 2 == 0, False)], monkeypatch, "banded")


TILE_ENV = dict(WFA_HIP_NO_FAST="1", WFA_HIP_NO_BAND="1", WFA_HIP_TILE="1", WFA_HIP_TILE_T="4", WFA_HIP_TILE_WT="64")


@pytest.mark.parametrize("cfg_idx", [0, 1, 2, 3, 4, 6, 11, 12])
def test_tile_kernel_small_geometry_is_optimal(gpu, cfg_idx, monkeypatch):
    """140 ragged pairs of 600 bases at 10 % with the register and banded stages out of the way: the temporally blocked form under
    a small geometry (4 steps per super-step, tiles of 64 diagonals: many tiles, many halo exchanges) and the step-by-step form
    for what it hands on; nothing may reach the general kernel."""
    check("tile", LONG[cfg_idx], [(TILE_ENV, True, True)], monkeypatch, "tile")


@pytest.mark.parametrize("tile", ["1", "0"])
@pytest.mark.parametrize("cfg_idx", [0, 1, 2])
def test_wide_kernels_are_optimal(gpu, cfg_idx, tile, monkeypatch):
    """140 ragged pairs of 1.3 kb at 8 % without a heuristic: the wavefronts outgrow the register window; the tiled form (1) or the
    step-by-step form alone (0) takes them, nothing reaches the general kernel."""
    check("wide", LONG[cfg_idx], [({"WFA_HIP_TILE": tile}, True, True)], monkeypatch, "wide")


@pytest.mark.parametrize("bilevel", ["1", "0"])
@pytest.mark.parametrize("kw", [dict(memory_mode="biwfa", span="end-to-end"), dict(memory_mode="biwfa", distance="affine2p", span="end-to-end"),
                                dict(memory_mode="low", span="end-to-end")])
def test_biwfa_splitting_is_optimal(gpu, kw, bilevel, monkeypatch):
    """The same 1.3 kb pairs score far above 250, so BiWFA splits every long pair at breakpoints (level by level, or depth first
    with WFA_HIP_BILEVEL=0); the halves' op strings joined must still cost the optimum.  The score may be unset (Appendix B Q6)."""
    batch, oc, nc, cost = cost_of("wide", dict(kw, scope="full"))
    assert int((cost > 250).sum()) >= 100
    check("wide", kw, [({"WFA_HIP_BILEVEL": bilevel}, True, False)], monkeypatch, "biwfa")


# ------------------------------------------------------------------------------------------ entry points
ENTRY_KW = [dict(span="end-to-end", scope="full"), dict(distance="affine2p", scope="full", **F1), dict(distance="levenshtein", scope="full"),
            dict(span="end-to-end", scope="score"), dict(match=-1, span="end-to-end", scope="full")]


def entry_pairs(acgt_only):
    """40 pairs of 150 bases with ragged lengths and a long gap; unless `acgt_only`, an N here and there."""
    base = datagen.generate(40, 150, 0.04, 4713)
    pats, txts = [], []
    for i in range(40):
        p, t = datagen.pair_strings(base, i)
        if i % 8 == 1: p = p[:40 + i]
        if i % 8 == 3 and not acgt_only: t = t[:50] + "N" + t[51:]
        if i % 8 == 4 and not acgt_only: p = p[:60] + "N" + p[61:]
        if i % 8 == 6: t = t[:60] + t[90:]
        pats.append(p); txts.append(t)
    return pats, txts


def entry_costs(kw, acgt_only=False):
    key = ("entry", acgt_only, tuple(sorted((k, v) for k, v in kw.items() if k != "scope")))
    pats, txts = entry_pairs(acgt_only)
    batch = datagen.from_strings(pats, txts)
    oc, nc = common.configs_pair(**kw)
    if key not in _costs:
        _costs[key] = dp.dp_cost(batch, oc)
    return pats, txts, batch, oc, nc, _costs[key]


@pytest.mark.parametrize("kw", ENTRY_KW)
@pytest.mark.parametrize("entry", ["align_batch", "resident", "packed2bits"])
def test_batch_entry_points_are_optimal(gpu, entry, kw):
    pats, txts, batch, oc, nc, cost = entry_costs(kw, acgt_only=(entry == "packed2bits"))
    full = oc.scope == 1
    if entry == "packed2bits":
        al = _native.Aligner(nc)
        score, status, cig = al.align_batch(datagen.to_packed2bits(batch), full)
        al.close()
        cigars = [dp.ops_of(cig, i) for i in range(40)] if full else None
    else:
        score, status, cigars = common.gpu_run(nc, batch, full, resident=(entry == "resident"))
    assert_optimal(oc, batch, cost, score, status, cigars, f"{entry} {kw}")


@pytest.mark.parametrize("kw", ENTRY_KW)
@pytest.mark.parametrize("mailbox", ["1", "0"])
def test_align_pair_calls_are_optimal(gpu, mailbox, kw, monkeypatch):
    """40 calls in a row: served from the mailbox by the kernel that stays on the device, or a launch per call."""
    monkeypatch.setenv("WFA_HIP_MAILBOX", mailbox)   # (read when the aligner is created)
    pats, txts, batch, oc, nc, cost = entry_costs(kw)
    full = oc.scope == 1
    al = _native.Aligner(nc)
    try:
        res = [al.align_pair(p.encode(), t.encode(), full) for p, t in zip(pats, txts)]
    finally:
        al.close()
    assert_optimal(oc, batch, cost, [r[0] for r in res], [r[1] for r in res], [r[2] for r in res] if full else None, f"align_pair mailbox={mailbox} {kw}")


@pytest.mark.parametrize("kw", ENTRY_KW)
def test_score_matrix_and_pair_lists_are_optimal(gpu, kw):
    """A dense 12 x 12 score matrix over two resident sets — every read against every text, related or not — and one list of pairs
    over the same sets, with op strings under scope full."""
    import pywfa_amd
    pats, txts, _, _, _, _ = entry_costs(kw)
    sel = [0, 1, 2, 3, 4, 5, 6, 9, 11, 12, 14, 17]   # (truncated patterns, N on either side, a long gap, plain pairs)
    P, T = [pats[i] for i in sel], [txts[i] for i in sel]
    if any(kw.get(k, 0) for k in ("pattern_begin_free", "pattern_end_free", "text_begin_free", "text_end_free")):
        assert min(map(len, P)) >= 8 and min(map(len, T)) >= 3
    ii, jj = np.divmod(np.arange(144), 12)
    cross = datagen.from_strings([P[i] for i in ii], [T[j] for j in jj])
    oc, _ = common.configs_pair(**kw)
    key = ("cross",) + tuple(sorted((k, v) for k, v in kw.items() if k != "scope"))
    if key not in _costs:
        _costs[key] = dp.dp_cost(cross, oc)
    cost = _costs[key]
    al = pywfa_amd.WavefrontAligner(**kw)
    try:
        with al.sequence_set(P) as ps, al.sequence_set(T) as ts:
            score, status = al.score_matrix(ps, ts)
            # (a score matrix carries no op strings and runs in score scope: there the score is set in every memory mode)
            assert_optimal(oc, cross, cost, score.reshape(-1), status.reshape(-1), None, f"score_matrix {kw}")
            li = np.r_[np.arange(12), 11 - np.arange(12), [3, 3, 7]]
            lj = np.r_[np.arange(12), np.arange(12), [8, 8, 0]]
            out = al.align_pairs(ps, ts, i=li, j=lj)
            sub = datagen.subset(cross, li * 12 + lj)
            cigars = [np.asarray(c, np.uint8).tobytes() for c in out["cigar_ops"]] if oc.scope == 1 else None
            assert_optimal(oc, sub, cost[li * 12 + lj], out["score"], out["status"], cigars, f"align_pairs {kw}")
    finally:
        al.close()


# ------------------------------------------------------------------------------------------ the step limit
@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("name,max_steps,kw", [("steps", 10, dict(span="end-to-end")), ("steps", 10, dict(distance="affine2p", **F1)),
                                              ("steps", 60, dict(span="end-to-end")), ("steps", 60, dict(**F2)), ("steps", 60, dict(mismatch=5, gap_opening=0, gap_extension=3)),
                                              ("tile", 300, dict(span="end-to-end")), ("tile", 300, dict(distance="affine2p", span="end-to-end"))])
def test_step_limit_splits_the_pairs_exactly(gpu, name, max_steps, kw, resident):
    """match == 0: a pair whose optimum is below the limit completes with that cost, a pair at or above it ends with status -100 and
    score -max_steps (oracle/wfa_oracle.c:740-745) — exactly, on corpora with at least ten pairs of either kind."""
    for scope in ("score", "full"):
        batch, oc, nc, cost = cost_of(name, dict(kw, scope=scope))
        below = cost < max_steps
        assert int(below.sum()) >= 10 and int((~below).sum()) >= 10, (int(below.sum()), int((~below).sum()))
        _, nc = common.configs_pair(**dict(kw, scope=scope, max_steps=max_steps))
        score, status, cigars = common.gpu_run(nc, batch, scope == "full", resident)
        ctx = f"max_steps={max_steps} {name} {kw} {scope}"
        assert np.array_equal(status == 0, below), (ctx, np.flatnonzero((status == 0) != below)[:5])
        assert (status[~below] == -100).all() and (score[~below] == -max_steps).all(), ctx
        idx = np.flatnonzero(below)
        assert_optimal(oc, datagen.subset(batch, idx), cost[idx], score[idx], status[idx], None if cigars is None else [cigars[i] for i in idx], ctx)


# ------------------------------------------------------------------------------------------ heuristics: a lower bound only
HEUR = [("lane", dict(heuristic="adaptive", span="end-to-end")), ("lane", dict(heuristic="adaptive", **F1)),
        ("lane", dict(heuristic="adaptive", distance="affine2p", span="end-to-end", min_wavefront_length=5, max_distance_threshold=10, steps_between_cutoffs=3)),
        ("banded", dict(heuristic="adaptive", span="end-to-end")), ("banded", dict(heuristic="adaptive", distance="affine2p", **F2)),
        ("tile", dict(heuristic="adaptive", span="end-to-end", min_wavefront_length=5, max_distance_threshold=20, steps_between_cutoffs=3)),
        ("wide", dict(heuristic="adaptive", span="end-to-end")),
        ("lane", dict(heuristic="X-drop", xdrop=100, match=-1, span="end-to-end")), ("banded", dict(heuristic="X-drop", xdrop=1000, span="end-to-end")),
        ("lane", dict(heuristic="X-drop", xdrop=400, span="end-to-end")), ("mini", dict(heuristic="X-drop", xdrop=1000, **F0)),
        ("mini", dict(heuristic="adaptive", **F0))]


@pytest.mark.parametrize("idx", range(len(HEUR)))
def test_heuristic_results_are_alignments_of_their_score_and_no_better_than_the_optimum(gpu, idx):
    """wf-adaptive and X-drop, scope full: a completed pair carries a valid op string whose price is the reported penalty, and that
    penalty is at least the recurrence's (one commented exception below, gap-affine two-piece: banded pair 17 under F2 reports 196
    for an op string the model prices 188).  How often a heuristic is optimal is not asserted — nobody has measured it.  The inputs
    are ones on which the oracle completes at least 90 % of the pairs (checked on the CPU), and so must the GPU."""
    name, kw = HEUR[idx]
    batch, oc, nc, cost = cost_of(name, dict(kw, scope="full"))
    score, status, cigars = common.gpu_run(nc, batch, True, resident=(idx % 2 == 0))
    done = np.flatnonzero(status == 0)
    assert len(done) >= 0.9 * len(status), (name, kw, len(done), len(status))
    for i in done:
        p, t = datagen.pair_strings(batch, i)
        ok, price = dp.price_ops(cigars[i], p, t, oc)
        assert ok, (name, kw, i, "the op string is no alignment of the pair")
        reported = dp.penalty_of_score(score[i], oc)
        if oc.distance == dp.AFFINE2P and price != reported:
            # The one exception: under gap-affine two-piece a cut-off can leave a long gap in the first piece's
            # component only, so the walk pays o1 + n e1 where the model prices the same run min(o1 + n e1, o2 + n e2) — the
            # reported penalty is then the price plus the piece differences of some of the op string's gaps, and nothing else.
            assert reported - price in dp.two_piece_slack(cigars[i], p, t, oc), (name, kw, i, price, reported)
        else:
            assert price == reported, (name, kw, i, price, int(score[i]))
        assert price >= cost[i], (name, kw, i, "better than the optimum", price, int(cost[i]))
