"""Recycled device memory filled with a poison byte (WFA_HIP_POISON): results must not depend on bytes nothing wrote.

The library hands pool blocks (rounded up to a power of two) from one batch to the next unchanged and keeps one workspace for every
run of an aligner; a fresh aligner's first allocation is usually a zero page, so a kernel that reads an unwritten byte sees 0 in the
rest of the suite.  Here ONE aligner runs corpora of very different sizes in a row, so that every size class is recycled into larger
and smaller requests and every run starts on the previous run's workspace — with the knob filling whatever is handed out with 0x7f
(int16 32 639, int32 2.1e9: above every real offset, out of range as an index), with 0xff (-1: negative, not the NULL offset, huge as
an unsigned number), and with the knob off (natural reuse: the previous batch's data).  Every check is exact equality with the oracle
or with the host statement of the API's own rig; nothing is compared with an unpoisoned GPU run."""
import importlib
import os

import numpy as np
import pytest

import common
import test_optimality_gpu as opt
from oracle import loader
from pywfa_amd import _native, datagen
import pywfa_amd

pytestmark = pytest.mark.gpu

POISON = ["127", "255", "0"]
F1 = opt.F1

# the cascade: every corpus of test_optimality_gpu.BUILDERS, large -> small -> large, so that blocks are recycled both ways
ORDER = ["wide", "mini", "lane", "banded", "tile", "steps", "lane", "mini"]
CONFIGS = {
    "affine-e2e": dict(span="end-to-end"),
    "affine2p-free": dict(distance="affine2p", **F1),
    "levenshtein": dict(distance="levenshtein"),
    "match-1": dict(match=-1, span="end-to-end"),
    "adaptive": dict(heuristic="adaptive", span="end-to-end"),
    "xdrop": dict(heuristic="X-drop", xdrop=100, span="end-to-end"),
    "low": dict(memory_mode="low", span="end-to-end"),
    "biwfa": dict(memory_mode="biwfa", span="end-to-end"),
}
_oracle = {}


def step_kw(name, kw, scope):
    """The configuration of one step: the step limit on `steps` (some pairs end at -100: score and status come from the limit path), the
    wildcard on `mini` (its N pairs run on bytes)."""
    kw = dict(kw, scope=scope)
    if name == "steps":
        kw["max_steps"] = 60
    if name == "mini":
        kw["wildcard"] = "N"
    return kw


def expected(name, kw):
    """(batch, oracle result, native config) of a step, the oracle run once per (corpus, configuration)."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _oracle:
        batch = opt.corpus(name, kw)
        oc, nc = common.configs_pair(**kw)
        _oracle[key] = (batch, loader.run(loader.oracle(), oc, batch), nc)
    return _oracle[key]


def run_on(al, nc, batch, full, resident):
    al.set_config(nc)
    if resident:
        rb = al.batch(batch)
        try:
            rb.run(); rb.sync()
            score, status, cig = rb.results(full)
        finally:
            rb.close()
    else:
        score, status, cig = al.align_batch(batch, full)
    cigars = None
    if full:
        ops, cbeg, clen = cig
        cigars = [ops[cbeg[i]:cbeg[i] + clen[i]].tobytes() for i in range(len(score))]
    return score, status, cigars


def cascade(order, kw, poison, monkeypatch, env=None, scopes=("score", "full")):
    """`order` on one aligner, resident batches and align_batch calls in turn, every step against the oracle."""
    monkeypatch.setenv("WFA_HIP_POISON", poison)   # (read when the aligner is created)
    for k_, v_ in (env or {}).items():
        monkeypatch.setenv(k_, v_)
    al = _native.Aligner(common.configs_pair(**kw)[1])
    try:
        for nscope, scope in enumerate(scopes):
            for step, name in enumerate(order):
                skw = step_kw(name, kw, scope)
                batch, o, nc = expected(name, skw)
                score, status, cigars = run_on(al, nc, batch, scope == "full", resident=((step + nscope) % 2 == 0))   # (the other form in the second scope)
                common.assert_same(o, score, status, cigars, batch, f"poison={poison} {env} step {step} {name} {skw}")
    finally:
        al.close()


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_cascade_on_one_aligner(gpu, cfg, poison, monkeypatch):
    cascade(ORDER, CONFIGS[cfg], poison, monkeypatch)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("cfg", ["affine-e2e", "affine2p-free"])
def test_tile_and_wide_rows_on_one_aligner(gpu, cfg, poison, monkeypatch):
    """The temporally blocked kernel under its small geometry, the wide kernel's rows over the same workspace, the tile kernel again."""
    cascade(["tile", "wide", "tile"], CONFIGS[cfg], poison, monkeypatch, env=opt.TILE_ENV)


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("cfg", ["affine-e2e", "levenshtein", "low"])
def test_cascade_without_the_single_launch_path(gpu, cfg, poison, monkeypatch):
    """WFA_HIP_NO_TINY=1: the small corpora take the batch machinery too (pool blocks of every small size class)."""
    cascade(ORDER, CONFIGS[cfg], poison, monkeypatch, env={"WFA_HIP_NO_TINY": "1"})


@pytest.mark.parametrize("poison", POISON)
def test_general_kernel_overflow_rerun(gpu, poison, monkeypatch):
    """WFA_HIP_ARENA_KB=16 is the general kernel's arena per pair (initial_arena_ints: 4 096 ints instead of about 56 000 for 300 bases),
    and with the register, banded, tile and wide stages out of the way every pair of `banded` and the byte pairs of `mini` reach that
    kernel: the arena overflows at scores of a few dozen, the pairs go to the overflow list and the synchronisation re-runs them with
    arenas 8 and 64 times larger, each time on a workspace that ensure_ws grows in mid-run."""
    env = {"WFA_HIP_ARENA_KB": "16", "WFA_HIP_NO_FAST": "1", "WFA_HIP_NO_BAND": "1", "WFA_HIP_NO_WIDE": "1", "WFA_HIP_TILE": "0", "WFA_HIP_NO_TINY": "1"}
    cascade(["banded", "mini", "banded"], CONFIGS["affine-e2e"], poison, monkeypatch, env=env, scopes=("full",))


# ------------------------------------------------------------------------------------------ single calls
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("mailbox", ["1", "0"])
@pytest.mark.parametrize("kw", [opt.ENTRY_KW[0], opt.ENTRY_KW[1], opt.ENTRY_KW[3]])
def test_align_pair_calls(gpu, kw, mailbox, poison, monkeypatch):
    """The 40 single calls of test_optimality_gpu.entry_pairs: the resident one-pair kernel (its history is the aligner's workspace) or
    a launch per call; the pairs with an N take the general form on the device copy of the pinned block."""
    monkeypatch.setenv("WFA_HIP_POISON", poison)
    monkeypatch.setenv("WFA_HIP_MAILBOX", mailbox)
    pats, txts = opt.entry_pairs(False)
    batch = datagen.from_strings(pats, txts)
    oc, nc = common.configs_pair(**kw)
    o = loader.run(loader.oracle(), oc, batch)
    full = oc.scope == 1
    al = _native.Aligner(nc)
    try:
        res = [al.align_pair(p.encode(), t.encode(), full) for p, t in zip(pats, txts)]
    finally:
        al.close()
    common.assert_same(o, np.array([r[0] for r in res]), np.array([r[1] for r in res]), [bytes(r[2]) for r in res] if full else None, batch,
                       f"align_pair poison={poison} mailbox={mailbox} {kw}")


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("scope", ["score", "full"])
def test_tiny_calls_between_batches(gpu, scope, poison, monkeypatch):
    """16 and 17 pairs (either side of the general-kernel tiny form's limit; with an N among them) around one 300-pair batch, twice."""
    monkeypatch.setenv("WFA_HIP_POISON", poison)
    kw = dict(scope=scope, wildcard="N")
    pats, txts = opt.entry_pairs(False)
    small = {n: datagen.from_strings(pats[:n], txts[:n]) for n in (16, 17)}
    oc, nc = common.configs_pair(**kw)
    big, o_big, _ = expected("lane", kw)
    o_small = {n: loader.run(loader.oracle(), oc, small[n]) for n in small}
    al = _native.Aligner(nc)
    try:
        for rnd in range(2):
            for n in (16, 17, 300, 17, 16):
                batch, o = (big, o_big) if n == 300 else (small[n], o_small[n])
                score, status, cigars = run_on(al, nc, batch, scope == "full", resident=False)
                common.assert_same(o, score, status, cigars, batch, f"tiny calls poison={poison} {scope} round {rnd} n={n}")
    finally:
        al.close()


# ------------------------------------------------------------------------------------------ resident-set APIs
# One aligner per poison value serves every step below, in this order, so that the pool blocks and the workspace of one API are what the
# next API is handed.  The steps are the smallest cases of the APIs' own modules (their assertions are the oracle and the host statements
# of the *_common.py rigs); while a step runs, the aligner those bodies create is this one: moved to the configuration they ask for, and
# left open when they close it.
class SharedAligner(_native.Aligner):
    def close(self):   # (a body's close: its resident batches go, the handle, the pool and the workspace stay for the next step)
        for rb in list(self._batches):
            rb.close()

    def really_close(self):
        _native.Aligner.close(self)


@pytest.fixture(scope="module", params=POISON)
def shared(request, gpu):
    before = os.environ.get("WFA_HIP_POISON")
    os.environ["WFA_HIP_POISON"] = request.param   # (read when the aligner is created)
    al = SharedAligner(_native.default_config(), 0)
    if before is None:
        del os.environ["WFA_HIP_POISON"]
    else:
        os.environ["WFA_HIP_POISON"] = before
    yield al
    al.really_close()


def step_cross(gpu, monkeypatch):
    """Dense 12 x 12 score matrix, its top-3 rows and a list of pairs over two resident sets, against the oracle of the 144 pairs."""
    import test_cross_topk_gpu as topk
    pats, txts = opt.entry_pairs(False)
    sel = [0, 1, 2, 3, 4, 5, 6, 9, 11, 12, 14, 17]
    P, T = [pats[i] for i in sel], [txts[i] for i in sel]
    ii, jj = np.divmod(np.arange(144), 12)
    cross = datagen.from_strings([P[i] for i in ii], [T[j] for j in jj])
    li = np.r_[np.arange(12), 11 - np.arange(12), [3, 3, 7]]
    lj = np.r_[np.arange(12), np.arange(12), [8, 8, 0]]
    for kw in (dict(span="end-to-end", scope="full"), dict(distance="affine2p", scope="score", **F1)):
        oc, _ = common.configs_pair(**kw)
        o = loader.run(loader.oracle(), oc, cross)
        al = pywfa_amd.WavefrontAligner(**kw)
        try:
            with al.sequence_set(P) as ps, al.sequence_set(T) as ts:
                score, status = al.score_matrix(ps, ts)
                assert np.array_equal(score.reshape(-1), o["score"]) and np.array_equal(status.reshape(-1), o["status"]), kw
                got = al.nearest(ps, ts, k=3)
                topk.assert_topk(got, topk.ref_topk(np.asarray(o["score"]).reshape(12, 12), np.asarray(o["status"]).reshape(12, 12), 3, False), f"{kw}")
                out = al.align_pairs(ps, ts, i=li, j=lj)
                sub = {k: [v[x] for x in li * 12 + lj] if isinstance(v, list) else np.asarray(v)[li * 12 + lj] for k, v in o.items() if v is not None}
                cigars = [np.asarray(c, np.uint8).tobytes() for c in out["cigar_ops"]] if oc.scope == 1 else None
                common.assert_same(sub, out["score"], out["status"], cigars, datagen.subset(cross, li * 12 + lj), f"align_pairs {kw}")
        finally:
            al.close()


def step_seeds(gpu, monkeypatch):
    """A k-mer index (k = 11, stride = 4) queried, another chained over the long reads (the chain workspace grows with max_anchors), then a
    minimizer index (k = 9, w = 5: its records are allocated by the counting pass's total) with seeds and chains."""
    import test_chains_gpu as chains
    import test_minimizers_gpu as minimizers
    import test_seeds_gpu as seeds
    al = _native.Aligner(_native.default_config(), 0)
    refs, reads, _ = seeds.corpus()
    T, P = seeds.native_set(al, refs), seeds.native_set(al, reads)
    seeds.test_every_index_and_query_equals_the_host_statement((al, T, P), 11, 4, 64)
    P.close(); T.close()
    T, P = chains.native_set(al, chains.long_corpus()[0]), chains.native_set(al, chains.all_reads())
    chains.test_every_index_and_query_equals_the_host_statement((al, T, P, _native.seeds_host_texts(chains.long_corpus()[0])), 11, 4, 64, 32, (5000, 500), (3, 40))
    P.close(); T.close()
    minimizers.test_seeds_and_chains_equal_the_host_statement_for_every_read(al, 9, 5)
    al.close()


def module_case(module, name, *args):
    """The test `name` of `module` as a step; MP among the arguments stands for the monkeypatch fixture."""
    def step(gpu, monkeypatch):
        getattr(importlib.import_module(module), name)(gpu, *[monkeypatch if a is MP else a for a in args])
    step.__doc__ = f"{module}.{name}{args}"
    return step


def first_aligner_shared(step):
    """`step` with only the FIRST aligner its body creates being the shared one: a body that holds two aligners of different
    configurations at once (a scope-score one beside the one under test) gets a fresh aligner for every further one, and closes it
    itself."""
    def wrapped(gpu, monkeypatch):
        same, made = _native.Aligner, []

        def once(cfg, device=0):
            made.append(cfg)
            return same(cfg, device) if len(made) == 1 else SharedAligner.__bases__[0](cfg, device)

        monkeypatch.setattr(_native, "Aligner", once)
        step(gpu, monkeypatch)
    wrapped.__doc__ = step.__doc__
    return wrapped


def step_pipeline(gpu, monkeypatch):
    """The whole paired-read pipeline with its handles held open (tests/test_pipeline_gpu.py, case 1), every call against the composed
    reference of pipeline_common."""
    import pipeline_common as pc
    import test_pipeline_gpu as pipeline
    wa = pywfa_amd.WavefrontAligner(**pc.KW)
    try:
        pipeline.test_handles_held_open_and_the_three_hand_off_traps(wa)
    finally:
        wa.close()


MP = object()
STEPS = [
    ("cross", step_cross),
    ("windows", module_case("test_windows_gpu", "test_edges_and_one_set", "full")),
    ("leftalign", module_case("test_leftalign_gpu", "test_align_windows_and_align_pairs", MP, "affine")),
    ("rle-stats", module_case("test_leftalign_gpu", "test_c_abi_stats_second_call_and_a_new_run")),
    ("pileup", module_case("test_pileup_gpu", "test_c_abi_two_adds_and_a_clear")),
    ("calls-sites", module_case("test_calls_gpu", "test_two_adds_a_clear_and_a_reopened_set", MP)),
    ("genotypes-ins", module_case("test_genotypes_gpu", "test_with_insertions_and_left_aligned")),
    ("strands-clear", module_case("test_genotypes_gpu", "test_strand_tables_in_pieces_ranges_and_after_a_clear", 3)),
    ("qualities", module_case("test_qualities_gpu", "test_keep_mask")),
    ("insertions-grow", module_case("test_insertions_gpu", "test_pieces_orders_stats_and_a_clear", MP, 3, (2, 1, 0))),
    ("placer-run", module_case("test_place_gpu", "test_add_hits_and_run_equal_the_host_statement")),
    ("placer-pairs", module_case("test_pair_gpu", "test_run_pairs_equals_the_host_statement_on_random_lists_and_edges")),
    ("rescue", module_case("test_rescue_gpu", "test_rescue_equals_the_host_statement_on_random_cases")),
    ("sam", first_aligner_shared(module_case("test_sam_gpu", "test_c_abi_two_steps_refusals_and_a_new_run"))),
    ("sam-leftalign", module_case("test_sam_gpu", "test_left_align_then_sam_and_summary_beside_sam", MP)),
    ("deletions", module_case("test_deletions_gpu", "test_pieces_orders_stats_and_a_clear", MP, 3, (2, 1, 0))),
    ("duplicates", module_case("test_dup_gpu", "test_duplicates_between_the_placers_other_runs_and_adds")),
    ("dup-ends-clips", first_aligner_shared(module_case("test_dup_ends_gpu", "test_record_kernel_stores_the_clips", MP, "edge"))),
    ("dup-ends-qsum", module_case("test_dup_ends_gpu", "test_quality_sums_at_every_offset_and_length")),
    ("seeds", step_seeds),
    ("cross-again", step_cross),
    ("pipeline", step_pipeline),
]


@pytest.mark.parametrize("step", range(len(STEPS)), ids=[name for name, _ in STEPS])
def test_resident_set_apis_in_sequence_on_one_aligner(gpu, shared, step, monkeypatch):
    """Score matrix, top-k and pair lists; windows on both strands with summaries, RLE and left-aligned gaps; pileup add / read / calls /
    sites / genotypes with the strand, quality and insertion tracks, a clear and adds that grow the tables; placer run / run_pairs /
    rescue; SAM fields (their rows and offsets are pool blocks kept across the runs of a batch), deletions, duplicates by core and by
    unclipped ends with the quality sums; the k-mer and minimizer seed indexes with query and chain; the score matrix again; the whole
    paired-read pipeline — one step per test (a few seconds each),
    in this order on the one aligner of the poison value (pytest keeps the tests of a module-scoped parameter together)."""
    def same_aligner(cfg, device=0):
        shared.set_config(cfg)
        return shared
    monkeypatch.setattr(_native, "Aligner", same_aligner)
    STEPS[step][1](gpu, monkeypatch)
