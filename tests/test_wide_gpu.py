"""The wide-wavefront kernel (csrc/wfa_wide.hpp: exact gap-affine alignment, one pair per workgroup, wavefront rows in LDS)
against the oracle.  Batches of more than 128 pairs so that the staged path runs (smaller batches go straight to the general
kernel); reads of 2-3 kb at 10 % without a heuristic outgrow the 256-diagonal register window, so the banded stages hand
them on (or are skipped: reads over 1.2 kb) and this kernel takes them."""
import os

import numpy as np
import pytest

import common
from corpus_common import ragged_batch
from oracle import loader
from pywfa_amd import _native, datagen

pytestmark = pytest.mark.gpu


CASES = [
    dict(span="end-to-end", scope="score"),
    dict(span="end-to-end", scope="full"),
    dict(span="ends-free", scope="full", pattern_begin_free=30, pattern_end_free=40, text_begin_free=20, text_end_free=10),
    dict(span="ends-free", scope="score", pattern_begin_free=0, pattern_end_free=0, text_begin_free=50, text_end_free=50),
    dict(span="end-to-end", scope="full", mismatch=2, gap_opening=3, gap_extension=1),
    dict(span="end-to-end", scope="full", mismatch=5, gap_opening=0, gap_extension=3),
    dict(span="end-to-end", scope="score", mismatch=1, gap_opening=1, gap_extension=1),
    dict(span="end-to-end", scope="full", mismatch=6, gap_opening=5, gap_extension=3, memory_mode="medium"),
    dict(span="end-to-end", scope="score", max_steps=300),
    dict(span="end-to-end", scope="full", max_steps=1000),
    # gap-affine-2p: the rows live in the HBM workspace (five components, M ring o2 + e2 + 1 deep)
    dict(distance="affine2p", span="end-to-end", scope="score"),
    dict(distance="affine2p", span="end-to-end", scope="full"),
    dict(distance="affine2p", span="ends-free", scope="full", pattern_begin_free=30, pattern_end_free=40, text_begin_free=20, text_end_free=10),
    dict(distance="affine2p", span="end-to-end", scope="full", mismatch=3, gap_opening=4, gap_extension=2, gap_opening2=12, gap_extension2=1),
    dict(distance="affine2p", span="end-to-end", scope="full", mismatch=2, gap_opening=2, gap_extension=2, gap_opening2=10, gap_extension2=1, memory_mode="low"),
    dict(distance="affine2p", span="end-to-end", scope="full", max_steps=700),
]


@pytest.mark.parametrize("tile", ["1", "0"])
@pytest.mark.parametrize("idx", range(len(CASES)))
def test_wide_kernel_matches_oracle(gpu, idx, tile, monkeypatch):
    """tile = 1: the temporally blocked form (csrc/wfa_tile.hpp, round 4) takes the batch first, the step-by-step form what it
    hands on; tile = 0: the step-by-step form alone (what it was before, and still is for wf-adaptive and reads over 16 kb)."""
    # (sampled in pairs of cases: CASES alternates score / full, so a stride on idx itself would tie the scope to `tile` — VERDICT r05)
    if os.environ.get("WFA_TEST_FULL") != "1" and (idx // 2 + int(tile)) % 2 == 1:
        pytest.skip("sampled on the suite's time budget (WFA_TEST_FULL=1 runs every cell)")
    monkeypatch.setenv("WFA_HIP_TILE", tile)
    batch = ragged_batch(180 if os.environ.get("WFA_TEST_FULL") == "1" else 110, 2500, 0.10, 9100 + idx)   # (the oracle's exact 2.5 kb runs are this test's time)
    kw = common.clamp_free(dict(CASES[idx]), batch)
    oc, nc = common.configs_pair(**kw)
    full = oc.scope == 1
    o = loader.run(loader.oracle(), oc, batch, want_cigar=full)
    score, status, cigars = common.gpu_run(nc, batch, full, resident=bool(idx % 2))
    common.assert_same(o, score, status, cigars, batch, f"wide {kw} tile={tile}")


TILE_GEOMETRIES = [dict(WFA_HIP_TILE_T="4", WFA_HIP_TILE_WT="64"), dict(WFA_HIP_TILE_T="16", WFA_HIP_TILE_WT="128"),
                   dict(WFA_HIP_TILE_T="8", WFA_HIP_TILE_WT="256", WFA_HIP_TILE_THREADS="128"),
                   dict(WFA_HIP_TILE_T="2", WFA_HIP_TILE_WT="64", WFA_HIP_TILE_THREADS="512"),
                   dict(WFA_HIP_TILE_T="32", WFA_HIP_TILE_WT="192", WFA_HIP_TILE_THREADS="192")]


@pytest.mark.parametrize("geo", range(len(TILE_GEOMETRIES)))
@pytest.mark.parametrize("idx", [1, 2, 4, 7, 11, 12, 13, 14])
def test_tile_kernel_geometries(gpu, idx, geo, monkeypatch):
    """The blocked form under other geometries than the defaults (steps per super-step, tile width, waves per workgroup): ring
    slots, halo widths, the far form of the M rows (gap-affine-2p with T <= 8) and the classic one, run-time penalties."""
    if os.environ.get("WFA_TEST_FULL") != "1" and ([1, 2, 4, 7, 11, 12, 13, 14].index(idx) // 2 + int(geo)) % 2 == 1:
        pytest.skip("sampled on the suite's time budget (WFA_TEST_FULL=1 runs every cell)")
    for k_, v_ in TILE_GEOMETRIES[geo].items():
        monkeypatch.setenv(k_, v_)
    batch = ragged_batch(150 if os.environ.get("WFA_TEST_FULL") == "1" else 90, 2200, 0.10, 9600 + idx)   # (the oracle's exact 2 kb runs are this test's time)
    kw = common.clamp_free(dict(CASES[idx]), batch)
    oc, nc = common.configs_pair(**kw)
    full = oc.scope == 1
    o = loader.run(loader.oracle(), oc, batch, want_cigar=full)
    score, status, cigars = common.gpu_run(nc, batch, full, resident=True)
    common.assert_same(o, score, status, cigars, batch, f"tile {kw} {TILE_GEOMETRIES[geo]}")


HANDS_ON = [dict(span="end-to-end", scope="full"), dict(span="end-to-end", scope="score", mismatch=1, gap_opening=1, gap_extension=1),
            dict(distance="affine2p", span="end-to-end", scope="full"),
            dict(span="ends-free", scope="full", pattern_begin_free=20, pattern_end_free=20, text_begin_free=10, text_end_free=10)]


@pytest.mark.parametrize("kw", HANDS_ON)
def test_tile_kernel_hands_on_what_trimming_would_change(gpu, kw, monkeypatch):
    """Unrelated sequences, prefixes and overhangs of 65-260 bases: wavefronts run into the ends of the diagonal range and gap cells
    past a sequence end lie outside their row's in-bounds cells — where the reference's per-step trimming changes values.  The
    blocked form must notice (tests/test_tile_model.py shows on the CPU that it does in most of these pairs) and hand such pairs to
    the step-by-step form: results equal the oracle's for every pair."""
    monkeypatch.setenv("WFA_HIP_NO_FAST", "1")   # (short reads: keep the register kernels out of the way, the wide-wavefront stages take the batch)
    monkeypatch.setenv("WFA_HIP_NO_BAND", "1")
    rng = np.random.default_rng(4242)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    pats, txts = [], []
    for i in range(400):
        pl = int(rng.integers(65, 260))
        p = alpha[rng.integers(0, 4, pl)]
        mode = i % 4
        if mode == 0:
            t = alpha[rng.integers(0, 4, int(rng.integers(65, 260)))]
        elif mode == 1:
            t = p[:int(rng.integers(40, pl + 1))]
        elif mode == 2:
            t = np.concatenate([alpha[rng.integers(0, 4, int(rng.integers(0, 40)))], p])
        else:
            t = p.copy()
            t[rng.integers(0, len(t), 12)] = alpha[rng.integers(0, 4, 12)]
        pats.append(p.tobytes().decode()); txts.append(t.tobytes().decode())
    batch = datagen.from_strings(pats, txts)
    kw = common.clamp_free(dict(kw), batch)
    oc, nc = common.configs_pair(**kw)
    full = oc.scope == 1
    o = loader.run(loader.oracle(), oc, batch, want_cigar=full)
    score, status, cigars = common.gpu_run(nc, batch, full, resident=True)
    common.assert_same(o, score, status, cigars, batch, f"tile, short unrelated pairs {kw}")


@pytest.mark.parametrize("scope", ["score", "full"])
def test_wide_kernel_rows_too_narrow_hand_on(gpu, scope, monkeypatch):
    """With 24 KB of LDS the rows hold a few hundred diagonals: most pairs outgrow them and are handed on to the general
    kernel; the results do not change.  (And with the kernel switched off.)"""
    monkeypatch.setenv("WFA_HIP_TILE", "0")   # (the step-by-step kernel's own forms)
    batch = ragged_batch(150, 3000, 0.10, 9200)
    oc, nc = common.configs_pair(span="end-to-end", scope=scope)
    full = scope == "full"
    o = loader.run(loader.oracle(), oc, batch, want_cigar=full)
    for env in ({"WFA_HIP_WIDE_LDS_KB": "24"}, {"WFA_HIP_NO_WIDE": "1"}, {"WFA_HIP_WIDE_THREADS": "256"}):
        for k_, v_ in env.items(): monkeypatch.setenv(k_, v_)
        score, status, cigars = common.gpu_run(nc, batch, full, resident=True)
        for k_ in env: monkeypatch.delenv(k_)
        common.assert_same(o, score, status, cigars, batch, f"wide {env}")


def test_wide_kernel_c4_as_written_sample(gpu):
    """BASELINE C4 as it is written — 10 kb, gap-affine-2p, ends-free 100 / 100, the text cut by 50 at both ends, no heuristic,
    full CIGAR — in a batch large enough for the staged path: wavefronts of ~9 000 diagonals in the 2p form of the wide kernel.
    A sample against the real library, every pair: scope=score and scope=full agree."""
    batch = datagen.trim_text(datagen.generate(132, 10000, 0.08, datagen.SEEDS["C4"]), 50)
    sel = np.r_[0:3, 129:132]
    kw = dict(distance="affine2p", span="ends-free", pattern_begin_free=100, pattern_end_free=100)
    res = {}
    for scope in ("score", "full"):
        oc, nc = common.configs_pair(**dict(kw, scope=scope))
        full = scope == "full"
        fn = loader.reference() if loader.have_reference() else loader.oracle()
        o = loader.run(fn, oc, datagen.subset(batch, sel), want_cigar=full)
        score, status, cigars = common.gpu_run(nc, batch, full, resident=True)
        assert np.array_equal(score[sel], o["score"]) and np.array_equal(status[sel], o["status"])
        if full:
            for j, i in enumerate(sel):
                assert bytes(cigars[i]) == o["cigars"][j]
        res[scope] = (score, status)
    assert np.array_equal(res["score"][0], res["full"][0]) and np.array_equal(res["score"][1], res["full"][1])


def test_wide_kernel_10kb_exact_sample(gpu):
    """BASELINE-sized reads: 10 kb at 8 % without a heuristic (wavefronts of ~5 000 diagonals), score and full CIGAR."""
    batch = datagen.generate(136, 10000, 0.08, datagen.SEEDS["C3"])
    sel = np.r_[0:6, 130:136]
    for scope in ("score", "full"):
        oc, nc = common.configs_pair(span="end-to-end", scope=scope)
        full = scope == "full"
        fn = loader.reference() if loader.have_reference() else loader.oracle()
        o = loader.run(fn, oc, datagen.subset(batch, sel), want_cigar=full)
        score, status, cigars = common.gpu_run(nc, batch, full, resident=True)
        assert np.array_equal(score[sel], o["score"]) and np.array_equal(status[sel], o["status"])
        if full:
            for j, i in enumerate(sel):
                assert bytes(cigars[i]) == o["cigars"][j]
        # every pair: full and score scopes agree (checked through the second pass of the loop)
        if scope == "score": s_score = score
        else: assert np.array_equal(s_score, score)


BEYOND_16KB = [dict(span="end-to-end", scope="score"), dict(span="end-to-end", scope="full"),
               dict(distance="affine2p", span="ends-free", pattern_end_free=50, text_end_free=50, scope="score")]


@pytest.mark.parametrize("kw", BEYOND_16KB)
@pytest.mark.parametrize("tile32", ["0", "1"])
def test_exact_reads_beyond_16kb_take_the_int32_rows(gpu, kw, tile32, monkeypatch):
    if tile32 == "1" and kw.get("scope") != "full" and os.environ.get("WFA_TEST_FULL") != "1":
        pytest.skip("the tiled int32 form: with CIGARs under -m gpu, the score forms with WFA_TEST_FULL=1 (the suite's time budget)")
    """Exact (no heuristic) alignment of reads beyond 16 kb against the oracle, score and full CIGAR; nothing is left to the general
    kernel.  Round 6: reads of up to 32 000 bases take the tiled kernel (int16 rows with NULL = -32768: csrc/wfa_tile_cell.hpp) — the
    30 kb pairs here; the 36 kb pairs take the workspace-row form of the wide-wavefront kernel with int32 offsets (VERDICT r02 item 8) or,
    with WFA_HIP_TILE32=1, the tiled kernel's int32 form (round 6: what batches of at least two pairs per CU take; sequences read from
    global memory)."""
    monkeypatch.setenv("WFA_HIP_TILE32", tile32)
    batch = datagen.generate(5, 30000, 0.06, 8801)
    long_b = datagen.generate(1, 36000, 0.05, 8802)
    batch = datagen.from_strings(*zip(*([datagen.pair_strings(batch, i) for i in range(4)] + [datagen.pair_strings(long_b, i) for i in range(1)])))
    oc, nc = common.configs_pair(**kw)
    o = loader.run(loader.oracle(), oc, batch)
    al = _native.Aligner(nc)
    rb = al.batch(batch)
    rb.run(); rb.sync()
    full = oc.scope == 1
    score, status, cig = rb.results(full)
    assert rb.fallback_pairs() == 0
    rb.close(); al.close()
    cigars = None
    if full:
        ops, cb, cl = cig
        cigars = [ops[cb[i]:cb[i] + cl[i]].tobytes() for i in range(len(score))]
    common.assert_same(o, score, status, cigars, batch, f"30 kb exact {kw}")


@pytest.mark.parametrize("idx", [0, 1, 2, 8, 9, 10, 12, 15])
def test_wide_kernel_many_pairs_take_the_workspace_rows(gpu, idx, monkeypatch):
    """Batches with pairs enough to fill every workgroup slot of the chip (>= 4 per CU) run the workspace-row form with small
    workgroups (8 x 256 threads per CU for gap-affine, 4 x 512 for gap-affine-2p: many pairs in flight per CU) instead of one
    1 024-thread workgroup with its rows in LDS; same results, nothing left to the general kernel; and the LDS form on the same
    batch when it is forced."""
    monkeypatch.setenv("WFA_HIP_TILE", "0")   # (the step-by-step kernel's own forms)
    batch = ragged_batch(1100, 1200, 0.10, 9500 + idx)   # (>= 4 pairs per CU; read length on the suite's time budget)
    kw = common.clamp_free(dict(CASES[idx]), batch)
    oc, nc = common.configs_pair(**kw)
    full = oc.scope == 1
    o = loader.run(loader.oracle(), oc, batch, want_cigar=full)
    for env in ({}, {"WFA_HIP_WIDE_GROWS": "0"}):
        for k_, v_ in env.items(): monkeypatch.setenv(k_, v_)
        score, status, cigars = common.gpu_run(nc, batch, full, resident=True)
        for k_ in env: monkeypatch.delenv(k_)
        common.assert_same(o, score, status, cigars, batch, f"wide, many pairs {kw} {env}")


ADAPT_CASES = [
    dict(span="end-to-end", scope="score", heuristic="adaptive"),
    dict(span="end-to-end", scope="full", heuristic="adaptive"),
    dict(span="end-to-end", scope="full", heuristic="adaptive", min_wavefront_length=5, max_distance_threshold=20, steps_between_cutoffs=3),
    dict(span="ends-free", scope="full", heuristic="adaptive", pattern_begin_free=30, pattern_end_free=40, text_begin_free=20, text_end_free=10),
    dict(span="end-to-end", scope="full", heuristic="adaptive", mismatch=2, gap_opening=3, gap_extension=1, max_distance_threshold=200),
    dict(distance="affine2p", span="end-to-end", scope="full", heuristic="adaptive"),
    dict(distance="affine2p", span="ends-free", scope="score", heuristic="adaptive", pattern_end_free=100, text_end_free=100, min_wavefront_length=20),
    dict(span="end-to-end", scope="full", heuristic="adaptive", max_steps=1500),
]


@pytest.mark.parametrize("lds", [1, 0, 48])
@pytest.mark.parametrize("idx", range(len(ADAPT_CASES)))
def test_wide_kernel_wf_adaptive(gpu, idx, lds, monkeypatch):
    """Round 3: the wide kernel evaluates the wf-adaptive cut-off itself (R/wavefront_heuristic.c:257-293) and takes what the banded
    stages hand on.  Here the banded stages are off and the form is forced (WFA_HIP_WIDE_ADAPT=2), so every pair runs through it:
    results must equal the oracle's, which prunes the same diagonals.  Round 4: the rows of that form live in LDS first (lds = 1),
    in the workspace for what outgrows them (0: the LDS stage off; 48: LDS rows of 48 diagonals, so most pairs take both stages)."""
    monkeypatch.setenv("WFA_HIP_NO_BAND", "1")
    monkeypatch.setenv("WFA_HIP_WIDE_ADAPT", "2")
    monkeypatch.setenv("WFA_HIP_WIDE_ADAPT_LDS", str(lds))
    batch = ragged_batch(180, 2500, 0.10, 9300 + idx)
    kw = common.clamp_free(dict(ADAPT_CASES[idx]), batch)
    oc, nc = common.configs_pair(**kw)
    full = oc.scope == 1
    o = loader.run(loader.oracle(), oc, batch, want_cigar=full)
    score, status, cigars = common.gpu_run(nc, batch, full, resident=bool(idx % 2))
    common.assert_same(o, score, status, cigars, batch, f"wide wf-adaptive {kw}")


def test_wide_kernel_takes_wf_adaptive_leftovers_of_the_banded_stages(gpu):
    """Default cascade, 30 kb reads at 12 % with a generous cut-off: some wavefronts outgrow the 256-diagonal window and the wide kernel
    (not the general kernel) finishes them; compared with the real library when it is there."""
    batch = datagen.generate(160, 30000, 0.12, 9400)
    kw = dict(span="end-to-end", scope="full", heuristic="adaptive", max_distance_threshold=400)
    oc, nc = common.configs_pair(**kw)
    fn = loader.reference() if loader.have_reference() else loader.oracle()
    o = loader.run(fn, oc, batch)
    score, status, cigars = common.gpu_run(nc, batch, True, resident=True)
    common.assert_same(o, score, status, cigars, batch, "wide takes the banded stages' wf-adaptive leftovers")


MIDLENGTH = [(600, 0.10, "affine"), (900, 0.01, "affine"), (300, 0.08, "affine2p"), (500, 0.01, "affine2p")]


@pytest.mark.parametrize("L,e,dist", MIDLENGTH)
def test_exact_midlength_batches_with_the_band_pilot(gpu, L, e, dist):
    """Round 5: exact reads of 300 - 1 200 bases in batches of >= 32 768 pairs — a pilot on 4 096 sampled pairs decides whether the
    256-diagonal register window runs before the tiled rows (csrc/wfa_hip.hip: pilot_band; 600 bp at 10 %: it does not, 900 bp at
    1 %: it does; gap-affine-2p likewise with its 192- and 256-diagonal stages) — against the oracle on every 80th pair, score and full CIGAR."""
    n = 33000
    batch = datagen.generate(n, L, e, 131)
    idx = np.arange(0, n, 80)
    sub = datagen.subset(batch, idx)
    for scope in ("score", "full"):
        oc, nc = common.configs_pair(span="end-to-end", scope=scope, distance=dist)
        full = scope == "full"
        o = loader.run(loader.oracle(), oc, sub, want_cigar=full)
        score, status, cigars = common.gpu_run(nc, batch, full, resident=True)
        assert np.array_equal(score[idx], o["score"]) and np.array_equal(status[idx], o["status"])
        if full:
            assert [cigars[i] for i in idx] == list(o["cigars"])
