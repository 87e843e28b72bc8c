"""Chaining on the seed index, the part that needs no GPU: the C entries are declared, exported and bound; the host-only statement
wfa_hip_chains_host (what the chain kernel computes, for one read) equals the Python restatement of the definitions in
chain_common.py (k-mer strings in a dict, sorted(), a double loop) on hand-made cases with known answers and on the long-read
corpus; every refusal names its parameter, in the C statement and in the Python form, before anything touches a device.

The hand-made cases plant chosen 8-mers into sequences of N: a k-mer over an N is no k-mer, so a case has exactly the anchors it
plants and its numbers can be worked out by hand (k = 8: cost(1) = 0, cost(5) = 1, cost(40) = 7, cost(47) = 7, cost(48) = 8)."""
import ctypes
import os
import re

import numpy as np
import pytest

from pywfa_amd import WavefrontAligner, _native
from pywfa_amd.align import SeedIndex
from chain_common import DEFAULTS, KEYS, anchor_count, cost, host_chain_rows, long_corpus, py_chains
from seed_common import LETTERS, locus_share, py_index, revcomp

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

ENTRIES = {
    "wfa_hip_seed_index_chain": "int wfa_hip_seed_index_chain(wfa_hip_seed_index_t* index, const wfa_hip_seqset_t* patterns, int n, int min_hits, "
                                "int min_score, int lookback, int max_dist, int band, int pad, int max_anchors, int32_t* j, int32_t* reverse, "
                                "int32_t* text_start, int32_t* text_len, int32_t* hits, int32_t* score, int32_t* pattern_start, "
                                "int32_t* pattern_len, uint8_t* overflow);",
    "wfa_hip_seed_index_chain_stats": "int wfa_hip_seed_index_chain_stats(const wfa_hip_seed_index_t* index, float* kernel_ms, "
                                      "int64_t* workspace_bytes);",
    "wfa_hip_chains_host": "int wfa_hip_chains_host(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, "
                           "const int64_t* t_off, const int32_t* t_len, int k, int stride, int max_occ, int n, int min_hits, int min_score, "
                           "int lookback, int max_dist, int band, int pad, int max_anchors, int32_t* j, int32_t* reverse, "
                           "int32_t* text_start, int32_t* text_len, int32_t* hits, int32_t* score, int32_t* pattern_start, "
                           "int32_t* pattern_len, uint8_t* overflow, char* msg, size_t msg_cap);",
}


def test_header_declares_and_native_binds_the_entries():
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    for decl in ENTRIES.values():
        assert decl in txt, decl
    assert "#define WFA_HIP_CHAIN_MAX_ANCHORS 65536 " in txt and "#define WFA_HIP_CHAIN_MAX_LOOKBACK 64 " in txt
    assert "32 BYTES x max_anchors PER RESIDENT WORKGROUP" in raw
    L = _native.lib()
    for name in ENTRIES:
        assert name in _native.SYMBOLS and hasattr(L, name), name
    assert _native.CHAIN_KEYS == ("j", "reverse", "text_start", "text_len", "hits", "score", "pattern_start", "pattern_len")
    assert (_native.CHAIN_MAX_LOOKBACK, _native.CHAIN_MAX_ANCHORS) == (64, 65536)
    pxd = open(os.path.join(ROOT, "pywfa_amd", "cython_shim", "wfa_hip.pxd")).read()
    for name in ENTRIES:
        assert name + "(" in pxd, name
    for f in (_native.SeedIndex.chain, _native.SeedIndex.chain_stats, _native.chains_host, SeedIndex.chains):
        assert callable(f)
    assert L.wfa_hip_seed_index_chain_stats(None, None, None) == _native.EINVAL
    assert L.wfa_hip_seed_index_chain(None, None, 4, 3, 40, 32, 5000, 500, 64, 16384, *[None] * 9) == _native.EINVAL
    assert [cost(g, 8) for g in (0, 1, 5, 40, 47, 48)] == [0, 0, 1, 7, 7, 8] and cost(65536, 15) == 15360 + 8


def rnd(seed, n):
    return LETTERS[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def plant(length, kmers):
    """`length` letters N with the given k-mers written at the given positions."""
    s = bytearray(b"N" * length)
    for pos, kmer in kmers.items():
        assert set(s[pos:pos + len(kmer)]) == {ord("N")}
        s[pos:pos + len(kmer)] = kmer
    return bytes(s)


K1, K2, K3 = b"AACCGGTA", b"CATTGACC", b"GGATCTAA"
REF = rnd(1, 400)
SMALL = dict(k=8, min_hits=2, min_score=0, pad=16)


def both(read, texts, **params):
    """The row of the host statement, which must be the row of the Python restatement: lists, and overflow."""
    p = dict(DEFAULTS, **params)
    want = py_chains(read, texts, py_index(texts, p["k"], p["stride"]), **p)
    got = _native.chains_host(read, texts, **p)
    got = {key: (got[key].tolist() if key != "overflow" else got[key]) for key in KEYS + ("overflow",)}
    assert got == want, (params, got, want)
    return got


def column(row, q):
    return tuple(row[key][q] for key in KEYS)


PAD_COLUMN = (-1, 0, 0, 0, 0, 0, 0, 0)


def test_a_perfect_chain_and_n_larger_than_the_number_of_chains():
    text = plant(400, {100: REF[:100]})
    row = both(REF[:100], [text], n=16, **SMALL)
    # 93 anchors on one diagonal, each worth one base more than the one before: f = 8 + 92
    assert column(row, 0) == (0, 0, 84, 132, 93, 100, 0, 100)
    assert all(column(row, q) == PAD_COLUMN for q in range(1, 16)) and row["overflow"] == 0
    assert both(REF[:100], [text], n=1, **SMALL)["j"] == [0]


def test_a_chain_across_an_insertion_that_splits_the_seed_clusters():
    text = plant(500, {100: REF[:200]})
    read = REF[:100] + b"N" * 40 + REF[100:200]
    row = both(read, [text], **SMALL)
    # the second half lies on diagonal 60: the step over the insertion has dr = 48, dt = 8, g = 40 and is worth 8 - cost(40) = 1
    assert column(row, 0) == (0, 0, 60 - 16, 100 + 240 + 16 - (60 - 16), 186, 100 + 1 + 92, 0, 240)
    assert column(row, 1) == PAD_COLUMN
    seeds = _native.seeds_host(read, [text], k=8, gap=16, pad=16)
    assert seeds["j"].tolist()[:3] == [0, 0, -1] and seeds["hits"].tolist()[:2] == [93, 93]
    # a band below the insertion's length: two chains of 93 again; the window of the first in the order holds the other one's anchors
    split = both(read, [text], band=39, **SMALL)
    assert column(split, 0) == (0, 0, 100 - 16, 240 + 32, 93, 100, 0, 100) and column(split, 1) == PAD_COLUMN


def three_anchors(b1, b2, a):
    """A read and a text with exactly the anchors b1, b2, a = (r, t) of K1, K2, K3 on the forward strand."""
    return plant(80, {b1[0]: K1, b2[0]: K2, a[0]: K3}), plant(300, {b1[1]: K1, b2[1]: K2, a[1]: K3})


def test_two_predecessors_tie_and_the_nearest_is_taken():
    # b1 on diagonal 105, b2 on 95, a on 100: b1 -> b2 is outside the band (g = 10); b1 -> a and b2 -> a are both worth 8 + 8 - cost(5)
    read, text = three_anchors((10, 115), (30, 125), (50, 150))
    row = both(read, [text], band=5, **SMALL)
    assert column(row, 0) == (0, 0, 95 - 16, 100 + 80 + 16 - (95 - 16), 2, 15, 30, 28)       # d_lo = 95, r_first = 30: through b2
    # with b2 gone the same anchor chains through b1
    read1, text1 = plant(80, {10: K1, 50: K3}), plant(300, {115: K1, 150: K3})
    assert column(both(read1, [text1], band=5, **SMALL), 0) == (0, 0, 100 - 16, 105 + 80 + 16 - (100 - 16), 2, 15, 10, 48)


def test_a_candidate_worth_exactly_k_is_not_adopted():
    read, text = plant(80, {10: K1, 30: K3}), plant(300, {110: K1, 178: K3})     # dr = 20, dt = 68, g = 48: 8 + 8 - cost(48) = 8
    assert column(both(read, [text], **SMALL), 0) == PAD_COLUMN
    read, text = plant(80, {10: K1, 30: K3}), plant(300, {110: K1, 177: K3})     # g = 47: worth 9
    assert column(both(read, [text], **SMALL), 0)[4:6] == (2, 9)


def test_lookback_one_against_sixty_four():
    # in the order: b (r = 10), an anchor of another text (r = 20), a (r = 30)
    read = plant(80, {10: K1, 20: K2, 30: K3})
    texts = [plant(300, {110: K1, 130: K3}), plant(50, {5: K2})]
    assert column(both(read, texts, lookback=1, **SMALL), 0) == PAD_COLUMN
    assert column(both(read, texts, lookback=64, **SMALL), 0) == (0, 0, 84, 112, 2, 16, 10, 28)
    assert column(both(read, texts, lookback=2, **SMALL), 0) == (0, 0, 84, 112, 2, 16, 10, 28)


def test_one_above_max_dist_and_one_above_band():
    read, text = plant(80, {10: K1, 40: K3}), plant(300, {110: K1, 140: K3})     # dr = dt = 30
    assert column(both(read, [text], max_dist=29, **SMALL), 0) == PAD_COLUMN
    assert column(both(read, [text], max_dist=30, **SMALL), 0)[4:6] == (2, 16)
    read, text = plant(80, {10: K1, 40: K3}), plant(300, {110: K1, 147: K3})     # dr = 30, dt = 37, g = 7
    assert column(both(read, [text], band=6, **SMALL), 0) == PAD_COLUMN
    assert column(both(read, [text], band=7, **SMALL), 0)[4:6] == (2, 8 + 8 - cost(7, 8))
    read, text = plant(80, {10: K1, 47: K3}), plant(300, {110: K1, 140: K3})     # dr = 37, dt = 30: the read side
    assert column(both(read, [text], max_dist=36, **SMALL), 0) == PAD_COLUMN
    assert column(both(read, [text], max_dist=37, band=7, **SMALL), 0)[4:6] == (2, 8 + 8 - cost(7, 8))


def test_a_read_repeated_twice_in_tandem_in_the_text():
    unit = REF[200:300]
    text = plant(500, {150: unit + unit})
    row = both(unit, [text], **SMALL)
    # both copies are whole chains of 93 anchors; the first in the order ends the first copy, whose window leaves the second copy's tail out
    assert column(row, 0) == (0, 0, 150 - 16, 132, 93, 100, 0, 100)
    assert row["j"][1] == 0 and row["text_start"][1] + row["text_len"][1] == 250 + 100 + 16 and row["hits"][1] >= 8


def test_windows_are_clipped_at_both_ends_of_a_text():
    text = REF[:110]
    row = both(text[5:105], [text], k=8, min_hits=2, min_score=0, pad=64)
    assert column(row, 0)[:4] == (0, 0, 0, 110) and column(row, 0)[6:] == (0, 100)


@pytest.mark.parametrize("reverse", (0, 1))
def test_the_pattern_window_on_either_strand(reverse):
    text = plant(400, {100: REF[:80]})
    inner = revcomp(REF[:80]) if reverse else REF[:80]
    stored = b"N" * 7 + inner + b"N" * 13
    row = both(stored, [text], **SMALL)
    j, rev, ts, tl, hits, score, ps, pl = column(row, 0)
    assert (j, rev, hits, ps, pl) == (0, reverse, 73, 7, 80)
    window = stored[ps:ps + pl]
    window = revcomp(window) if rev else window
    assert window == REF[:80] and window[:8] == text[100:108] and text[ts:ts + tl][100 - ts:][:80] == window


PARAMETER_SETS = (
    dict(),
    dict(k=11, stride=4, lookback=8, band=50, max_dist=500, n=2),
    dict(k=11, max_occ=4, min_hits=1, min_score=0, n=16, pad=0, lookback=64),
)


@pytest.mark.parametrize("params", PARAMETER_SETS, ids=("defaults", "narrow", "wide"))
def test_the_long_read_corpus(params):
    refs, reads, _ = long_corpus()
    p = dict(DEFAULTS, **params)
    want = host_chain_rows(reads, refs, **p)
    index = py_index(refs, p["k"], p["stride"])
    for i, read in enumerate(reads):
        row = py_chains(read, refs, index, **p)
        got = {key: (want[key][i].tolist() if key != "overflow" else int(want[key][i])) for key in KEYS + ("overflow",)}
        assert got == row, (i, len(read), got, row)
    assert (want["j"][len(reads) - 4:len(reads) - 1] == -1).all()                 # the empty read and the reads shorter than k
    if not params:
        assert want["j"][-1].tolist()[:2] == [0, 1] and want["pattern_start"][-1].tolist()[:2] == [0, 1500 - 1]   # the joined read
        assert want["overflow"].sum() >= 1                                         # the read over the tandem block


def test_the_overflow_boundary():
    refs, reads, _ = long_corpus()
    N = anchor_count(reads[0], refs, 13, 1, 64)
    assert 1000 < N <= 16384
    row = _native.chains_host(reads[0], refs, max_anchors=N)
    assert row["overflow"] == 0 and row["j"][0] == 0 and row["hits"][0] > 100
    row = _native.chains_host(reads[0], refs, max_anchors=N - 1)
    assert row["overflow"] == 1 and column({key: row[key].tolist() for key in KEYS}, 0) == PAD_COLUMN
    both(reads[1], refs, max_anchors=anchor_count(reads[1], refs, 13, 1, 64))
    both(reads[1], refs, max_anchors=anchor_count(reads[1], refs, 13, 1, 64) - 1)


def test_the_locus_share_of_the_host_statement():
    refs, reads, origin = long_corpus()
    assert len(origin) == 48 and sum(o[3] for o in origin) == 24 and {o[2] for o in origin} >= {1000, 6000}
    rows = host_chain_rows(reads[:len(origin)], refs, k=11, stride=4)
    share = locus_share(rows, origin)
    print(f"locus share of the host statement, k = 11, stride 4: {share:.4f}")
    assert share >= 0.95


REFUSALS = [("k", 7), ("k", 16), ("stride", 0), ("max_occ", 0), ("n", 0), ("n", 17), ("min_hits", 0), ("min_score", -1), ("lookback", 0),
            ("lookback", 65), ("max_dist", 0), ("max_dist", (1 << 20) + 1), ("band", -1), ("band", (1 << 16) + 1), ("pad", -1),
            ("max_anchors", 0), ("max_anchors", 65537)]


@pytest.mark.parametrize("name,value", REFUSALS)
def test_every_refusal_names_its_parameter(name, value):
    with pytest.raises(ValueError, match=rf"\b{name} = {value} is out of range"):
        _native.chains_host(REF[:100], [REF], **{name: value})
    if name in ("k", "stride", "max_occ"):
        return
    # the Python form refuses before it touches a device: an aligner without one, an index handle that is no handle
    al = object.__new__(WavefrontAligner)
    idx = SeedIndex(al, type("NoIndex", (), {"_h": 1, "n": 1})())
    with pytest.raises(ValueError, match=rf"\b{name} = {value} is out of range"):
        idx.chains(["ACGT"], **{name: value})


def test_other_refusals():
    idx = SeedIndex(object.__new__(WavefrontAligner), None)
    with pytest.raises(ValueError, match="seed index is closed"):
        idx.chains(["ACGT"])
    with pytest.raises(ValueError, match="must be an integer"):
        SeedIndex(object.__new__(WavefrontAligner), type("NoIndex", (), {"_h": 1, "n": 1})()).chains(["ACGT"], band=1.5)
    out = np.zeros(4, np.int32)
    over = np.zeros(1, np.uint8)
    msg = ctypes.create_string_buffer(256)
    p = out.ctypes.data_as(ctypes.c_void_p)
    rc = _native.lib().wfa_hip_chains_host(None, -1, 0, None, None, None, 13, 1, 64, 4, 3, 40, 32, 5000, 500, 64, 16384, p, p, p, p, p, p, p, p,
                                           over.ctypes.data_as(ctypes.c_void_p), msg, len(msg))
    assert rc == _native.EINVAL and b"negative length" in msg.value
    rc = _native.lib().wfa_hip_chains_host(None, 0, 0, None, None, None, 13, 1, 64, 4, 3, 40, 32, 5000, 500, 64, 16384, p, p, p, p, p, None, p, p,
                                           over.ctypes.data_as(ctypes.c_void_p), msg, len(msg))
    assert rc == _native.EINVAL and b"missing array" in msg.value
