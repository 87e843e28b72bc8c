"""The seed finder, the part that needs no GPU: the C entries are declared, exported and bound; the host-only statement
wfa_hip_seeds_host (what the query kernel computes, for one read) equals the Python restatement of the definitions in seed_common.py
(k-mer strings in a dict, sorted()) on hand-written cases with known answers and on random sets; every refusal names its parameter,
in the C statement and in the Python forms, before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from pywfa_amd import WavefrontAligner, _native
from pywfa_amd.align import SeedIndex
from seed_common import DEFAULTS, KEYS, LETTERS, mutate, py_index, py_seeds, revcomp

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

ENTRIES = {
    "wfa_hip_seed_index_create": "wfa_hip_seed_index_t* wfa_hip_seed_index_create(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* texts, "
                                 "int k, int stride, int max_occ);",
    "wfa_hip_seed_index_destroy": "void wfa_hip_seed_index_destroy(wfa_hip_seed_index_t* index);",
    "wfa_hip_seed_index_query": "int wfa_hip_seed_index_query(wfa_hip_seed_index_t* index, const wfa_hip_seqset_t* patterns, int n, int min_hits, "
                                "int gap, int pad, int max_hits, int32_t* j, int32_t* reverse, int32_t* text_start, int32_t* text_len, "
                                "int32_t* hits, uint8_t* overflow);",
    "wfa_hip_seed_index_stats": "int wfa_hip_seed_index_stats(const wfa_hip_seed_index_t* index, int64_t* positions, int64_t* masked_kmers, "
                                "int64_t* table_bytes, float* build_ms, float* query_ms);",
    "wfa_hip_seeds_host": "int wfa_hip_seeds_host(const uint8_t* read, int32_t read_len, int64_t ntexts, const uint8_t* texts, "
                          "const int64_t* t_off, const int32_t* t_len, int k, int stride, int max_occ, int n, int min_hits, int gap, int pad, "
                          "int max_hits, int32_t* j, int32_t* reverse, int32_t* text_start, int32_t* text_len, int32_t* hits, "
                          "uint8_t* overflow, char* msg, size_t msg_cap);",
}


def test_header_declares_and_native_binds_the_entries():
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    for decl in ENTRIES.values():
        assert decl in txt, decl
    assert "#define WFA_HIP_SEED_MAX_N 16 " in txt and "#define WFA_HIP_SEED_MAX_HITS 4096 " in txt
    assert "4^k * 4 BYTES" in raw and "8 BYTES PER INDEXED POSITION" in raw
    L = _native.lib()
    for name in ENTRIES:
        assert name in _native.SYMBOLS and hasattr(L, name), name
    assert L.wfa_hip_seed_index_create.restype is ctypes.c_void_p and L.wfa_hip_seed_index_destroy.restype is None
    assert (_native.SEED_MAX_N, _native.SEED_MAX_HITS) == (16, 4096)
    pxd = open(os.path.join(ROOT, "pywfa_amd", "cython_shim", "wfa_hip.pxd")).read()
    for name in ENTRIES:
        assert name + "(" in pxd, name
    for f in (_native.Aligner.seed_index, _native.SeedIndex.query, _native.SeedIndex.stats, _native.seeds_host, WavefrontAligner.seed_index,
              SeedIndex.seeds, SeedIndex.stats, SeedIndex.close):
        assert callable(f)
    assert L.wfa_hip_seed_index_stats(None, None, None, None, None, None) == _native.EINVAL
    assert L.wfa_hip_seed_index_query(None, None, 4, 2, 16, 16, 2048, None, None, None, None, None, None) == _native.EINVAL
    L.wfa_hip_seed_index_destroy(None)


def rnd(seed, n):
    return LETTERS[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def both(read, texts, **params):
    """The host statement's row, checked against the Python restatement; returned as a dict of lists."""
    p = dict(DEFAULTS, **params)
    want = py_seeds(read, texts, py_index(texts, p["k"], p["stride"]), **p)
    got = _native.seeds_host(read, texts, **p)
    for key in KEYS:
        assert got[key].dtype == np.int32 and got[key].tolist() == want[key], (key, got[key].tolist(), want[key], p)
    assert got["overflow"] == want["overflow"], p
    return want


PAD_ROW = dict(j=[-1] * 4, reverse=[0] * 4, text_start=[0] * 4, text_len=[0] * 4, hits=[0] * 4, overflow=0)
REF = rnd(5, 400)


def test_a_read_equal_to_a_slice_and_its_reverse_complement():
    read = REF[100:160]
    row = both(read, [REF])
    # 48 13-mers on the diagonal 100; the window: 16 bases of padding on both sides of [100, 160)
    assert (row["j"], row["reverse"], row["text_start"], row["text_len"], row["hits"]) == \
        ([0, -1, -1, -1], [0, 0, 0, 0], [84, 0, 0, 0], [92, 0, 0, 0], [48, 0, 0, 0])
    row = both(revcomp(read), [REF])
    assert (row["j"][0], row["reverse"][0], row["text_start"][0], row["text_len"][0], row["hits"][0]) == (0, 1, 84, 92, 48)
    assert row["j"][1:] == [-1, -1, -1]
    both(read, [rnd(6, 300), REF, rnd(7, 20)], pad=0, gap=0)


def test_a_palindromic_kmer_hits_on_both_strands():
    pal = b"ACGTACGT"
    assert revcomp(pal) == pal
    text = b"TTTTTTTTTTTTTTTTTTTTCC" + pal + b"CCTTTTTTTTTTTTTTTTTTTTT"
    row = both(pal, [text], k=8, min_hits=1, pad=0)
    assert row["j"] == [0, 0, -1, -1] and row["reverse"] == [0, 1, 0, 0] and row["hits"] == [1, 1, 0, 0]
    assert row["text_start"][:2] == [22, 22] and row["text_len"][:2] == [8, 8]
    assert both(pal, [text], k=8, min_hits=2) == PAD_ROW


def test_a_kmer_over_an_n_is_no_kmer():
    read = bytearray(REF[100:140])
    read[20] = ord("N")
    row = both(bytes(read), [REF], k=8)
    assert row["hits"][0] == 13 + 12 and row["j"] == [0, -1, -1, -1]   # read positions 0 .. 12 and 21 .. 32
    text = bytearray(REF)
    text[120] = ord("N")
    row = both(REF[100:140], [bytes(text)], k=8)
    assert row["hits"][0] == 13 + 12
    # the N of the read against the N of the text: equal bytes, but no k-mer on either side
    assert both(bytes(read), [bytes(text)], k=8)["hits"][0] == 25
    assert both(b"N" * 40, [b"N" * 100], k=8) == PAD_ROW
    both(bytes(read).lower(), [REF], k=8)   # (lower case is outside ACGT for the C statement: no hits)


@pytest.mark.parametrize("stride,hits", [(1, 48), (4, 12)])
def test_stride(stride, hits):
    row = both(REF[100:160], [REF], stride=stride)
    assert row["hits"][0] == hits and row["text_start"][0] == 84 and row["text_len"][0] == 92
    for off in (1, 2, 3):
        both(REF[100 + off:160 + off], [REF, REF[off:]], stride=stride, gap=0)


UNIT = b"ACGGTCATTCA"
TANDEM = rnd(8, 200) + UNIT * 30 + rnd(9, 200)


def test_a_tandem_repeat_trips_max_occ():
    read = (UNIT * 30)[5:65]
    assert both(read, [TANDEM], k=8, max_occ=8) == PAD_ROW          # every k-mer of the unit occurs about 30 times
    row = both(read, [TANDEM], k=8, max_occ=64)
    assert row["overflow"] == 0 and row["hits"][0] > 64
    # a read that reaches out of the repeat keeps its unique part
    read = TANDEM[170:230]
    row = both(read, [TANDEM], k=8, max_occ=8)
    assert row["j"][0] == 0 and row["text_start"][0] == 154 and 0 < row["hits"][0] <= 30


def test_a_read_that_trips_max_hits():
    read = (UNIT * 30)[5:65]
    row = both(read, [TANDEM], k=8, max_occ=64, max_hits=64)
    assert row == dict(PAD_ROW, overflow=1)
    assert both(read, [TANDEM], k=8, max_occ=64, max_hits=4096)["overflow"] == 0
    total = sum(both(read, [TANDEM], k=8, max_occ=64, gap=1 << 20, n=16)["hits"])     # one cluster per strand and text: H itself
    assert both(read, [TANDEM], k=8, max_occ=64, max_hits=total)["overflow"] == 0
    assert both(read, [TANDEM], k=8, max_occ=64, max_hits=total - 1)["overflow"] == 1


def test_reads_shorter_than_k():
    for read in (b"", b"A", REF[100:112]):
        assert both(read, [REF]) == PAD_ROW
    assert both(REF[100:113], [REF], min_hits=1)["hits"][0] == 1
    assert both(REF[100:160], [b"", REF[:12], b"ACGT"]) == PAD_ROW


def test_windows_are_clipped_at_both_ends_of_a_text():
    row = both(REF[:50], [REF])
    assert (row["text_start"][0], row["text_len"][0]) == (0, 66)
    row = both(REF[-50:], [REF])
    assert (row["text_start"][0], row["text_len"][0]) == (400 - 50 - 16, 66)
    row = both(REF, [REF[100:160]], pad=1000)                        # the read hangs over both ends: d = -100
    assert (row["text_start"][0], row["text_len"][0], row["hits"][0]) == (0, 60, 48)
    row = both(revcomp(REF), [REF[100:160]], pad=0)
    assert (row["reverse"][0], row["text_start"][0], row["text_len"][0]) == (1, 0, 60)


def test_ties_in_hits_go_to_the_smaller_strand_text_and_diagonal():
    seg = REF[100:160]
    texts = [revcomp(REF), REF, REF, rnd(10, 50) + seg + rnd(11, 70) + seg + rnd(12, 30)]
    row = both(seg, texts, n=8)
    assert row["hits"][:5] == [48] * 5 and row["j"][5:] == [-1] * 3
    assert row["reverse"][:5] == [0, 0, 0, 0, 1] and row["j"][:5] == [1, 2, 3, 3, 0]
    assert row["text_start"][2:4] == [50 - 16, 50 + 60 + 70 - 16]
    # more hits win over the smaller strand: the reverse complement of a longer stretch
    row = both(revcomp(REF[90:170]), [rnd(13, 40) + REF[100:150] + rnd(14, 40), REF], n=2)
    assert row["reverse"] == [1, 1] and row["j"] == [1, 0] and row["hits"][0] == 68 > row["hits"][1] >= 38   # (a random flank may go on matching)
    assert both(seg, texts, n=3)["j"] == [1, 2, 3]


def test_n_larger_than_the_number_of_clusters_and_the_first_n_of_one_ranking():
    seg = REF[100:160]
    texts = [REF, rnd(15, 80) + seg[:30] + rnd(16, 80)]
    row16 = both(seg, texts, n=16)
    assert row16["j"][:2] == [0, 1] and row16["j"][2:] == [-1] * 14 and row16["hits"][2:] == [0] * 14
    for n in (1, 2, 3, 4, 15):
        row = both(seg, texts, n=n)
        for key in KEYS:
            assert row[key] == row16[key][:n]


@pytest.mark.parametrize("k", [8, 11, 13, 15])
def test_random_sets(k):
    rng = np.random.default_rng(100 + k)
    bases = [rng.integers(0, 4, n) for n in (1500, 2777, 64, 0, 3001)]
    bases[1][1000:1000 + 23 * 20] = np.tile(rng.integers(0, 4, 23), 20)
    bases[4][500:800] = np.tile(np.array([2, 3]), 150)
    texts = [bytearray(LETTERS[b].tobytes()) for b in bases]
    for a, b in [(0, 3), (700, 701), (1400, 1440), (2990, 3001)]:
        texts[4][a:b] = b"N" * (b - a)
    texts = [bytes(t) for t in texts]
    index = {stride: py_index(texts, k, stride) for stride in (1, 3, 4)}
    nonempty = 0
    for q in range(60):
        j = (0, 1, 4)[q % 3]
        ln = int(rng.integers(k - 2, 260)) if q % 10 else int(rng.integers(600, 1200))
        pos = int(rng.integers(0, len(bases[j]) - ln + 1))
        read = LETTERS[mutate(rng, bases[j][pos:pos + ln], (0.0, 0.02, 0.1)[q % 3])].tobytes()
        if q % 7 == 0:
            read = read[:len(read) // 2] + b"N" + read[len(read) // 2 + 1:]
        if q % 2:
            read = revcomp(read)
        p = dict(k=k, stride=(1, 3, 4)[q % 3], max_occ=(1, 8, 64, 1000)[q % 4], n=(1, 4, 16)[q % 3], min_hits=(1, 2, 5)[(q // 3) % 3],
                 gap=(0, 16, 3, 100000)[(q // 2) % 4], pad=(0, 16, 1000)[(q // 5) % 3], max_hits=(64, 2048, 4096)[(q // 4) % 3])
        want = py_seeds(read, texts, index[p["stride"]], **p)
        got = _native.seeds_host(read, texts, **p)
        for key in KEYS:
            assert got[key].tolist() == want[key], (q, key, p, got[key].tolist(), want[key])
        assert got["overflow"] == want["overflow"], (q, p)
        nonempty += want["j"][0] >= 0
    assert nonempty >= 20, nonempty


BAD = [("k", 7), ("k", 16), ("stride", 0), ("stride", -4), ("max_occ", 0), ("n", 0), ("n", 17), ("min_hits", 0), ("gap", -1), ("pad", -1),
       ("max_hits", 0), ("max_hits", 4097)]


@pytest.mark.parametrize("name,value", BAD)
def test_every_refusal_names_its_parameter(name, value):
    with pytest.raises(ValueError, match=rf"\b{name} = {value} is out of range"):
        _native.seeds_host(REF[100:160], [REF], **{name: value})
    # the Python forms refuse before they touch a device: an aligner without one, an index handle that is no handle
    al = object.__new__(WavefrontAligner)
    idx = SeedIndex(al, type("NoIndex", (), {"_h": 1, "n": 1})())
    with pytest.raises(ValueError, match=rf"\b{name} = {value} is out of range"):
        if name in ("k", "stride", "max_occ"):
            al.seed_index([REF.decode()], **{name: value})
        else:
            idx.seeds([REF.decode()], **{name: value})
    with pytest.raises(ValueError, match=rf"\b{name} must be an integer"):
        if name in ("k", "stride", "max_occ"):
            al.seed_index([REF.decode()], **{name: 2.5})
        else:
            idx.seeds([REF.decode()], **{name: True})


def test_other_refusals():
    al = object.__new__(WavefrontAligner)
    with pytest.raises(ValueError, match="texts = a set of 0 sequences"):
        al.seed_index([])
    idx = SeedIndex(al, None)
    for call in (lambda: idx.seeds(["ACGT"]), idx.stats, lambda: len(idx)):
        with pytest.raises(ValueError, match="seed index is closed"):
            call()
    idx.close()
    msg = ctypes.create_string_buffer(200)
    out = np.zeros(4, np.int32)
    over = np.zeros(1, np.uint8)
    p = out.ctypes.data_as(ctypes.c_void_p)
    rc = _native.lib().wfa_hip_seeds_host(None, -1, 0, None, None, None, 13, 1, 64, 4, 2, 16, 16, 2048, p, p, p, p, p,
                                          over.ctypes.data_as(ctypes.c_void_p), msg, len(msg))
    assert rc == _native.EINVAL and b"negative length" in msg.value
    rc = _native.lib().wfa_hip_seeds_host(None, 0, 0, None, None, None, 13, 1, 64, 4, 2, 16, 16, 2048, p, p, p, p, None,
                                          over.ctypes.data_as(ctypes.c_void_p), None, 0)
    assert rc == _native.EINVAL
