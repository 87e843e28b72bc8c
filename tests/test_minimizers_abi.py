"""Minimizers, the part that needs no GPU: the C entries are declared, exported and bound; wfa_hip_minimizers_host equals the Python
restatement of the rule (minimizer_common.py: a plain loop over strings) on the lengths and letters where it can go wrong; three
properties of the rule hold exactly; the host statements of seeds and chains under a minimizer index equal the Python restatements
over a minimizer-filtered index and minimizer-filtered read positions, and with w = 1 the stride-1 host statements row for row; every
refusal names w and its value.

Density (recorded, not asserted; test_density_is_recorded prints it): on a random 60 kb sequence the share of selected positions is
0.3336 at (k, w) = (13, 5), 0.1833 at (13, 10), 0.1822 at (15, 10) and 0.1194 at (13, 16); 2 / (w + 1) gives 0.333 / 0.182 / 0.118."""
import os
import re

import numpy as np
import pytest

from pywfa_amd import WavefrontAligner, _native
from pywfa_amd.align import SeedIndex
import chain_common
import seed_common
from minimizer_common import (CHAIN_KEYS, SEED_KEYS, host_chain_rows, host_seed_rows, py_min_chains, py_min_index, py_min_seeds,
                              py_minimizers, rand, same)
from seed_common import revcomp

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KS, WS = (8, 9, 13, 15), (1, 2, 5, 10, 32)

ENTRIES = {
    "wfa_hip_seed_index_create_minimizer": "wfa_hip_seed_index_t* wfa_hip_seed_index_create_minimizer(wfa_hip_aligner_t* aligner, "
                                           "const wfa_hip_seqset_t* texts, int k, int w, int max_occ);",
    "wfa_hip_seed_index_params": "int wfa_hip_seed_index_params(const wfa_hip_seed_index_t* index, int* k, int* stride, int* w);",
    "wfa_hip_minimizers_host": "int wfa_hip_minimizers_host(const uint8_t* seq, int64_t len, int k, int w, uint8_t* selected , char* msg, "
                               "size_t msg_cap);",
    "wfa_hip_seeds_host_minimizer": "int wfa_hip_seeds_host_minimizer(const uint8_t* read, int32_t read_len, int64_t ntexts, "
                                    "const uint8_t* texts, const int64_t* t_off, const int32_t* t_len, int k, int w, int max_occ, int n, "
                                    "int min_hits, int gap, int pad, int max_hits,",
    "wfa_hip_chains_host_minimizer": "int wfa_hip_chains_host_minimizer(const uint8_t* read, int32_t read_len, int64_t ntexts, "
                                     "const uint8_t* texts, const int64_t* t_off, const int32_t* t_len, int k, int w, int max_occ, int n, "
                                     "int min_hits, int min_score, int lookback, int max_dist, int band, int pad, int max_anchors,",
}


def test_header_declares_and_native_binds_the_entries():
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    for decl in ENTRIES.values():
        assert decl in txt, decl
    assert "#define WFA_HIP_MINIMIZER_MAX_W 32 " in txt and _native.MINIMIZER_MAX_W == 32
    assert raw.index("---- minimizers") > raw.index("---- chains") and "0x85ebca6b" in raw and "0xc2b2ae35" in raw
    L = _native.lib()
    pxd = open(os.path.join(ROOT, "pywfa_amd", "cython_shim", "wfa_hip.pxd")).read()
    for name in ENTRIES:
        assert name in _native.SYMBOLS and hasattr(L, name), name
        assert name + "(" in pxd, name
    assert L.wfa_hip_seed_index_params(None, None, None, None) == _native.EINVAL
    for f in (_native.minimizers_host, _native.SeedIndex.params):
        assert callable(f)
    for prop in ("k", "w", "stride"):
        assert isinstance(getattr(SeedIndex, prop), property) and getattr(SeedIndex, prop).fset is None


def sequences(k, w):
    """name -> sequence: the lengths and letters where the rule can go wrong."""
    rng = np.random.default_rng(1000 * k + w)
    seqs = {f"len {n}": rand(rng, max(n, 0)) for n in (0, k - 1, k, k + 1, k + w - 2, k + w - 1, 15, 16, 17, 31, 32, 33)}
    seqs["len 5000"] = rand(rng, 5000)
    seqs["homopolymer"] = b"C" * 200
    base = rand(rng, 400)
    seqs["N at 0"] = b"N" + base[1:]
    seqs["N at the end"] = base[:-1] + b"N"
    seqs["N in the middle"] = base[:200] + b"N" + base[201:]
    seqs["a long N run"] = base[:150] + b"N" * (w + k + 3) + base[150:]
    seqs["lower case"] = base[:100] + base[100:140].lower() + base[140:]
    return seqs


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("w", WS)
def test_host_equals_the_restatement(k, w):
    for name, seq in sequences(k, w).items():
        got = _native.minimizers_host(seq, k, w)
        assert got.dtype == bool and got.tolist() == py_minimizers(seq, k, w), (name, k, w)
    assert _native.minimizers_host(b"C" * 200, k, w).tolist() == [True] * (200 - k + 1) + [False] * (k - 1)   # every position ties


@pytest.mark.parametrize("k", KS)
def test_w_1_selects_exactly_the_valid_kmers(k):
    for name, seq in sequences(k, 1).items():
        valid = [len(seq[p:p + k]) == k and seed_common.ACGT.issuperset(seq[p:p + k]) for p in range(len(seq))]
        assert _native.minimizers_host(seq, k, 1).tolist() == valid, name


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("w", WS)
def test_the_reverse_complement_has_the_mirrored_flags(k, w):
    for name, seq in sequences(k, w).items():
        if len(seq) < k:
            continue
        fw, rc = _native.minimizers_host(seq, k, w), _native.minimizers_host(revcomp(seq), k, w)
        n = len(seq) - k + 1     # k-mer starts: p <-> len - k - p
        assert rc[:n].tolist() == fw[:n][::-1].tolist() and not rc[n:].any() and not fw[n:].any(), (name, k, w)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("w", WS)
def test_a_shared_stretch_of_w_plus_k_minus_1_shares_a_minimizer(k, w):
    rng = np.random.default_rng(7 * k + w)
    for q in range(200):
        e = (0, 1, 7)[q % 3]
        stretch = rand(rng, w + k - 1 + e)
        a, b = int(rng.integers(0, 80)), int(rng.integers(0, 80))
        x = rand(rng, a) + stretch + rand(rng, int(rng.integers(0, 80)))
        y = rand(rng, b) + stretch + rand(rng, int(rng.integers(0, 80)))
        fx, fy = _native.minimizers_host(x, k, w), _native.minimizers_host(y, k, w)
        starts = len(stretch) - k + 1
        assert (fx[a:a + starts] & fy[b:b + starts]).any(), (k, w, q, e)


def short_corpus():
    refs, reads, _ = seed_common.corpus(nreads=48)
    return refs, reads


def long_reads():
    refs, reads, _ = chain_common.long_corpus()
    return refs, [reads[q] for q in (1, 2, 3, 9, 15, 21)] + reads[48:]     # 1 - 3 kb, the placed ones, and the reads from nowhere


@pytest.mark.parametrize("k,w", [(13, 10), (9, 5)])
def test_seeds_and_chains_host_equal_the_restatement(k, w):
    refs, reads = short_corpus()
    index = py_min_index(refs, k, w)
    for min_hits in (1, 2):
        got = host_seed_rows(reads, refs, k=k, w=w, min_hits=min_hits)
        for i, read in enumerate(reads):
            want = py_min_seeds(read, refs, index, k=k, w=w, min_hits=min_hits)
            for key in SEED_KEYS + ("overflow",):
                assert np.array_equal(got[key][i], want[key]), ("seeds", k, w, min_hits, i, key, got[key][i], want[key])
    refs, reads = long_reads()
    got = host_chain_rows(reads, refs, k=k, w=w, min_hits=2, min_score=20)
    some = 0
    for i, read in enumerate(reads):
        want = py_min_chains(read, refs, index, k=k, w=w, min_hits=2, min_score=20)
        for key in CHAIN_KEYS + ("overflow",):
            assert np.array_equal(got[key][i], want[key]), ("chains", k, w, i, key, got[key][i], want[key])
        some += want["j"][0] >= 0
    assert some >= 4


@pytest.mark.parametrize("k", [9, 13])
def test_w_1_is_the_stride_1_host_statement(k):
    refs, reads = short_corpus()
    same(host_seed_rows(reads, refs, k=k, w=1), seed_common.host_rows(reads, refs, k=k, stride=1), SEED_KEYS, ("seeds", k))
    refs, reads = long_reads()
    same(host_chain_rows(reads, refs, k=k, w=1), chain_common.host_chain_rows(reads, refs, k=k, stride=1), CHAIN_KEYS, ("chains", k))


@pytest.mark.parametrize("w", [0, 33, -1])
def test_every_refusal_names_w(w):
    for call in (lambda: _native.minimizers_host(b"ACGT" * 20, 13, w), lambda: _native.seeds_host(b"ACGT" * 20, [b"ACGT" * 30], w=w),
                 lambda: _native.chains_host(b"ACGT" * 20, [b"ACGT" * 30], w=w)):
        with pytest.raises(ValueError, match=rf"\bw = {w} is out of range \(1 \.\. 32\)"):
            call()
    al = object.__new__(WavefrontAligner)     # the Python form refuses before it touches a device
    with pytest.raises(ValueError, match=rf"\bw = {w} is out of range"):
        al.seed_index(["ACGT" * 20], w=w)
    with pytest.raises(ValueError, match=r"\bw must be an integer"):
        al.seed_index(["ACGT" * 20], w=2.5)
    with pytest.raises(ValueError, match=r"w = 10 goes with stride = 1 only"):
        al.seed_index(["ACGT" * 20], w=10, stride=4)
    for k in (7, 16):
        with pytest.raises(ValueError, match=rf"\bk = {k} is out of range"):
            _native.minimizers_host(b"ACGT" * 20, k, 10)
    with pytest.raises(ValueError, match=r"\bmax_occ = 0 is out of range"):
        _native.seeds_host(b"ACGT" * 20, [b"ACGT" * 30], w=10, max_occ=0)


def test_density_is_recorded():
    seq = rand(np.random.default_rng(60), 60000)
    for k, w in ((13, 5), (13, 10), (15, 10), (13, 16)):
        share = _native.minimizers_host(seq, k, w).sum() / (len(seq) - k + 1)
        print(f"density k = {k}, w = {w}: {share:.4f} (2 / (w + 1) = {2 / (w + 1):.4f})")
