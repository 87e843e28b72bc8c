"""Indexed batches (wfa_hip_batch_create_indexed, WavefrontAligner.align_pairs): the header declares the entry, the Python binding
lists and binds it, a NULL aligner returns NULL, and align_pairs refuses bad index arrays before it touches a device (no GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

from pywfa_amd import _native
from pywfa_amd.align import SequenceSet, WavefrontAligner

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_header_declares_indexed_batch():
    txt = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"wfa_hip_batch_t\*\s*wfa_hip_batch_create_indexed\s*\(\s*wfa_hip_aligner_t\*\s*aligner\s*,\s*"
                     r"const\s+wfa_hip_seqset_t\*\s*patterns\s*,\s*const\s+wfa_hip_seqset_t\*\s*texts\s*,\s*"
                     r"int64_t\s+npairs\s*,\s*const\s+int32_t\*\s*i\s*,\s*const\s+int32_t\*\s*j\s*\)\s*;", code)


def test_binding_lists_and_binds_indexed_batch():
    s = "wfa_hip_batch_create_indexed"
    assert s in _native.SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), s)
    L = _native.lib()
    assert len(L.wfa_hip_batch_create_indexed.argtypes) == 6 and L.wfa_hip_batch_create_indexed.restype is ctypes.c_void_p
    assert hasattr(_native.Aligner, "batch_indexed") and hasattr(_native.ResidentBatch, "indexed")


def test_null_aligner_returns_null():
    L = _native.lib()
    i = np.zeros(1, np.int32)
    assert not L.wfa_hip_batch_create_indexed(None, None, None, 0, None, None)
    assert not L.wfa_hip_batch_create_indexed(None, None, None, 1, i.ctypes.data, i.ctypes.data)
    assert b"null aligner" in L.wfa_hip_global_error()


def _bare():
    return WavefrontAligner.__new__(WavefrontAligner)   # (no device needed: the checks come before any use of the instance)


SEQS = ["ACGT", "ACGA", "AC"]


@pytest.mark.parametrize("i,j,msg", [
    ([0, 1], [0], "differ in length"),
    ([0], [0, 1, 2], "differ in length"),
    ([0.0, 1.0], [0, 1], "integers"),
    (np.array([0.5]), np.array([0]), "integers"),
    ([True, False], [0, 1], "integers"),
    (np.array([0, 1]), np.array([True, False]), "integers"),
    (["0", "1"], [0, 1], "integers"),
    ([0, 1], "01", "one-dimensional|integers"),
    ([[0, 1]], [[0, 1]], "one-dimensional"),
    ([0, -1], [0, 1], "negative"),
    ([0, 1], [2, -1], r"j\[1\] is negative.*filter"),
    ([3], [0], r"i\[0\] = 3 is out of range"),
    ([0, 1], [1, 3], r"j\[1\] = 3 is out of range"),
    (np.array([2 ** 32], np.int64), np.array([0], np.int64), "out of range"),
    (None, [0], "i is missing"),
    ([0], None, "j is missing"),
])
def test_align_pairs_rejects_indices_before_any_device_work(i, j, msg):
    with pytest.raises(ValueError, match=msg):
        _bare().align_pairs(SEQS, i=i, j=j)


def test_align_pairs_checks_each_index_against_its_own_set():
    with pytest.raises(ValueError, match=r"j\[0\] = 1 is out of range for a set of 1"):
        _bare().align_pairs(SEQS, ["ACGT"], i=[2], j=[1])
    with pytest.raises(ValueError, match=r"i\[1\] = 1 is out of range for a set of 1"):
        _bare().align_pairs(["ACGT"], SEQS, i=[0, 1], j=[2, 2])
    with pytest.raises(ValueError, match="out of range for a set of 0"):
        _bare().align_pairs([], i=[0], j=[0])


def test_index_arrays_are_keyword_only():
    with pytest.raises(TypeError):
        _bare().align_pairs(SEQS, None, [0], [0])


def test_sequence_set_handle_surface():
    assert hasattr(WavefrontAligner, "sequence_set") and hasattr(WavefrontAligner, "align_pairs")
    for name in ("__len__", "close", "__enter__", "__exit__"):
        assert hasattr(SequenceSet, name)
    s = SequenceSet(None, None)   # a closed handle
    s.close()
    with pytest.raises(ValueError, match="closed"):
        len(s)
    with pytest.raises(ValueError, match="closed"):
        _bare().align_pairs(s, i=[0], j=[0])
