"""Windowed batches, the part that needs no GPU: the two C entries are declared, exported and bound; wfa_hip_window_2bit (the plain-C
statement of what the device gather stores) equals wfa_hip_pack_2bit of the materialised string for every start and length residue on
both strands; align_windows refuses bad arrays before it touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from pywfa_amd import WavefrontAligner, _native

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp(s):
    return s.translate(COMP)[::-1]


def header_text():
    txt = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_header_declares_both_entries():
    txt = header_text()
    assert ("wfa_hip_batch_t* wfa_hip_batch_create_windows(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* patterns, "
            "const wfa_hip_seqset_t* texts, int64_t npairs, const int32_t* i, const int32_t* j, const int32_t* p_start, "
            "const int32_t* p_len, const int32_t* t_start, const int32_t* t_len, const uint8_t* reverse);") in txt
    assert "int wfa_hip_window_2bit(const uint32_t* words, int64_t start, int32_t len, int reverse, uint32_t* out);" in txt


def test_native_lists_and_binds_both_entries():
    for name in ("wfa_hip_batch_create_windows", "wfa_hip_window_2bit"):
        assert name in _native.SYMBOLS
    L = _native.lib()
    vp = ctypes.c_void_p
    assert L.wfa_hip_batch_create_windows.argtypes == [vp, vp, vp, ctypes.c_int64] + [vp] * 7
    assert L.wfa_hip_batch_create_windows.restype is vp
    assert L.wfa_hip_window_2bit.argtypes == [vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, vp]
    assert L.wfa_hip_abi_version() == _native.ABI_VERSION
    assert callable(_native.Aligner.batch_windows) and callable(_native.ResidentBatch.windows) and callable(_native.window_2bit)


def test_null_aligner():
    L = _native.lib()
    e = np.zeros(1, np.int32)
    assert not L.wfa_hip_batch_create_windows(None, None, None, 1, e.ctypes.data, e.ctypes.data, None, None, None, None, None)
    assert L.wfa_hip_global_error().decode() == "null aligner"


def random_seq(seed, n):
    return "".join(np.array(list("ACGT"))[np.random.default_rng(seed).integers(0, 4, n)])


def check_window(seq, words, start, length, reverse):
    m = seq[start:start + length]
    want, flagged = _native.pack_2bit((revcomp(m) if reverse else m).encode())
    assert not flagged
    got = _native.window_2bit(words, start, length, reverse)
    assert got.dtype == np.uint32 and np.array_equal(got, want), (start, length, reverse)


def test_window_2bit_every_residue():
    seq = random_seq(1, 1200)
    words, _ = _native.pack_2bit(seq.encode())
    for base in (0, 336):
        for s in range(16):
            for ln in range(0, 49):           # every len % 16, three times over, len 0 and 1 among them
                for reverse in (False, True):
                    check_window(seq, words, base + s, ln, reverse)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 1199, 1200])
def test_window_2bit_ends_and_long(n):
    seq = random_seq(2, n)
    words, _ = _native.pack_2bit(seq.encode())
    for reverse in (False, True):
        check_window(seq, words, 0, n, reverse)                  # the whole sequence
        check_window(seq, words, 0, min(n, 5), reverse)          # the very start
        check_window(seq, words, n - min(n, 5), min(n, 5), reverse)   # the very end
        check_window(seq, words, n - 1, 1, reverse)
        check_window(seq, words, n, 0, reverse)
        if n > 600:
            for s in (0, 3, 16, 37):
                check_window(seq, words, s, 513, reverse)        # longer than 512 bases
                check_window(seq, words, s, n - s, reverse)


def test_window_2bit_reads_only_the_windows_words():
    """The words that hold no base of the window are not read: a window at the end of a buffer with nothing behind it."""
    seq = random_seq(3, 64)
    words, _ = _native.pack_2bit(seq.encode())
    tail = words[3:].copy()                                       # one word, bases 48 .. 63
    for reverse in (False, True):
        m = seq[48 + 5:48 + 16]
        want, _ = _native.pack_2bit((revcomp(m) if reverse else m).encode())
        assert np.array_equal(_native.window_2bit(tail, 5, 11, reverse), want)


def test_window_2bit_refuses_negative():
    L = _native.lib()
    words, out = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    assert L.wfa_hip_window_2bit(words.ctypes.data, -1, 4, 0, out.ctypes.data) == _native.EINVAL
    assert L.wfa_hip_window_2bit(words.ctypes.data, 0, -4, 0, out.ctypes.data) == _native.EINVAL
    assert L.wfa_hip_window_2bit(words.ctypes.data, 0, 4, 0, out.ctypes.data) == _native.OK
    assert L.wfa_hip_window_2bit(None, 7, 0, 1, None) == _native.OK
    with pytest.raises(ValueError):
        _native.window_2bit(words, -1, 4)
    with pytest.raises(ValueError):
        _native.window_2bit(words, 0, -4)


SEQS = ["ACGTACGTACGTACGT", "ACGTACGAACGTACGTAA", "ACGT", ""]


@pytest.mark.parametrize("kw,match", [
    (dict(i=[0, 1], j=[1.0, 2.0]), "j must hold integers"),
    (dict(i=[[0, 1]], j=[[1, 2]]), "i must be a one-dimensional"),
    (dict(i=[0, 1], j=[1]), "differ in length"),
    (dict(i=[0, 1], j=[1, 2], text_start=[0.5, 1.0]), "text_start must hold integers"),
    (dict(i=[0, 1], j=[1, 2], pattern_len=[[1, 2]]), "pattern_len must be a one-dimensional"),
    (dict(i=[0, 1], j=[1, 2], text_len=[1, 2, 3]), "text_len and i differ in length"),
    (dict(i=[0, 1], j=[1, 2], pattern_start=[0]), "pattern_start and i differ in length"),
    (dict(i=[0, 1], j=[1, 2], reverse=[1]), "reverse and i differ in length"),
    (dict(i=[0, -1], j=[1, 2]), r"i\[1\] is negative"),
    (dict(i=[0, 1], j=[1, 4]), r"j\[1\] = 4 is out of range"),
    (dict(i=[0, 1], j=[1, 2], text_start=[0, -3]), r"text_start\[1\] = -3 is negative"),
    (dict(i=[0, 1], j=[1, 2], pattern_len=[-1, 2]), r"pattern_len\[0\] = -1 is negative"),
    (dict(i=[0, 1, 0], j=[1, 2, 2], text_start=[0, 2, 3], text_len=[18, 3, 1]), r"text_start\[1\] \+ text_len\[1\] = 2 \+ 3 runs past the end of text sequence 2 \(4 bases\)"),
    (dict(i=[0, 2], j=[1, 1], pattern_start=[16, 5]), r"pattern_start\[1\] .* runs past the end of pattern sequence 2"),
    (dict(i=[0, 2], j=[1, 1], pattern_len=[16, 5]), r"pattern_len\[1\] = 0 \+ 5 runs past the end of pattern sequence 2"),
    (dict(i=[0, 1], j=[1, 2], reverse=[0, 2]), r"reverse\[1\] = 2 is neither 0 nor 1"),
    (dict(i=[0, 1], j=[1, 2], reverse=[0.0, 1.0]), "reverse must hold booleans"),
    (dict(i=[0, 1], j=[1, 2], reverse=[[True, False]]), "reverse must be a one-dimensional"),
])
def test_align_windows_refuses_before_any_device(kw, match):
    """The checks come before anything is uploaded: they pass on an object that has no native aligner at all."""
    al = object.__new__(WavefrontAligner)
    with pytest.raises(ValueError, match=match):
        al.align_windows(SEQS, **kw)
    with pytest.raises(ValueError, match=match):
        al.align_windows(SEQS, list(SEQS), **kw)
