"""Top-k per row of the score matrices (wfa_hip_cross_run_k / wfa_hip_cross_topk): the header declares both functions and both
constants, the Python binding lists and binds them, and nearest() refuses an invalid k before it touches a device (no GPU)."""
import ctypes
import os
import re

import pytest

from pywfa_amd import _native

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _header():
    return open(os.path.join(ROOT, "include", "wfa_hip.h")).read()


def test_header_declares_topk():
    txt = _header()
    assert re.search(r"#define\s+WFA_HIP_CROSS_TOPK\s+4\b", txt)
    assert re.search(r"#define\s+WFA_HIP_CROSS_MAX_K\s+64\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"wfa_hip_cross_t\*\s*wfa_hip_cross_run_k\s*\(\s*wfa_hip_aligner_t\*[^;]*int\s+want\s*,\s*int\s+k\s*\)\s*;", code)
    assert re.search(r"int\s+wfa_hip_cross_topk\s*\(\s*wfa_hip_cross_t\*[^;]*int32_t\*\s*j\s*,\s*int32_t\*\s*score\s*\)\s*;", code)


def test_binding_lists_and_binds_topk():
    assert _native.CROSS_TOPK == 4 and _native.CROSS_MAX_K == 64
    assert _native.CROSS_TOPK & (_native.CROSS_DENSE | _native.CROSS_COMPLETED) == 0
    for s in ("wfa_hip_cross_run_k", "wfa_hip_cross_topk"):
        assert s in _native.SYMBOLS
        assert hasattr(ctypes.CDLL(_native.LIB_PATH), s)
    L = _native.lib()
    assert len(L.wfa_hip_cross_run_k.argtypes) == 5 and L.wfa_hip_cross_run_k.restype is ctypes.c_void_p
    assert len(L.wfa_hip_cross_topk.argtypes) == 3


def test_topk_on_null_handle_is_einval():
    L = _native.lib()
    assert L.wfa_hip_cross_topk(None, None, None) == _native.EINVAL
    assert not L.wfa_hip_cross_run_k(None, None, None, _native.CROSS_TOPK, 1)


@pytest.mark.parametrize("k", [0, 65, -1, 1.5, "3", None, True])
def test_nearest_rejects_k_before_any_device_work(k):
    """nearest() validates k first: the aligner object is never asked to upload anything."""
    from pywfa_amd.align import WavefrontAligner
    al = WavefrontAligner.__new__(WavefrontAligner)   # (no device needed: the check comes before any use of the instance)
    with pytest.raises(ValueError, match="k must be"):
        al.nearest(["ACGT", "ACGA"], k=k)
