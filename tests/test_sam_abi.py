"""The SAM fields without a GPU: the host statement of the rule (wfa_hip_ops_sam) against its Python restatement (sam_common.py) on the
examples of include/wfa_hip.h and on the ORACLE's op strings of the repeat corpus, the properties a SAM reader relies on, the
refusals, and the new keywords of the Python surface."""
import inspect

import numpy as np
import pytest

from pywfa_amd import WavefrontAligner, _native
from sam_common import CORE, EQX, FLAGS, MD_FORM, UNMAPPED, corpus_strings, py_sam, ref_from, span_counts

EXAMPLES = [
    (b"MMXMIIMDM", b"ACGTACGT", 0, b"4M2D1M1I1M", b"2G1^AC2", (0, 8, 0, 0, 4, 10, 7, 7)),
    (b"MMXMIIMDM", b"ACGTACGT", EQX, b"2=1X1=2D1=1I1=", b"2G1^AC2", (0, 8, 0, 0, 4, 14, 7, 7)),
    (b"DDIIIMMMXMD", b"ACGTACGT", 0, b"2S5M1S", b"3G1", (3, 5, 2, 1, 1, 6, 3, 5)),
    (b"XMMMX", b"ACGTA", 0, b"5M", b"0A3A0", (0, 5, 0, 0, 2, 2, 5, 5)),
    (b"XMMMX", b"ACGTA", CORE, b"1S3M1S", b"3", (1, 3, 1, 1, 0, 6, 1, 3)),
    (b"MIIDIIXM", b"ACGTACG", 0, b"1M2D1I2D2M", b"1^CG0^TA0C1", (0, 7, 0, 0, 6, 10, 11, 4)),
]


def plen_of(ops):
    return sum(c in b"MXD" for c in ops)


@pytest.mark.parametrize("ops,text,flags,cigar,md,row", EXAMPLES)
def test_the_examples_of_the_header(ops, text, flags, cigar, md, row):
    assert py_sam(ops, text, flags) == (row, cigar, md)
    got = _native.ops_sam(ops, text, plen_of(ops), flags)
    assert (tuple(got[0]), got[1], got[2]) == (row, cigar, md)


@pytest.mark.parametrize("metric", ["affine", "levenshtein", "indel"])
def test_host_rule_equals_the_restatement_on_the_oracles_strings(metric):
    pats, txts, cigars, status = corpus_strings(metric)
    assert (status == 0).all() and len(cigars) == 500
    kinds = set()
    for flags in FLAGS:
        for p, t, ops in zip(pats, txts, cigars):
            want = py_sam(ops, t.encode(), flags)
            got = _native.ops_sam(ops, t.encode(), len(p), flags)
            assert (tuple(got[0]), got[1], got[2]) == want, (metric, flags, ops)
            kinds.update(chr(c) for c in want[1] if not chr(c).isdigit())
    assert kinds >= set("M=XID" if metric != "indel" else "M=ID"), kinds


@pytest.mark.parametrize("metric", ["affine", "levenshtein", "indel"])
def test_a_reader_rebuilds_the_reference_from_read_cigar_and_md(metric):
    """Every end free: leading and trailing gap ops become clips and a position."""
    pats, txts, cigars, status = corpus_strings(metric, ends_free=True)
    mapped = clipped = moved = 0
    for flags in FLAGS:
        for p, t, ops, st in zip(pats, txts, cigars, status):
            if st != 0:
                continue
            row, cigar, md = _native.ops_sam(ops, t.encode(), len(p), flags)
            assert (tuple(row), cigar, md) == py_sam(ops, t.encode(), flags)
            if row[0] < 0:
                assert (tuple(row), cigar, md) == UNMAPPED
                continue
            pos, ref_len, clip_left, clip_right, nm, cigar_len, md_len, query_len = (int(x) for x in row)
            assert ref_from(p, cigar.decode(), md.decode()) == t[pos:pos + ref_len], (metric, flags, ops)
            assert MD_FORM.fullmatch(md), md
            assert clip_left + query_len + clip_right == len(p) and pos + ref_len <= len(t)
            assert nm == sum(span_counts(ops, flags)) and (cigar_len, md_len) == (len(cigar), len(md))
            mapped += 1
            clipped += clip_left > 0 or clip_right > 0
            moved += pos > 0
    assert mapped >= 4 * 450 and clipped >= 20 and moved >= 20, (mapped, clipped, moved)


def test_ref_from_is_a_check():
    assert ref_from("ACTTCA", "4M1I1M", "2G1^AC2") is None                     # a deletion the CIGAR does not have
    assert ref_from("ACTTGCA", "4M2D1M1I1M", "2G1^AC2") == "ACGTACGA"
    assert ref_from("ACTTGCA", "4M2D1M1I1M", "2G1^AC3") is None and ref_from("ACTTGCA", "4M2D1M1I2M", "2G1^AC2") is None
    assert ref_from("TTACGTT", "2S3M2S", "1T1") == "ATG"


def test_refusals_of_the_host_rule():
    L = _native.lib()
    ops, text = np.frombuffer(b"MMXMIIMDM", np.uint8), np.frombuffer(b"ACGTACGT", np.uint8)
    row, cigar, md = np.full(8, -7, np.int32), np.full(32, 0x2e, np.uint8), np.full(32, 0x2e, np.uint8)

    def call(ops_=ops, n=9, text_=text, tlen=8, plen=7, flags=0, row_=row, cigar_=cigar, ccap=32, md_=md, mcap=32):
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        return L.wfa_hip_ops_sam(ptr(ops_), n, ptr(text_), tlen, plen, flags, ptr(row_), ptr(cigar_), ccap, ptr(md_), mcap)

    refused = [dict(ccap=9), dict(mcap=6), dict(ccap=0), dict(mcap=-1),                       # a buffer is too small
               dict(ops_=None), dict(text_=None), dict(row_=None), dict(cigar_=None), dict(md_=None),   # a pointer is missing
               dict(plen=6), dict(plen=8), dict(tlen=7), dict(n=8), dict(n=0),                # not exactly plen and tlen bases
               dict(ops_=np.frombuffer(b"MMXMIIMSM", np.uint8)), dict(flags=4), dict(flags=-1), dict(n=-1)]
    for kw in refused:
        assert call(**kw) == _native.EINVAL, kw
        assert (row == -7).all() and (cigar == 0x2e).all() and (md == 0x2e).all(), kw
    assert call(ccap=10, mcap=7) == _native.OK and cigar[:10].tobytes() == b"4M2D1M1I1M" and md[:7].tobytes() == b"2G1^AC2"
    assert (cigar[10:] == 0x2e).all() and (md[7:] == 0x2e).all()
    # a pair of two empty sequences is no alignment
    assert call(ops_=None, n=0, text_=None, tlen=0, plen=0, cigar_=None, ccap=0, md_=None, mcap=0) == _native.OK
    assert tuple(row) == UNMAPPED[0]
    with pytest.raises(ValueError, match="wfa_hip_ops_sam"):
        _native.ops_sam(b"MMM", b"ACGT", 3)
    with pytest.raises(ValueError, match="wfa_hip_ops_sam"):
        _native.ops_sam(b"MMM", b"ACG", 3, 8)


def test_abi_version_symbols_and_keywords():
    assert _native.lib().wfa_hip_abi_version() == _native.ABI_VERSION == 4
    for name in ("wfa_hip_batch_sam_counts", "wfa_hip_batch_sam_strings", "wfa_hip_batch_sam_kernel_ms", "wfa_hip_ops_sam"):
        assert name in _native.SYMBOLS and hasattr(_native.lib(), name), name
    assert (_native.SAM_COLS, _native.SAM_EQX, _native.SAM_CORE) == (8, EQX, CORE) and len(_native.SAM_COLUMNS) == 8
    for fn in (WavefrontAligner.align_windows, WavefrontAligner.align_pairs):
        par = inspect.signature(fn).parameters
        for name in ("sam", "eqx", "clip_mismatches"):
            assert par[name].default is False and par[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__name__, name)
