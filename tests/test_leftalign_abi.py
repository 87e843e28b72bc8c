"""Left alignment on the host (wfa_hip_ops_left_align, pywfa_amd.left_align_ops; no GPU): the four examples of the header, hand-written
strings for every way a run stops, the repeat corpus against the Python restatement of the rule (leftalign_common) applied to the
ORACLE's op strings, the invariants the header states, and the refusals."""
import ctypes

import numpy as np
import pytest

import pywfa_amd
from common import rle
from leftalign_common import corpus_oracle, expand, py_left_align, repeat_corpus
from oracle import loader
from pywfa_amd import _native
from reduce_common import core_of

FLANK_L, FLANK_R = "TGCATCGATTCGAGCTAGCTTGACCGTATCGGATCCGTAG", "CTGGATCCTAGGCTTAGCGATCGTAGGCTAACGTTAGCGT"   # 40 + 40, no A beside the repeat


def both(ops, pattern, text):
    """The host function and the Python rule on one pair: they agree; (rewritten ops as a run-length string, runs moved, merges)."""
    ops = ops if isinstance(ops, bytes) else expand(ops)
    got, moved, merges = _native.ops_left_align(ops, pattern.encode(), text.encode())
    assert (got.tobytes(), moved, merges) == py_left_align(ops, pattern.encode(), text.encode()), (ops, pattern, text)
    return rle(got.tobytes()), moved, merges


@pytest.mark.parametrize("text_mid,read_mid,wfa,want", [
    ("G" + "A" * 8 + "C", "G" + "A" * 9 + "C", "49M1D41M", "41M1D49M"),       # one extra A in the read
    ("G" + "A" * 8 + "C", "G" + "A" * 7 + "C", "48M1I41M", "41M1I48M"),       # one missing A
    ("CA" * 5 + "G", "CA" * 6 + "G", "50M2D41M", "40M2D51M"),                  # an extra CA in (CA)5
    ("CA" * 5 + "G", "CA" * 4 + "G", "48M2I41M", "40M2I49M"),                  # a missing CA in (CA)5
])
def test_the_four_examples(text_mid, read_mid, wfa, want):
    text, read = FLANK_L + text_mid + FLANK_R, FLANK_L + read_mid + FLANK_R
    # the string to rewrite is the ORACLE's: gap-affine 4/6/2, end to end
    o = loader.run(loader.oracle(), loader.make_config(span="end-to-end"), pywfa_amd.datagen.from_strings([read], [text], upper=True))
    assert o["status"][0] == 0 and rle(o["cigars"][0]) == wfa
    assert both(o["cigars"][0], read, text) == (want, 1, 0)
    assert pywfa_amd.left_align_ops(o["cigars"][0].decode(), read, text) == expand(want).decode()
    assert pywfa_amd.left_align_ops(o["cigars"][0], read.encode(), text.encode()) == expand(want)
    out = pywfa_amd.left_align_ops(np.frombuffer(o["cigars"][0], np.uint8), read, text)
    assert isinstance(out, np.ndarray) and out.tobytes() == expand(want)


def test_hand_written_strings():
    # a run stopped by an X inside the repeat: the read has a T in the middle of the As and one A more
    assert both("4M1X4M1D3M", "GAAATAAAAACGT", "GAAAAAAAACGT") == ("4M1X1D7M", 1, 0)
    # a run that would reach the core's first M stays one op behind it
    assert both("5M1D2M", "AAAAAACG", "AAAAACG") == ("1M1D6M", 1, 0)
    assert both("5M1I2M", "AAAAACG", "AAAAAACG") == ("1M1I6M", 1, 0)
    assert both("1X4M1D2M", "CAAAAACG", "GAAAACG") == ("1X1M1D5M", 1, 0)
    # leading and trailing runs outside the core stay where they are
    assert both("2D4M1I", "AAAAAA", "AAAAA") == ("2D4M1I", 0, 0)
    assert both("1I3M1D", "AAAA", "AAAA") == ("1I3M1D", 0, 0)
    # an I run stopped by a D run
    assert both("2M2D1I3M", "GCTTAAG", "GCAAAG") == ("2M2D1I3M", 0, 0)
    assert both("2M2D3M1I2M", "GCTTAAAAG", "GCAAAAAG") == ("2M2D1I5M", 1, 0)
    # a merge: ...MIMMI... over a homopolymer becomes one run at its left end
    assert both("2M1I2M1I3M", "GAAAACT", "GAAAAAACT") == ("1M2I6M", 2, 1)
    assert both("2M1D2M1D3M", "GAAAAAACT", "GAAAACT") == ("1M2D6M", 2, 1)
    # a string without M, and strings of length 1
    assert both("2X1I", "AC", "GTA") == ("2X1I", 0, 0)
    assert both("1M", "A", "A") == ("1M", 0, 0)
    assert both("1D", "A", "") == ("1D", 0, 0)
    assert both("1I", "", "A") == ("1I", 0, 0)
    assert both("", "", "") == ("", 0, 0)


@pytest.mark.parametrize("metric", ["affine", "levenshtein", "indel"])
def test_the_repeat_corpus(metric):
    kw, batch, o, want = corpus_oracle(metric)
    pats, txts = repeat_corpus()
    assert len(pats) == 500 and (o["status"] == 0).all()
    changed = merged = 0
    out, merging = [], np.zeros(len(pats), bool)
    for q, (ops, p, t) in enumerate(zip(o["cigars"], pats, txts)):
        got, moved, merges = _native.ops_left_align(ops, p.encode(), t.encode())
        got = got.tobytes()
        assert (got, moved, merges) == want[q], (metric, q, rle(ops))                              # the host function is the Python rule
        assert len(got) == len(ops) and all(got.count(c) == ops.count(c) for c in b"MXID") and core_of(got) == core_of(ops), (metric, q)
        assert _native.ops_left_align(got, p.encode(), t.encode())[0].tobytes() == got, (metric, q)   # a second application changes nothing
        assert (moved > 0) == (got != ops) and (merges == 0 or moved >= 1), (metric, q)
        changed += got != ops
        merged += merges > 0
        merging[q] = merges > 0
        out.append(got)
    print(f"{metric}: {changed} of {len(pats)} strings change, {merged} with a merge")
    assert changed > len(pats) // 2
    if metric == "affine":
        assert merged == 0            # under exact gap-affine a merge would have been the cheaper alignment
    if metric == "levenshtein":
        assert merged >= 1            # the merge branch is exercised
    # every rewritten string is a valid transcript of its pair; the score is checked where no merge changed it.  The checker prices a
    # transcript by gap-affine penalties, so the one-component metrics are given as such: levenshtein = (x 1, o 0, e 1) and indel, which
    # has no X, likewise; their scores are compared by magnitude
    ops = np.frombuffer(b"".join(out), np.uint8)
    clen = np.array([len(x) for x in out], np.int32)
    cbeg = np.concatenate(([0], np.cumsum(clen)[:-1])).astype(np.int64)
    priced = loader.make_config(**kw) if metric == "affine" else loader.make_config(span="end-to-end", mismatch=1, gap_opening=0, gap_extension=1)
    score = o["score"] if metric == "affine" else -np.abs(o["score"])
    assert loader.check_cigars(priced, batch, score, ops, cbeg, clen, check_score=False) == (0, -1)
    keep = np.flatnonzero(~merging)
    sub = {k: np.asarray(batch[k])[keep] for k in ("p_off", "p_len", "t_off", "t_len")}
    sub["seqs"] = batch["seqs"]
    assert loader.check_cigars(priced, sub, score[keep], ops, cbeg[keep], clen[keep], check_score=True) == (0, -1)
    # ... and a merge can only improve it
    for q in np.flatnonzero(merging):
        runs = lambda s: sum(1 for k in range(len(s)) if s[k] in b"ID" and (k == 0 or s[k - 1] != s[k]))   # noqa: E731
        assert runs(out[q]) < runs(o["cigars"][q])


def test_refusals_leave_the_buffer_unchanged():
    L = _native.lib()
    ops0, P, T = expand("5M1D2M"), b"AAAAAACG", b"AAAAACG"
    stats = np.full(2, -5, np.int64)

    def call(ops, n, p, pl, t, tl, null_ops=False):
        buf = np.frombuffer(ops, np.uint8).copy()
        rc = L.wfa_hip_ops_left_align(None if null_ops else buf.ctypes.data, len(buf) if n is None else n, p, pl, t, tl, stats.ctypes.data)
        assert rc == _native.EINVAL and buf.tobytes() == ops and (stats == -5).all(), (ops, n, pl, tl)

    call(ops0, -1, P, 8, T, 7)                 # negative lengths
    call(ops0, None, P, -1, T, 7)
    call(ops0, None, P, 8, T, -1)
    call(ops0, None, P, 8, T, 7, null_ops=True)   # missing pointers
    call(ops0, None, None, 8, T, 7)
    call(ops0, None, P, 8, None, 7)
    call(ops0, None, P, 9, T, 7)               # an op string that does not consume exactly plen and tlen
    call(ops0, None, P, 7, T, 7)
    call(ops0, None, P, 8, T, 8)
    call(ops0, None, P, 8, T, 6)
    call(ops0, 7, P, 8, T, 7)
    # stats is optional
    buf = np.frombuffer(ops0, np.uint8).copy()
    assert L.wfa_hip_ops_left_align(buf.ctypes.data, len(buf), P, 8, T, 7, None) == _native.OK and rle(buf.tobytes()) == "1M1D6M"
    with pytest.raises(ValueError, match="does not consume exactly"):
        pywfa_amd.left_align_ops("5M", "AAAAAA", "AAAAA")
    assert ctypes.sizeof(ctypes.c_int64) == stats.itemsize
