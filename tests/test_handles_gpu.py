"""Lifetimes of the resident handles on the GPU: an aligner closed under open handles, every handle closed twice, a set of another
aligner refused, and the windows entry points fed with lists and with ``SequenceSet`` handles — equal results, the caller's sets left
open.  Two sets of three short sequences and four windows: no large shapes, no timing."""
import numpy as np
import pytest

from pywfa_amd import WavefrontAligner, datagen

pytestmark = pytest.mark.gpu

READS = ["ACGTTGCATGCCATGA", "TTGACCATGGCATGCAACGTACGATCGATCGGATCCAT", "GATTACAGATTACA"]                     # 16, 38, 14 bases
REFS = ["ACGTTGCATGGCATGATTGACCATGGCATG", "TGTAATCTGTAATCGGATGGATCGATCGATCGTACGTTG", "CCATGGCAAGCAACGTAC"]   # 30, 39, 18 bases
WINDOWS = dict(i=[0, 1, 2, 1], j=[0, 0, 1, 2], pattern_start=[0, 0, 2, 10], pattern_len=[16, 20, 12, 12], text_start=[0, 10, 0, 3],
               text_len=[20, 20, 16, 15], reverse=[0, 0, 1, 0])
MATES = np.array([[0, 1]])   # (read 2 is in no fragment)
KW = dict(span="ends-free", text_begin_free=4, text_end_free=4)


def same(a, b):
    """Results of two calls, equal value for value: dicts of arrays, dicts, sequences of op strings."""
    assert type(a) is type(b)
    if isinstance(a, dict):
        assert list(a) == list(b)
        for k in a:
            same(a[k], b[k])
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    else:
        assert [np.asarray(x).tolist() for x in a] == [np.asarray(x).tolist() for x in b]


def open_handles(wa):
    """One of each resident handle of the aligner (the native objects)."""
    na = wa._native
    reads, refs = wa.sequence_set(READS), wa.sequence_set(REFS)
    pile = wa.pileup(reads, refs, **WINDOWS)
    index = wa.seed_index(refs, k=8)   # (the smallest k the library takes)
    return dict(seqset=reads._set, texts=refs._set, pileup=pile._pileup, placer=na.placer(len(READS)), seed_index=index._index,
                cross=na.cross(reads._set, refs._set), batch=wa.resident_batch(datagen.from_strings(READS, REFS, upper=True)))


def test_the_aligner_is_closed_under_open_handles(gpu):
    wa = WavefrontAligner(**KW)
    handles = open_handles(wa)
    assert all(h._h for h in handles.values())
    wa.close()
    for name, h in handles.items():
        assert h._h is None, name
        h.close()
        h.close()


def test_every_handle_closes_twice(gpu):
    wa = WavefrontAligner(**KW)
    for name, h in open_handles(wa).items():
        h.close()
        assert h._h is None, name
        h.close()
    wa.close()
    wa.close()


def test_a_set_of_another_aligner_is_refused(gpu):
    wa, other = WavefrontAligner(**KW), WavefrontAligner(**KW)
    with other.sequence_set(REFS) as foreign:
        for call in (lambda: wa.pileup(READS, foreign, **WINDOWS), lambda: wa.score_matrix(READS, foreign), lambda: wa.seed_index(foreign, k=8)):
            with pytest.raises(ValueError, match="^sequence set of another aligner$"):
                call()
        assert foreign._set._h
    wa.close()
    other.close()


@pytest.mark.parametrize("entry,how", [("align_windows", {}), ("align_windows", dict(summary=True)), ("pileup", dict(min_score=-40)),
                                       ("place_windows", dict(full_gap=24)), ("place_pairs", dict(mates=MATES, rescue=False, full_gap=24))])
def test_lists_and_handles_give_the_same(gpu, entry, how):
    wa = WavefrontAligner(**KW)
    reads, refs = wa.sequence_set(READS), wa.sequence_set(REFS)
    got = [getattr(wa, entry)(p, t, **WINDOWS, **how) for p, t in ((READS, REFS), (reads, refs), (READS, refs))]
    assert reads._set._h and refs._set._h   # (the session closes the sets it uploaded, never a caller's)
    if entry == "pileup":
        counts = [got[0].counts(j) for j in range(len(REFS))]
        assert sum(int(c.sum()) for c in counts) > 0
        for p in got:
            with p:
                same(p.score, got[0].score)
                same(p.status, got[0].status)
                for j in range(len(REFS)):
                    same(p.counts(j), counts[j])
            assert p._pileup is None
    else:
        assert (got[0]["status"] == 0).all()
        for g in got[1:]:
            same(g, got[0])
    assert reads._set._h and refs._set._h
    wa.close()


def test_a_refused_window_leaves_the_callers_sets_open(gpu):
    wa = WavefrontAligner(**KW)
    reads, refs = wa.sequence_set(READS), wa.sequence_set(REFS)
    past = dict(WINDOWS, text_len=[20, 21, 16, 15])   # (window 1: 10 + 21 bases of a text of 30)
    for entry, how in (("align_windows", {}), ("pileup", {}), ("place_windows", {}), ("place_pairs", dict(mates=MATES))):
        with pytest.raises(ValueError, match=r"text_start\[1\] \+ text_len\[1\] = 10 \+ 21 runs past the end of text sequence 0 \(30 bases\)"):
            getattr(wa, entry)(reads, refs, **past, **how)
        assert reads._set._h and refs._set._h
    same(wa.align_windows(reads, refs, **WINDOWS), wa.align_windows(READS, REFS, **WINDOWS))
    wa.close()
