"""Mate rescue, the part that needs no GPU: the C entries are declared, exported and bound; the host statement wfa_hip_rescue_host
equals the Python restatement of the rule (rescue_common.py_rescue) on random cases in which every clause occurs and on hand-written
edges; its refusals, with the outputs untouched.  (tools/rescue_host_check.cpp is the stand-alone program for the sanitizers.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from pair_common import INT32_MAX, INT32_MIN, as_hit_arrays
from pywfa_amd import _native
from rescue_common import CLAUSES, RESCUE_COLUMNS, py_rescue, random_rescue_case
from test_pair_abi import H

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRIES = ("wfa_hip_placer_rescue", "wfa_hip_rescue_host")
PAR = dict(min_score=INT32_MIN, full_gap=24, min_insert=150, max_insert=600, unpaired=0)
HIT_KEYS = ("i", "j", "reverse", "score", "status", "text_start", "text_end")


def host(hits, nreads, mates, par, read_len, text_len, pad, min_len, anchor_mapq, cap=None):
    a = as_hit_arrays(hits)
    return _native.rescue_host(nreads, *[a[k] for k in HIT_KEYS], mates, read_len, text_len, pad=pad, min_len=min_len,
                               anchor_mapq=anchor_mapq, cap=cap, **par)


def test_header_binding_and_shim_declare_the_entries():
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    pxd = open(os.path.join(ROOT, "pywfa_amd", "cython_shim", "wfa_hip.pxd")).read()
    L = _native.lib()
    for name in ENTRIES:
        assert name + "(" in txt and name in _native.SYMBOLS and hasattr(L, name) and name + "(" in pxd, name
    assert "#define WFA_HIP_RESCUE_COLS 8 " in txt
    assert raw.index("---- pairing:") < raw.index("---- rescue:") < raw.index("---- seed finder:")
    assert "RESCUED FRAGMENT" in raw and "WHAT RESCUE DOES NOT DO" in raw and "lo = ts_a + min_insert - len(o) - pad" in raw
    assert _native.RESCUE_COLUMNS == RESCUE_COLUMNS and _native.RESCUE_COLS == 8
    assert hasattr(_native.Placer, "rescue") and L.wfa_hip_abi_version() == _native.ABI_VERSION
    build = open(os.path.join(ROOT, "pywfa_amd", "csrc", "build.sh")).read()
    assert "host_rescue.cpp" in build and os.path.exists(os.path.join(ROOT, "pywfa_amd", "csrc", "k_rescue.hip"))


def test_host_statement_equals_the_restatement_on_random_cases():
    rng = np.random.default_rng(2026)
    seen = {}
    for k in range(2000):
        nreads, hits, mates, par, read_len, text_len, pad, min_len, anchor_mapq = random_rescue_case(rng)
        want = py_rescue(hits, nreads, mates, par, read_len, text_len, pad, min_len, anchor_mapq, seen)
        count, rows = host(hits, nreads, mates, par, read_len, text_len, pad, min_len, anchor_mapq)
        assert count == len(want) and rows.dtype == np.int32 and rows.shape == want.shape, (k, count, len(want))
        assert np.array_equal(rows, want), (k, mates, par, pad, min_len, anchor_mapq, rows.tolist(), want.tolist())
    # the generator itself: every clause of the rule decided somewhere
    assert set(seen) == set(CLAUSES) and all(seen[c] >= 5 for c in CLAUSES), sorted(seen.items())
    assert seen["made"] >= 100, sorted(seen.items())


F0, R1 = (0, 0, 0), (1, 0, 1)      # (i, j, reverse): a forward hit of read 0, a reverse hit of read 1, text 0


def test_edges_by_hand():
    lens, tl = [150, 100], [5000]
    # mate 1 anchored forward at [1000, 1150), mate 2 without a hit: one window, for read 1, reverse strand
    one = H(F0 + (-4, 0, 1000, 1150))
    for what in ("python", "host"):
        def run(hits, nreads=2, mates=1, par=PAR, read_len=lens, text_len=tl, pad=16, min_len=0, anchor_mapq=0, **kw):
            if what == "python":
                return py_rescue(hits, nreads, mates, par, read_len, text_len, pad, min_len, anchor_mapq).tolist()
            return host(hits, nreads, mates, par, read_len, text_len, pad, min_len, anchor_mapq, **kw)[1].tolist()
        assert run(one) == [[1, 0, 1000 + 150 - 100 - 16, 600 - 150 + 100 + 32, 1, 0, 0, 0]], what
        # the anchor on the reverse strand: [te - max - pad, te - min + len(o) + pad), forward strand
        assert run(H((0, 0, 1, -4, 0, 1000, 1150))) == [[1, 0, 1150 - 600 - 16, 600 - 150 + 100 + 32, 0, 0, 0, 0]], what
        # mate 2 the anchor: the window is for read 0 (150 bases)
        assert run(H(R1 + (-4, 0, 1000, 1150))) == [[0, 0, 1150 - 600 - 16, 600 - 150 + 150 + 32, 0, 0, 0, 0]], what
        # both mates placed on different texts: two windows, mate 1's first; clipped at 0 and at the end of text 1 (300 bases)
        two = H(F0 + (-4, 0, 100, 250), (1, 1, 1, -4, 0, 100, 250))
        assert run(two, text_len=[5000, 300]) == [[1, 0, 134, 582, 1, 0, 0, 0], [0, 1, 0, 266, 0, 0, 1, 0]], what
        # min_len: the clipped window of 266 bases is dropped at 267, kept at 266
        assert len(run(two, text_len=[5000, 300], min_len=266)) == 2 and len(run(two, text_len=[5000, 300], min_len=267)) == 1, what
        # a text shorter than lo: nothing; an empty window is dropped even with min_len = 0
        assert run(one, text_len=[1034]) == [] and run(one, text_len=[1035]) == [[1, 0, 1034, 1, 1, 0, 0, 0]], what
        # a proper pairing: not rescued; a fragment that has one but lost to its single-end primaries (unpaired = 0): not rescued
        assert run(H(F0 + (-4, 0, 1000, 1150), R1 + (-4, 0, 1300, 1450))) == [], what
        lost = H(F0 + (0, 0, 1000, 1150), F0 + (-30, 0, 3000, 3150), R1 + (-4, 0, 3300, 3450), (1, 0, 1, 0, 0, 4800, 4950))
        assert run(lost) == [], what
        # an empty interval is no anchor; anchor_mapq: a tie (mapq 0) is refused at 1, taken at 0
        assert run(H(F0 + (-4, 0, 1000, 1000))) == [], what
        tie = H(F0 + (-4, 0, 1000, 1150), F0 + (-4, 0, 3000, 3150))
        assert run(tie, anchor_mapq=1) == [] and [r[6] for r in run(tie)] == [0], what
        assert [r[2] for r in run(one, anchor_mapq=60)] == [1034], what
        # 64-bit arithmetic: ts next to 2^31 - 1 with max_insert = 2^31 - 1 (a 32-bit sum would wrap below 0 and clip to an empty window)
        big = dict(PAR, min_insert=0, max_insert=INT32_MAX)
        far = H(F0 + (-4, 0, INT32_MAX - 200, INT32_MAX - 50))
        assert run(far, par=big, text_len=[INT32_MAX]) == [[1, 0, INT32_MAX - 200 - 100 - 16, 316, 1, 0, 0, 0]], what
        assert run(H((0, 0, 1, -4, 0, 10, 160)), par=big, text_len=[INT32_MAX], pad=INT32_MAX) == [[1, 0, 0, INT32_MAX, 0, 0, 0, 0]], what
        # no fragment; no hit at all
        assert run(one, mates=0) == [] and run(H()) == [], what
        # mates as an array, backwards: fragment 0 = reads (3, 2), the anchor is its mate 2
        assert run(H((2, 0, 0, -4, 0, 1000, 1150)), nreads=4, mates=[[3, 2], [1, 0]], read_len=[1, 2, 3, 40]) == [[3, 0, 1000 + 150 - 40 - 16, 522, 1, 0, 0, 0]], what
    # cap below the count: the count is full, only cap rows are written
    a = as_hit_arrays(two)
    count, rows = host(two, 2, 1, PAR, lens, [5000, 300], 16, 0, 0, cap=1)
    assert count == 2 and rows.tolist() == [[1, 0, 134, 582, 1, 0, 0, 0]]
    buf = np.full((3, 8), 7, np.int32)
    n = ctypes.c_int64(-1)
    rl, tlen = np.array(lens, np.int32), np.array([5000, 300], np.int32)
    ptrs = [None if a[k] is None else a[k].ctypes.data for k in HIT_KEYS]
    rc = _native.lib().wfa_hip_rescue_host(2, 2, *ptrs, INT32_MIN, 24, 150, 600, 0, 1, None, None, rl.ctypes.data, 2, tlen.ctypes.data, 16, 0, 0, 1,
                                           ctypes.byref(n), buf.ctypes.data, None, 0)
    assert rc == _native.OK and n.value == 2 and buf[0].tolist() == [1, 0, 134, 582, 1, 0, 0, 0] and (buf[1:] == 7).all()
    rc = _native.lib().wfa_hip_rescue_host(2, 2, *ptrs, INT32_MIN, 24, 150, 600, 0, 1, None, None, rl.ctypes.data, 2, tlen.ctypes.data, 16, 0, 0, 0,
                                           ctypes.byref(n), None, None, 0)
    assert rc == _native.OK and n.value == 2                                     # the counting call
    assert host(two, 2, 1, PAR, lens, [5000, 300], 16, 0, 0, cap=0)[0] == 2


def test_refusals():
    ok = H(F0 + (-4, 0, 1000, 1150), (2, 1, 0, -4, 0, 5, 100))
    lens, tl = [150, 100, 50, 50], [5000, 300]

    def call(hits=ok, mates=2, read_len=lens, text_len=tl, pad=16, min_len=0, anchor_mapq=0, cap=None, **change):
        return host(hits, 4, mates, dict(PAR, **change), read_len, text_len, pad, min_len, anchor_mapq, cap)

    assert call()[0] == 2
    for kw, msg in ((dict(pad=-1), r"pad = -1, min_len = 0 are out of range"), (dict(min_len=-5), r"pad = 16, min_len = -5 are out of range"),
                    (dict(anchor_mapq=-1), r"anchor_mapq = -1 is out of range \(0 \.\. 60\)"), (dict(anchor_mapq=61), r"anchor_mapq = 61 is out of range"),
                    (dict(cap=-1), r"cap = -1 is out of range"),
                    (dict(read_len=[150, 100, -1, 50]), r"negative length of read 2: read_len = -1"),
                    (dict(text_len=[5000, -3]), r"negative length of text 1: text_len = -3"),
                    (dict(text_len=[5000]), r"text index out of range at position 1 of the hit list: j = 1 over 1 texts"),
                    (dict(text_len=[]), r"text index out of range at position 0 of the hit list: j = 0 over 0 texts"),
                    # whatever wfa_hip_pair_host refuses
                    (dict(hits=H((4, 0, 0, -4, 0, 1, 2))), r"read index out of range at position 0 of the hit list: i = 4 over 4 reads"),
                    (dict(hits=H((0, 0, 0, -4, 0, 100, 99))), r"text_end below text_start at position 0"),
                    (dict(full_gap=0), r"full_gap = 0 is out of range"), (dict(min_insert=-1), r"min_insert = -1, max_insert = 600 are out of range"),
                    (dict(min_insert=700), r"min_insert = 700, max_insert = 600 are out of range"), (dict(unpaired=-1), r"unpaired = -1 is out of range"),
                    (dict(mates=-1), r"a negative number of fragments"), (dict(mates=3), r"3 interleaved fragments need 6 reads, there are 4"),
                    (dict(mates=[[0, 1], [2, 4]]), r"mate out of range at fragment 1"), (dict(mates=[[0, 0]]), r"the mates of fragment 0 are one read"),
                    (dict(mates=[[0, 1], [1, 2]]), r"read 1 is named by two fragments")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match="one value per read"):
        call(read_len=[1, 2, 3])
    # straight at the C entry: missing pointers and the refusals above; nothing is written
    L = _native.lib()
    a = as_hit_arrays(ok)
    ptrs = [a[k].ctypes.data for k in HIT_KEYS]
    rl, tlen = np.array(lens, np.int32), np.array(tl, np.int32)
    rows = np.full((4, 8), 7, np.int32)
    count = ctypes.c_int64(-9)
    msg = ctypes.create_string_buffer(256)

    def raw(nfrag=2, read_len=rl.ctypes.data, ntexts=2, text_len=tlen.ctypes.data, pad=16, min_len=0, anchor_mapq=0, cap=4, count_p=ctypes.byref(count),
            rows_p=rows.ctypes.data, max_insert=600, mate1=None, mate2=None):
        return L.wfa_hip_rescue_host(4, 2, *ptrs, INT32_MIN, 24, 150, max_insert, 0, nfrag, mate1, mate2, read_len, ntexts, text_len, pad, min_len,
                                     anchor_mapq, cap, count_p, rows_p, msg, 256)

    m = np.array([0, 2], np.int32)
    assert raw(count_p=None) == _native.EINVAL and b"missing array (count)" in msg.value
    assert raw(rows_p=None) == _native.EINVAL and b"missing array (rows)" in msg.value
    assert raw(read_len=None) == _native.EINVAL and b"missing array (read_len)" in msg.value
    assert raw(text_len=None) == _native.EINVAL and b"missing array (text_len)" in msg.value
    assert raw(ntexts=-1) == _native.EINVAL and b"a negative number of texts" in msg.value
    assert raw(mate1=m.ctypes.data) == _native.EINVAL and b"mate2 is missing" in msg.value
    for kw in (dict(pad=-1), dict(min_len=-1), dict(anchor_mapq=61), dict(cap=-1), dict(ntexts=1), dict(nfrag=3), dict(nfrag=-1), dict(max_insert=100)):
        assert raw(**kw) == _native.EINVAL and msg.value, kw
    assert (rows == 7).all() and count.value == -9
    assert raw() == _native.OK and msg.value == b"" and count.value == 2
    assert rows[:2].tolist() == [[1, 0, 1034, 582, 1, 0, 0, 0], [3, 1, 5 + 150 - 50 - 16, 300 - 89, 1, 1, 1, 0]] and (rows[2:] == 7).all()
    # no reads, no texts, no fragments
    assert L.wfa_hip_rescue_host(0, 0, *([None] * 7), 0, 1, 0, 0, 0, 0, None, None, None, 0, None, 0, 0, 0, 0, ctypes.byref(count), None, None, 0) == _native.OK
    assert count.value == 0


def test_reference_rescues_every_dropped_mate_of_the_corpus():
    """No GPU: what test_rescue_gpu.py relies on, from the oracle on the materialised windows and the restatements alone.  Without the
    window at mate 2's true place the fragment has no proper pairing; the rule's window, aligned with F free text bases at either end,
    brings every one of them back proper at mate 2's true place."""
    from oracle import loader
    from pair_common import py_pair
    from place_common import hits_of
    from pywfa_amd import datagen
    from rescue_common import join_hits, rescue_corpus, window_list
    from test_windows_gpu import materialise
    refs, reads, W, truth, dropped = rescue_corpus()
    assert len(dropped) == 27 and len(W["i"]) == 420 - 27
    kw = dict(span="ends-free", scope="full")
    # (min_score -100: a 150-base read at 3 % stays far above it, the alignment of a read to its random window far below, so that a
    # dropped mate has no eligible hit and cannot pair by chance)
    par = dict(min_score=-100, full_gap=24, min_insert=150, max_insert=600, unpaired=24)
    free = 450 + 2 * 16

    def run(Wl, free_ends):
        pats, txts = materialise(reads, refs, Wl)
        o = loader.run(loader.oracle(), loader.make_config(**dict(kw, text_begin_free=free_ends, text_end_free=free_ends)), datagen.from_strings(pats, txts, upper=True))
        return hits_of(o, Wl, True)

    hits0 = run(W, 20)
    n0 = len(W["i"])
    before = py_pair(hits0, len(reads), len(truth), *par.values())[2]
    assert not before[dropped, 2].any() and not before[dropped, 9].any()
    read_len, text_len = [len(r) for r in reads], [len(r) for r in refs]
    found = py_rescue(hits0, len(reads), len(truth), par, read_len, text_len, 16, free, 0)
    assert set(dropped) <= set(found[:, 5].tolist()) and (found[:, 3] >= free).all()
    hits = join_hits(hits0, run(window_list(found, read_len), free))
    after = py_pair(hits, len(reads), len(truth), *par.values())[2]
    for f in dropped:
        r2, pos2 = truth[f][6]
        h2 = int(after[f, 1])
        assert after[f, 2] == 1 and h2 >= n0 and hits["j"][h2] == r2, (f, after[f].tolist())
        assert min(hits["text_end"][h2], pos2 + 150) - max(hits["text_start"][h2], pos2) >= 75, (f, int(hits["text_start"][h2]), pos2)
