#!/usr/bin/env python3
"""The refusals of the resident-set entries of libwfa_hip.so (csrc/api_*.hip and wfa_hip_batch_summary), case by case.

``record()`` makes one aligner (and a second one, for foreign handles), two sets of three sequences of 14 - 40 bases, two finished
batches on three pairs (scope = full and scope = score), one of every resident handle, and walks a table of bad calls through
``_native.lib()``.  Every case gives ``{"entry", "case", "rc", "last_error", "global_error"}``: ``rc`` is the entry's code, or "null" /
"handle" for a creator; the two messages are ``wfa_hip_last_error(al)`` and ``wfa_hip_global_error()`` right after the call (a refusal
that sets neither leaves the ones before it: the walk is one fixed sequence, so they are part of the record).

Run as a script it writes the record as JSON (default tests/golden/api_refusals.json).  tests/test_api_refusals_gpu.py replays the
same walk against the current library and compares it with that file, which was recorded from the library BEFORE the entries were
rewritten on their shared helpers; record it again only from a library whose messages are the reference.

Branches that no call from outside reaches are listed in SKIPPED, each with the failed HIP call that guards it.
"""
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pywfa_amd import _native  # noqa: E402

READS = ["ACGTTGCATGCCATGA", "TTGACCATGGCATGCAACGTACGATCGATCGGATCCAT", "GATTACAGATTACA"]                     # 16, 38, 14 bases
REFS = ["ACGTTGCATGGCATGATTGACCATGGCATG", "TGTAATCTGTAATCGGATGGATCGATCGATCGTACGTTG", "CCATGGCAAGCAACGTAC"]   # 30, 39, 18 bases

SKIPPED = [
    ("every creator", "hipSetDevice failed", "guarded by a failed hipSetDevice"),
    ("every entry", "HIP_TRY messages (pool_alloc, copies, events, synchronisations)", "guarded by a failed HIP call"),
    ("wfa_hip_pileup_create", "pileup table: hipMalloc of N bytes failed", "guarded by a failed hipMalloc"),
    ("wfa_hip_placer_create / _add / _run*", "placement: the allocation of N bytes failed", "guarded by a failed pool allocation"),
    ("wfa_hip_placer_create", "placement: hipEventCreate failed", "guarded by a failed hipEventCreate"),
    ("wfa_hip_seed_index_create*", "seed index table / records: hipMalloc of N bytes failed", "guarded by a failed hipMalloc"),
    ("wfa_hip_seed_index_chain", "seed chain workspace: hipMalloc of N bytes failed", "guarded by a failed hipMalloc"),
    ("every entry that launches", "... kernel launch failed", "guarded by a failed kernel launch"),
    ("wfa_hip_seqset_create / wfa_hip_cross_run* / wfa_hip_batch_create_*", "more than 2^31 / 2^32 packed words",
     "needs gigabytes of sequence: out of a quick test's reach, and behind it only a message"),
]


def _blob(seqs):
    length = np.array([len(s) for s in seqs], np.int32)
    off = np.zeros(len(seqs), np.int64)
    off[1:] = np.cumsum(length[:-1])
    return np.frombuffer("".join(seqs).encode() + b"\0", np.uint8).copy(), off, length


def i32(*v):
    return np.array(v, np.int32)


def record():
    """The walk: a list of case records, then every handle and both aligners destroyed."""
    L = _native.lib()
    p = _native._ptr
    out = []

    cfg = _native.default_config()
    cfg.scope = _native.SCOPE["full"]
    al = L.wfa_hip_create(ctypes.byref(cfg), 0)
    other = L.wfa_hip_create(ctypes.byref(cfg), 0)
    assert al and other, L.wfa_hip_global_error().decode()

    def case(entry, name, fn, creator=None):
        """One bad call; a creator's handle, should it come back, is destroyed through ``creator``."""
        r = fn()
        if creator is not None:
            if r:
                getattr(L, creator)(r)
            r = "handle" if r else "null"
        out.append(dict(entry=entry, case=name, rc=r if isinstance(r, str) else int(r),
                        last_error=L.wfa_hip_last_error(al).decode(), global_error=L.wfa_hip_global_error().decode()))

    def seqset(a, seqs):
        blob, off, length = _blob(seqs)
        h = L.wfa_hip_seqset_create(a, len(seqs), p(blob), p(off), p(length))
        assert h, L.wfa_hip_global_error().decode()
        return h

    def set_cfg(**kw):
        c = cfg.copy()
        for k, v in kw.items():
            setattr(c, k, v)
        rc = L.wfa_hip_set_config(al, ctypes.byref(c))
        assert rc == _native.OK, L.wfa_hip_last_error(al).decode()

    reads, refs, one, foreign = seqset(al, READS), seqset(al, REFS), seqset(al, REFS[:1]), seqset(other, REFS)
    empty = L.wfa_hip_seqset_create(al, 0, None, None, None)
    assert empty
    ij = i32(0, 1, 2)

    def indexed(a, P, T):
        h = L.wfa_hip_batch_create_indexed(a, P, T, 3, p(ij), p(ij))
        assert h, L.wfa_hip_global_error().decode()
        return h

    def run(b):
        assert L.wfa_hip_batch_run(b, None) == _native.OK and L.wfa_hip_batch_sync(b) == _native.OK, L.wfa_hip_last_error(al).decode()

    set_cfg(scope=_native.SCOPE["score"])
    b_score = indexed(al, reads, refs)
    run(b_score)
    set_cfg()
    b_full, b_notrun, b_foreign = indexed(al, reads, refs), indexed(al, reads, refs), indexed(other, foreign, foreign)
    run(b_full)

    blob, off, length = _blob(READS)
    SC, SD = "wfa_hip_seqset_create", "wfa_hip_seqset_destroy"
    case(SC, "null aligner", lambda: L.wfa_hip_seqset_create(None, 3, p(blob), p(off), p(length)), SD)
    case(SC, "n < 0", lambda: L.wfa_hip_seqset_create(al, -1, p(blob), p(off), p(length)), SD)
    case(SC, "missing lengths", lambda: L.wfa_hip_seqset_create(al, 3, p(blob), p(off), None), SD)
    neg = length.copy()
    neg[1] = -1
    case(SC, "a negative length", lambda: L.wfa_hip_seqset_create(al, 3, p(blob), p(off), p(neg)), SD)
    noff = off.copy()
    noff[2] = -5
    case(SC, "a negative offset", lambda: L.wfa_hip_seqset_create(al, 3, p(blob), p(noff), p(length)), SD)

    D, K = _native.CROSS_DENSE, _native.CROSS_TOPK
    CR, CK, CD = "wfa_hip_cross_run", "wfa_hip_cross_run_k", "wfa_hip_cross_destroy"
    case(CR, "null aligner", lambda: L.wfa_hip_cross_run(None, reads, refs, D), CD)
    case(CR, "top-k through cross_run", lambda: L.wfa_hip_cross_run(al, reads, refs, D | K), CD)
    case(CR, "null patterns", lambda: L.wfa_hip_cross_run(al, None, refs, D), CD)
    case(CR, "texts of another aligner", lambda: L.wfa_hip_cross_run(al, reads, foreign, D), CD)
    case(CR, "patterns of another aligner", lambda: L.wfa_hip_cross_run(al, foreign, None, D), CD)
    case(CR, "want = 0", lambda: L.wfa_hip_cross_run(al, reads, refs, 0), CD)
    case(CR, "want = 8", lambda: L.wfa_hip_cross_run(al, reads, refs, 8), CD)
    case(CK, "null aligner", lambda: L.wfa_hip_cross_run_k(None, reads, refs, K, 2), CD)
    case(CK, "k = 0", lambda: L.wfa_hip_cross_run_k(al, reads, refs, K, 0), CD)
    case(CK, "k = 65", lambda: L.wfa_hip_cross_run_k(al, reads, refs, D | K, 65), CD)
    BI, BW, BD = "wfa_hip_batch_create_indexed", "wfa_hip_batch_create_windows", "wfa_hip_batch_destroy"
    set_cfg(wildcard=ord("N"))
    case(CR, "sets packed under another wildcard", lambda: L.wfa_hip_cross_run(al, reads, refs, D), CD)
    case(BI, "sets packed under another wildcard", lambda: L.wfa_hip_batch_create_indexed(al, reads, refs, 3, p(ij), p(ij)), BD)
    set_cfg(span=_native.SPAN["ends-free"], pattern_begin_free=15, text_end_free=19)
    case(CR, "free ends longer than a sequence", lambda: L.wfa_hip_cross_run(al, reads, refs, D), CD)
    case(BI, "free ends longer than a sequence", lambda: L.wfa_hip_batch_create_indexed(al, reads, refs, 3, p(ij), p(ij)), BD)
    set_cfg()

    x_dense = L.wfa_hip_cross_run(al, reads, refs, D)
    x_topk = L.wfa_hip_cross_run_k(al, reads, refs, K, 2)
    assert x_dense and x_topk, L.wfa_hip_last_error(al).decode()
    buf, cnt = np.zeros(16, np.int32), ctypes.c_int64(0)
    case("wfa_hip_cross_topk", "null run", lambda: L.wfa_hip_cross_topk(None, p(buf), p(buf)))
    case("wfa_hip_cross_topk", "a run without top-k", lambda: L.wfa_hip_cross_topk(x_dense, p(buf), p(buf)))
    case("wfa_hip_cross_topk", "null outputs", lambda: L.wfa_hip_cross_topk(x_topk, None, p(buf)))
    case("wfa_hip_cross_dense", "null run", lambda: L.wfa_hip_cross_dense(None, p(buf), p(buf)))
    case("wfa_hip_cross_dense", "a run without the matrix", lambda: L.wfa_hip_cross_dense(x_topk, p(buf), p(buf)))
    case("wfa_hip_cross_dense", "null outputs", lambda: L.wfa_hip_cross_dense(x_dense, p(buf), None))
    case("wfa_hip_cross_completed", "null run", lambda: L.wfa_hip_cross_completed(None, ctypes.byref(cnt), None, None, None))
    case("wfa_hip_cross_completed", "null count", lambda: L.wfa_hip_cross_completed(x_dense, None, None, None, None))
    case("wfa_hip_cross_completed", "a run without completed pairs", lambda: L.wfa_hip_cross_completed(x_dense, ctypes.byref(cnt), None, None, None))
    case("wfa_hip_cross_kernel_ms", "null run", lambda: L.wfa_hip_cross_kernel_ms(None, None, None))
    case("wfa_hip_plan_cross_bands", "m < 0", lambda: L.wfa_hip_plan_cross_bands(-1, 3, 0, 4, None, 0))
    case("wfa_hip_plan_cross_bands", "max_pairs = 0", lambda: L.wfa_hip_plan_cross_bands(3, 3, 1, 0, None, 0))
    case("wfa_hip_window_2bit", "a negative start", lambda: L.wfa_hip_window_2bit(p(buf), -1, 4, 0, p(buf)))
    case("wfa_hip_window_2bit", "null words", lambda: L.wfa_hip_window_2bit(None, 0, 4, 0, p(buf)))

    case(BI, "null aligner", lambda: L.wfa_hip_batch_create_indexed(None, reads, refs, 3, p(ij), p(ij)), BD)
    case(BI, "null patterns", lambda: L.wfa_hip_batch_create_indexed(al, None, refs, 3, p(ij), p(ij)), BD)
    case(BI, "texts of another aligner", lambda: L.wfa_hip_batch_create_indexed(al, reads, foreign, 3, p(ij), p(ij)), BD)
    case(BI, "npairs < 0", lambda: L.wfa_hip_batch_create_indexed(al, reads, refs, -1, p(ij), p(ij)), BD)
    case(BI, "missing j", lambda: L.wfa_hip_batch_create_indexed(al, reads, refs, 3, p(ij), None), BD)
    i_out, j_neg = i32(0, 3, 1), i32(0, 1, -1)
    case(BI, "i out of range", lambda: L.wfa_hip_batch_create_indexed(al, reads, refs, 3, p(i_out), p(ij)), BD)
    case(BI, "j negative, one set", lambda: L.wfa_hip_batch_create_indexed(al, reads, None, 3, p(ij), p(j_neg)), BD)

    def windows(i=ij, j=ij, ps=None, pl=None, ts=None, tl=None, P=reads, T=refs, a=al, n=3):
        return L.wfa_hip_batch_create_windows(a, P, T, n, p(i), p(j), p(ps), p(pl), p(ts), p(tl), None)

    case(BW, "null aligner", lambda: windows(a=None), BD)
    case(BW, "patterns of another aligner", lambda: windows(P=foreign), BD)
    case(BW, "missing i", lambda: windows(i=None), BD)
    case(BW, "i out of range", lambda: windows(i=i_out), BD)
    w_neg, w_len, w_past = i32(0, -2, 0), i32(4, -1, 4), i32(0, 30, 0)
    case(BW, "a negative pattern start", lambda: windows(ps=w_neg), BD)
    case(BW, "a negative text length", lambda: windows(tl=w_len), BD)
    case(BW, "a text window past the end", lambda: windows(ts=w_past, tl=i32(10, 10, 10)), BD)
    case(BW, "a pattern start past the end", lambda: windows(ps=i32(0, 39, 0)), BD)

    summ = np.zeros(30, np.int32)
    SU = "wfa_hip_batch_summary"
    case(SU, "null batch", lambda: L.wfa_hip_batch_summary(None, p(summ)))
    case(SU, "scope = score", lambda: L.wfa_hip_batch_summary(b_score, p(summ)))
    case(SU, "a batch that has not run", lambda: L.wfa_hip_batch_summary(b_notrun, p(summ)))
    case(SU, "null output", lambda: L.wfa_hip_batch_summary(b_full, None))

    PC, PD = "wfa_hip_pileup_create", "wfa_hip_pileup_destroy"
    case(PC, "null aligner", lambda: L.wfa_hip_pileup_create(None, refs), PD)
    case(PC, "null texts", lambda: L.wfa_hip_pileup_create(al, None), PD)
    case(PC, "texts of another aligner", lambda: L.wfa_hip_pileup_create(al, foreign), PD)
    pile = L.wfa_hip_pileup_create(al, refs)
    assert pile, L.wfa_hip_last_error(al).decode()
    PA = "wfa_hip_pileup_add"
    case(PA, "null pileup", lambda: L.wfa_hip_pileup_add(None, b_full, p(ij), None, None))
    case(PA, "null batch", lambda: L.wfa_hip_pileup_add(pile, None, p(ij), None, None))
    case(PA, "batch of another aligner", lambda: L.wfa_hip_pileup_add(pile, b_foreign, p(ij), None, None))
    case(PA, "scope = score", lambda: L.wfa_hip_pileup_add(pile, b_score, p(ij), None, None))
    case(PA, "a batch that has not run", lambda: L.wfa_hip_pileup_add(pile, b_notrun, p(ij), None, None))
    case(PA, "missing j", lambda: L.wfa_hip_pileup_add(pile, b_full, None, None, None))
    case(PA, "j out of range", lambda: L.wfa_hip_pileup_add(pile, b_full, p(i_out), None, None))
    case(PA, "j negative", lambda: L.wfa_hip_pileup_add(pile, b_full, p(j_neg), None, None))
    case(PA, "a negative t_start", lambda: L.wfa_hip_pileup_add(pile, b_full, p(ij), p(w_neg), None))
    case(PA, "a text window past the end", lambda: L.wfa_hip_pileup_add(pile, b_full, p(ij), p(i32(0, 1, 0)), None))
    PR = "wfa_hip_pileup_read"
    rows = np.zeros(64 * 8, np.int32)
    case(PR, "null pileup", lambda: L.wfa_hip_pileup_read(None, 0, 0, 4, p(rows)))
    for name, a in (("seq = -1", (-1, 0, 4)), ("seq = 3", (3, 0, 4)), ("start < 0", (0, -1, 4)), ("len < 0", (0, 0, -1)),
                    ("rows past the end", (2, 10, 9))):
        case(PR, name, lambda a=a: L.wfa_hip_pileup_read(pile, *a, p(rows)))
    case(PR, "null output", lambda: L.wfa_hip_pileup_read(pile, 0, 0, 4, None))
    PCs, PS = "wfa_hip_pileup_calls", "wfa_hip_pileup_sites"
    calls = np.zeros(64, np.uint8)
    case(PCs, "null pileup", lambda: L.wfa_hip_pileup_calls(None, refs, 0, 0, 4, 1, p(calls)))
    case(PCs, "null texts", lambda: L.wfa_hip_pileup_calls(pile, None, 0, 0, 4, 1, p(calls)))
    case(PCs, "texts of another aligner", lambda: L.wfa_hip_pileup_calls(pile, foreign, 0, 0, 4, 1, p(calls)))
    case(PCs, "a set of another size", lambda: L.wfa_hip_pileup_calls(pile, one, 0, 0, 4, 1, p(calls)))
    case(PCs, "a set of other lengths", lambda: L.wfa_hip_pileup_calls(pile, reads, 0, 0, 4, 1, p(calls)))
    case(PCs, "min_depth = 0", lambda: L.wfa_hip_pileup_calls(pile, refs, 0, 0, 4, 0, p(calls)))
    case(PCs, "seq = -1", lambda: L.wfa_hip_pileup_calls(pile, refs, -1, 0, -1, 1, p(calls)))
    case(PCs, "rows past the end", lambda: L.wfa_hip_pileup_calls(pile, refs, 1, 30, 10, 1, p(calls)))
    case(PCs, "null output", lambda: L.wfa_hip_pileup_calls(pile, refs, 0, 0, 4, 1, None))

    def sites(P=pile, T=refs, seq=-1, start=0, length=-1, depth=1, permille=500, cap=4, count=ctypes.byref(cnt), r=rows):
        return L.wfa_hip_pileup_sites(P, T, seq, start, length, depth, permille, cap, count, p(r))

    case(PS, "null pileup", lambda: sites(P=None))
    case(PS, "texts of another aligner", lambda: sites(T=foreign))
    case(PS, "a set of another size", lambda: sites(T=one))
    case(PS, "min_depth = -3", lambda: sites(depth=-3))
    case(PS, "min_permille = 0", lambda: sites(permille=0))
    case(PS, "min_permille = 1001", lambda: sites(permille=1001))
    case(PS, "cap = -1", lambda: sites(cap=-1))
    case(PS, "seq = -1 with a start", lambda: sites(start=2))
    case(PS, "seq = -1 with a length", lambda: sites(length=5))
    case(PS, "seq = 3", lambda: sites(seq=3, length=1))
    case(PS, "rows past the end", lambda: sites(seq=2, start=9, length=10))
    case(PS, "null count", lambda: sites(count=None))
    case(PS, "null rows with cap > 0", lambda: sites(r=None))
    case("wfa_hip_pileup_clear", "null pileup", lambda: L.wfa_hip_pileup_clear(None))

    LC, LD = "wfa_hip_placer_create", "wfa_hip_placer_destroy"
    case(LC, "null aligner", lambda: L.wfa_hip_placer_create(None, 3), LD)
    case(LC, "nreads = -1", lambda: L.wfa_hip_placer_create(al, -1), LD)
    case(LC, "nreads = 2^31 - 1", lambda: L.wfa_hip_placer_create(al, 2**31 - 1), LD)
    placer, placer5 = L.wfa_hip_placer_create(al, 3), L.wfa_hip_placer_create(al, 5)
    assert placer and placer5, L.wfa_hip_last_error(al).decode()
    LA = "wfa_hip_placer_add"
    case(LA, "null placer", lambda: L.wfa_hip_placer_add(None, b_full, p(ij), p(ij), None, None))
    case(LA, "null batch", lambda: L.wfa_hip_placer_add(placer, None, p(ij), p(ij), None, None))
    case(LA, "batch of another aligner", lambda: L.wfa_hip_placer_add(placer, b_foreign, p(ij), p(ij), None, None))
    case(LA, "a batch that has not run", lambda: L.wfa_hip_placer_add(placer, b_notrun, p(ij), p(ij), None, None))
    case(LA, "missing i", lambda: L.wfa_hip_placer_add(placer, b_full, None, p(ij), None, None))
    case(LA, "i out of range", lambda: L.wfa_hip_placer_add(placer, b_full, p(i_out), p(ij), None, None))
    case(LA, "j negative", lambda: L.wfa_hip_placer_add(placer, b_score, p(ij), p(j_neg), None, None))
    case(LA, "a negative t_start", lambda: L.wfa_hip_placer_add(placer, b_full, p(ij), p(ij), p(w_neg), None))
    LH = "wfa_hip_placer_add_hits"
    sc, st, ts, te = i32(-4, -8, 0), i32(0, 0, 0), i32(0, 5, 2), i32(16, 30, 16)

    def hits(P=placer, n=3, i=ij, j=ij, score=sc, status=st, start=ts, end=te):
        return L.wfa_hip_placer_add_hits(P, n, p(i), p(j), None, p(score), p(status), p(start), p(end))

    case(LH, "null placer", lambda: hits(P=None))
    case(LH, "missing status", lambda: hits(status=None))
    case(LH, "missing j", lambda: hits(j=None))
    case(LH, "n < 0", lambda: hits(n=-1))
    case(LH, "i out of range", lambda: hits(i=i_out))
    case(LH, "text_end below text_start", lambda: hits(end=i32(16, 4, 16)))
    LR, LP, LS = "wfa_hip_placer_run", "wfa_hip_placer_run_pairs", "wfa_hip_placer_rescue"
    prow, pflag, pairs = np.zeros(5 * 8, np.int32), np.zeros(8, np.uint8), np.zeros(4 * 12, np.int32)
    case(LR, "null placer", lambda: L.wfa_hip_placer_run(None, -100, 24, p(prow), p(pflag)))
    case(LR, "full_gap = 0", lambda: L.wfa_hip_placer_run(placer, -100, 0, p(prow), p(pflag)))
    case(LR, "null rows", lambda: L.wfa_hip_placer_run(placer, -100, 24, None, p(pflag)))
    m1, m2, m_out = i32(0), i32(1), i32(3)

    def run_pairs(P=placer, gap=24, lo=0, hi=1000, unpaired=0, nfrag=1, a=m1, b=m2, pr=pairs):
        return L.wfa_hip_placer_run_pairs(P, -100, gap, lo, hi, unpaired, nfrag, p(a), p(b), p(prow), p(pflag), p(pr), None)

    case(LP, "null placer", lambda: run_pairs(P=None))
    case(LP, "full_gap = -1", lambda: run_pairs(gap=-1))
    case(LP, "min_insert above max_insert", lambda: run_pairs(lo=10, hi=5))
    case(LP, "min_insert negative", lambda: run_pairs(lo=-1))
    case(LP, "unpaired = -1", lambda: run_pairs(unpaired=-1))
    case(LP, "nfrag = -1", lambda: run_pairs(nfrag=-1))
    case(LP, "interleaved fragments beyond the reads", lambda: run_pairs(nfrag=2, a=None, b=None))
    case(LP, "one mate array", lambda: run_pairs(b=None))
    case(LP, "a mate outside the reads", lambda: run_pairs(b=m_out))
    case(LP, "a read as its own mate", lambda: run_pairs(b=m1))
    case(LP, "null pair_rows", lambda: run_pairs(pr=None))

    def rescue(P=placer, S=reads, T=refs, gap=24, lo=0, nfrag=1, pad=16, min_len=0, mapq=0, cap=2, count=ctypes.byref(cnt), r=prow):
        return L.wfa_hip_placer_rescue(P, S, T, -100, gap, lo, 1000, 0, nfrag, p(m1), p(m2), pad, min_len, mapq, cap, count, p(r))

    case(LS, "null placer", lambda: rescue(P=None))
    case(LS, "full_gap = 0", lambda: rescue(gap=0))
    case(LS, "min_insert negative", lambda: rescue(lo=-2))
    case(LS, "pad = -1", lambda: rescue(pad=-1))
    case(LS, "min_len = -1", lambda: rescue(min_len=-1))
    case(LS, "anchor_mapq = 61", lambda: rescue(mapq=61))
    case(LS, "cap = -1", lambda: rescue(cap=-1))
    case(LS, "null count", lambda: rescue(count=None))
    case(LS, "null rows with cap > 0", lambda: rescue(r=None))
    case(LS, "a missing sequence set", lambda: rescue(T=None))
    case(LS, "texts of another aligner", lambda: rescue(T=foreign))
    case(LS, "a pattern set smaller than the placer", lambda: rescue(P=placer5))
    assert hits() == _native.OK, L.wfa_hip_last_error(al).decode()   # (three hits, on texts 0, 1 and 2)
    case(LS, "a hit on a text the set does not hold", lambda: rescue(T=one))
    case("wfa_hip_placer_kernel_ms", "null output", lambda: L.wfa_hip_placer_kernel_ms(placer, None))
    case("wfa_hip_placer_clear", "null placer", lambda: L.wfa_hip_placer_clear(None))

    XC, XM, XD = "wfa_hip_seed_index_create", "wfa_hip_seed_index_create_minimizer", "wfa_hip_seed_index_destroy"
    case(XC, "null aligner", lambda: L.wfa_hip_seed_index_create(None, refs, 8, 1, 64), XD)
    case(XC, "null texts", lambda: L.wfa_hip_seed_index_create(al, None, 8, 1, 64), XD)
    case(XC, "texts of another aligner", lambda: L.wfa_hip_seed_index_create(al, foreign, 8, 1, 64), XD)
    for name, a in (("k = 3", (3, 1, 64)), ("k = 16", (16, 1, 64)), ("stride = 0", (8, 0, 64)), ("max_occ = 0", (8, 1, 0))):
        case(XC, name, lambda a=a: L.wfa_hip_seed_index_create(al, refs, *a), XD)
    case(XC, "an empty set", lambda: L.wfa_hip_seed_index_create(al, empty, 8, 1, 64), XD)
    case(XM, "null aligner", lambda: L.wfa_hip_seed_index_create_minimizer(None, refs, 8, 4, 64), XD)
    for name, a in (("k = 3", (3, 4, 64)), ("w = 0", (8, 0, 64)), ("w = 33", (8, 33, 64)), ("max_occ = -1", (8, 4, -1))):
        case(XM, name, lambda a=a: L.wfa_hip_seed_index_create_minimizer(al, refs, *a), XD)
    case(XM, "an empty set", lambda: L.wfa_hip_seed_index_create_minimizer(al, empty, 8, 4, 64), XD)
    index = L.wfa_hip_seed_index_create(al, refs, 8, 1, 64)
    assert index, L.wfa_hip_last_error(al).decode()
    cols = [np.zeros(3 * 16, np.int32) for _ in range(8)]
    over = np.zeros(3, np.uint8)
    XQ, XH = "wfa_hip_seed_index_query", "wfa_hip_seed_index_chain"

    def query(X=index, P=reads, n=4, min_hits=2, gap=16, pad=16, max_hits=2048, c=cols, o=over):
        return L.wfa_hip_seed_index_query(X, P, n, min_hits, gap, pad, max_hits, *[p(a) for a in c[:5]], p(o))

    case(XQ, "null index", lambda: query(X=None))
    case(XQ, "null patterns", lambda: query(P=None))
    case(XQ, "patterns of another aligner", lambda: query(P=foreign))
    for name, kw in (("n = 0", dict(n=0)), ("n = 17", dict(n=17)), ("min_hits = 0", dict(min_hits=0)), ("gap = -1", dict(gap=-1)),
                     ("pad = -1", dict(pad=-1)), ("max_hits = 0", dict(max_hits=0)), ("max_hits = 4097", dict(max_hits=4097))):
        case(XQ, name, lambda kw=kw: query(**kw))
    case(XQ, "a missing result array", lambda: query(c=cols[:3] + [None] + cols[4:]))
    case(XQ, "missing overflow", lambda: query(o=None))

    def chain(X=index, P=reads, n=4, min_hits=3, min_score=40, lookback=32, max_dist=5000, band=500, pad=64, max_anchors=1024, c=cols, o=over):
        return L.wfa_hip_seed_index_chain(X, P, n, min_hits, min_score, lookback, max_dist, band, pad, max_anchors, *[p(a) for a in c], p(o))

    case(XH, "null index", lambda: chain(X=None))
    case(XH, "null patterns", lambda: chain(P=None))
    case(XH, "patterns of another aligner", lambda: chain(P=foreign))
    for name, kw in (("n = 0", dict(n=0)), ("n = 17", dict(n=17)), ("min_hits = 0", dict(min_hits=0)), ("min_score = -1", dict(min_score=-1)),
                     ("lookback = 0", dict(lookback=0)), ("lookback = 65", dict(lookback=65)), ("max_dist = -1", dict(max_dist=-1)),
                     ("band = -1", dict(band=-1)), ("pad = -1", dict(pad=-1)), ("max_anchors = 0", dict(max_anchors=0)),
                     ("max_anchors = 65537", dict(max_anchors=65537))):
        case(XH, name, lambda kw=kw: chain(**kw))
    case(XH, "a missing result array", lambda: chain(c=cols[:6] + [None] + cols[7:]))
    case("wfa_hip_seed_index_params", "null index", lambda: L.wfa_hip_seed_index_params(None, None, None, None))
    case("wfa_hip_seed_index_stats", "null index", lambda: L.wfa_hip_seed_index_stats(None, None, None, None, None, None))
    case("wfa_hip_seed_index_chain_stats", "null index", lambda: L.wfa_hip_seed_index_chain_stats(None, None, None))

    # every handle goes, then the aligners under no live handle: a refused create that had kept its count would leave `al` marked, not freed
    L.wfa_hip_seed_index_destroy(index)
    L.wfa_hip_placer_destroy(placer)
    L.wfa_hip_placer_destroy(placer5)
    L.wfa_hip_pileup_destroy(pile)
    L.wfa_hip_cross_destroy(x_dense)
    L.wfa_hip_cross_destroy(x_topk)
    for b in (b_score, b_full, b_notrun, b_foreign):
        L.wfa_hip_batch_destroy(b)
    for s in (reads, refs, one, empty, foreign):
        L.wfa_hip_seqset_destroy(s)
    L.wfa_hip_destroy(al)
    L.wfa_hip_destroy(other)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "api_refusals.json")
    cases = record()
    with open(path, "w") as f:
        json.dump(dict(cases=cases, skipped=[dict(entry=e, branch=b, reason=r) for e, b, r in SKIPPED]), f, indent=1)
        f.write("\n")
    print(f"{len(cases)} cases -> {path}")


if __name__ == "__main__":
    main()
