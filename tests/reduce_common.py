"""Shared by the tests of the two op-string reductions (per-pair summary, pileup): their rules restated in plain Python, straight
from include/wfa_hip.h, and the expected tables built from the ORACLE's op strings."""
import itertools

import numpy as np

from pywfa_amd.align import _flank_scan, _ops_to_tuples

LETTER_COL = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}


def py_summary(ops, plen, tlen):
    """Row of the per-pair summary: counts of M, X, I, D; maximal I and D runs; the four locations as the reference's class derives
    them (`_flank_scan` on the run-length encoding, threshold 1; zeros for an empty pair or an empty op string)."""
    ops = bytes(ops)
    out = [ops.count(b"M"), ops.count(b"X"), ops.count(b"I"), ops.count(b"D"),
           sum(1 for c, _ in itertools.groupby(ops) if c == ord("I")), sum(1 for c, _ in itertools.groupby(ops) if c == ord("D"))]
    locs = [0, 0, 0, 0]
    ct = _ops_to_tuples(np.frombuffer(ops, np.uint8))
    if ct and plen and tlen:
        locs = list(_flank_scan(ct, 1, 1, tlen, plen)[2:])
    return np.array(out + locs, np.int32)


def core_of(ops):
    """(first M, last M) of an op string, or None."""
    ops = bytes(ops)
    f = ops.find(b"M")
    return None if f < 0 else (f, ops.rfind(b"M"))


def py_pileup(ops, pattern, rows):
    """One pair's contribution added to its window-relative rows (tlen x 8)."""
    ops, pattern = bytes(ops), bytes(pattern)
    core = core_of(ops)
    if core is None:
        return rows
    v = h = 0
    for k, c in enumerate(ops[:core[1] + 1]):
        inside = k >= core[0]
        if c in b"MX":
            if inside:
                rows[h, LETTER_COL.get(pattern[v], 4)] += 1
                if c == ord("X"):
                    rows[h, 7] += 1
            v += 1
            h += 1
        elif c == ord("I"):
            if inside:
                rows[h, 5] += 1
            h += 1
        elif c == ord("D"):
            if inside and ops[k - 1] != ord("D"):
                rows[h, 6] += 1
            v += 1
    return rows


def expected_tables(ref_lens, o, pats, j, t_start, t_len, keep=None):
    """The pileup of a list from the oracle's results `o` of its materialised pairs: a table per reference; and per reference the
    number of contributing pairs whose aligned core covers each base."""
    tables = [np.zeros((n, 8), np.int32) for n in ref_lens]
    cover = [np.zeros(n, np.int32) for n in ref_lens]
    for q, ops in enumerate(o["cigars"]):
        if o["status"][q] != 0 or (keep is not None and not keep[q]):
            continue
        ts, tl = int(t_start[q]), int(t_len[q])
        py_pileup(ops, pats[q].encode(), tables[j[q]][ts:ts + tl])
        core = core_of(ops)
        if core is not None:
            h0 = sum(1 for c in ops[:core[0]] if c in b"MXI")
            h1 = sum(1 for c in ops[:core[1] + 1] if c in b"MXI")
            cover[j[q]][ts + h0:ts + h1] += 1
    return tables, cover
