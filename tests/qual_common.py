"""Shared by the tests of base qualities in the pileup: the rule restated in plain Python and NumPy, straight from the text of
include/wfa_hip.h ("base qualities") and not from the C++; seeded quality arrays for the corpus of calls_common; a list of small
pairs chosen for where the table kernel can go wrong; and the expectations of both lists, built from the ORACLE's op strings."""
import functools

import numpy as np

from calls_common import KW, REF_COL, expectation
from genotype_common import wrap32
from oracle import loader
from pywfa_amd import datagen
from reduce_common import LETTER_COL, core_of
from test_windows_gpu import materialise, revcomp

MAX_Q = 93
# (min_base_quality, quality_cap): 0, 13 and 94 - 1; 1, 40 and 93
PARAMS = [(0, 40), (13, 40), (93, 93), (13, 1)]
# the values at which one of the comparisons Q < min_base_quality, Q < quality_cap changes under one of PARAMS
EDGES = np.array([0, 1, 2, 12, 13, 14, 39, 40, 41, 92, 93], np.uint8)
# (min_depth, min_permille, err_q, min_alt_strand) of the genotypes
GENO_PARAMS = [(1, 500, 20, 0), (8, 200, 20, 0), (8, 200, 20, 2), (1, 1, 1, 0), (4, 1000, 60, 1)]
COLS = 16


# ---- the rule ---------------------------------------------------------------------------------------------------------------------

def py_pileup_quals(ops, pattern, quals, mbq, cap, rows, qrows):
    """One pair's contribution added to its window-relative rows and qrows (tlen x 8 each); quals[v] is the quality of pattern[v]."""
    ops, pattern = bytes(ops), bytes(pattern)
    n = len(pattern)
    assert len(quals) == n
    core = core_of(ops)
    if core is None:
        return
    qc = lambda x: min(int(quals[x]), cap)
    v = h = 0
    for k, c in enumerate(ops[:core[1] + 1]):
        inside = k >= core[0]
        if c in b"MX":
            if inside and int(quals[v]) >= mbq:
                col = LETTER_COL.get(pattern[v], 4)
                rows[h, col] += 1
                qrows[h, col] += qc(v)
                if c == ord("X"):
                    rows[h, 7] += 1
                    qrows[h, 7] += qc(v)
            v += 1
            h += 1
        elif c == ord("I"):
            if inside:
                flank = [qc(x) for x in (v - 1, v) if 0 <= x < n]
                rows[h, 5] += 1
                qrows[h, 5] += min(flank) if flank else 0
            h += 1
        elif c == ord("D"):
            if inside and ops[k - 1] != ord("D"):
                rows[h, 6] += 1
                qrows[h, 6] += qc(v)
            v += 1


def window_quals(quals, W, q):
    """Q(v) for v = 0 .. n - 1 of pair q of the list W over the reads' quality arrays."""
    r = int(W["i"][q])
    s = int(W["p_start"][q]) if W.get("p_start") is not None else 0
    n = int(W["p_len"][q]) if W.get("p_len") is not None else len(quals[r]) - s
    w = quals[r][s:s + n]
    return w[::-1] if W.get("reverse") is not None and W["reverse"][q] else w


def tables_q(ref_lens, o, pats, W, quals, mbq, cap, keep=None):
    """(counts, qsums, forward counts) per reference of the list W from the op strings of `o`."""
    out = [[np.zeros((n, 8), np.int32) for n in ref_lens] for _ in range(3)]
    for q, ops in enumerate(o["cigars"]):
        if o["status"][q] != 0 or (keep is not None and not keep[q]):
            continue
        j, ts, tl = int(W["j"][q]), int(W["t_start"][q]), int(W["t_len"][q])
        rows, qrows = np.zeros((tl, 8), np.int32), np.zeros((tl, 8), np.int32)
        py_pileup_quals(ops, pats[q].encode(), window_quals(quals, W, q), mbq, cap, rows, qrows)
        out[0][j][ts:ts + tl] += rows
        out[1][j][ts:ts + tl] += qrows
        if not W["reverse"][q]:
            out[2][j][ts:ts + tl] += rows
    for tables in out:
        for t in tables:
            t.setflags(write=False)
    return tuple(out)


def py_costs(L):
    gt = min(range(3), key=lambda k: (L[k], k))
    low = sorted(L)
    return gt, min(99, low[1] - low[0])


def py_genotypes_quals(counts, qsums, fwd, ref, seq, start, min_depth, min_permille, err_q, min_alt_strand):
    """The rows (int32, n x 16) of the quality-weighted genotypes over the rows of counts, qsums and fwd (None: no strands)."""
    assert fwd is not None or min_alt_strand == 0
    rows = []
    for g in range(len(counts)):
        c = [int(x) for x in counts[g]]
        qs = [int(x) for x in qsums[g]]
        depth = sum(c[:6])
        if depth < min_depth:
            continue
        r = REF_COL.get(ref[g], 4)
        alt = max((x for x in range(6) if x != r), key=lambda x: (c[x], -x))
        a = c[alt]
        snv = a >= 1 and 1000 * a >= min_permille * depth
        ins = c[6] >= 1 and 1000 * c[6] >= min_permille * depth
        f = None if fwd is None else [int(x) for x in fwd[g]]
        if min_alt_strand > 0:
            snv = snv and f[alt] >= min_alt_strand and a - f[alt] >= min_alt_strand
            ins = ins and f[6] >= min_alt_strand and c[6] - f[6] >= min_alt_strand
        if not (snv or ins):
            continue
        gt = py_costs([qs[alt], 3 * (c[r] + a), qs[r]]) if snv else (-1, -1)
        R = max(0, depth - c[6])
        igt = py_costs([qs[6], 3 * (R + c[6]), err_q * R]) if ins else (-1, -1)
        strands = [-1] * 4 if f is None else [wrap32(sum(f[:6])), f[r], f[alt] if snv else 0, f[6]]
        rows.append([seq, start + g, r, alt if snv else -1, wrap32(depth), c[r], a if snv else 0, c[6], *gt, *igt, *strands])
    return np.array(rows, np.int64).reshape(-1, COLS).astype(np.int32)


def py_genotypes_quals_all(counts, qsums, fwds, refs, params):
    return np.concatenate([py_genotypes_quals(t, qsums[j], None if fwds is None else fwds[j], refs[j].encode(), j, 0, *params)
                           for j, t in enumerate(counts)])


# ---- qualities --------------------------------------------------------------------------------------------------------------------

def seeded_quals(lengths, seed):
    """A quality array per read: values drawn from 0 .. 93, every fourth position exactly at one of EDGES."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        q = rng.integers(0, MAX_Q + 1, n).astype(np.uint8)
        q[::4] = EDGES[rng.integers(0, len(EDGES), len(q[::4]))]
        q.setflags(write=False)
        out.append(q)
    return out


def fastq(q, offset=33):
    return (q.astype(np.int32) + offset).astype(np.uint8).tobytes().decode("ascii")


# ---- the two lists ----------------------------------------------------------------------------------------------------------------

class Case:
    """A list with everything the tests need: refs, reads, W, quals, the oracle's results, the materialised patterns."""

    def __init__(self, refs, reads, W, o, pats, seed, kw=KW):
        self.refs, self.reads, self.W, self.o, self.pats, self.kw = refs, reads, W, o, pats, kw
        self.quals = seeded_quals([len(r) for r in reads], seed)
        self.lens = [len(r) for r in refs]

    @functools.lru_cache(maxsize=None)
    def tables(self, mbq, cap):
        return tables_q(self.lens, self.o, self.pats, self.W, self.quals, mbq, cap)


@functools.lru_cache(maxsize=None)
def corpus_case():
    e = expectation()
    pats, _ = materialise(e["reads"], e["refs"], e["W"])
    return Case(e["refs"], e["reads"], e["W"], e["o"], pats, 11)


LETTERS = np.array(list("ACGT"))
EDGE_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
EDGE_KW = dict(span="end-to-end")


def _differs(*letters):
    return next(x for x in "ACGT" if x not in letters)


@functools.lru_cache(maxsize=None)
def edge_case():
    """Small pairs over one reference of 1200 bases: reads of 1 .. 200 bases that match it (op strings that end on, just before and
    just behind a 64-op round), an insertion run of 3 at ops 62 .. 64 (across a round boundary), a deletion at op 64, a read with an
    N (the byte path); each stored forward and reverse-complemented, each as the whole read (pattern_start 0) and as a window that
    starts 7 bases in and stops 5 short of the read's end.  The text window is the locus itself and the alignment end-to-end
    (EDGE_KW), so that an op's index in its string is what this list says."""
    rng = np.random.default_rng(23)
    ref = "".join(LETTERS[rng.integers(0, 4, 1200)])
    cores = []   # (read on the text's strand, first text base, text bases)
    for k, n in enumerate(EDGE_LENGTHS):
        p = 40 + 100 * k
        cores.append((ref[p:p + n], p, n))
    p = 1000
    ins = _differs(ref[p + 61], ref[p + 62]) * 3
    cores.append((ref[p:p + 62] + ins + ref[p + 62:p + 122], p, 122))                    # 62 M, 3 D, 60 M
    p = next(x for x in range(860, 980) if ref[x + 64] != ref[x + 65] and ref[x + 63] != ref[x + 64])   # (the deleted base cannot slide)
    cores.append((ref[p:p + 64] + ref[p + 65:p + 125], p, 125))                           # 64 M, 1 I, 60 M
    p = 300
    cores.append((ref[p:p + 30] + "N" + ref[p + 31:p + 90], p, 90))
    reads, rows = [], []
    for core, p, n in cores:
        for rev in (0, 1):
            stored = revcomp(core) if rev else core
            for windowed in (0, 1):
                read = "GATTACA" + stored + "CCATG" if windowed else stored
                t0, t1 = p, p + n
                rows.append((len(reads), 0, 7 if windowed else 0, len(stored), t0, t1 - t0, rev))
                reads.append(read)
    cols = list(zip(*rows))
    W = dict(i=np.array(cols[0], np.int32), j=np.array(cols[1], np.int32), p_start=np.array(cols[2], np.int32),
             p_len=np.array(cols[3], np.int32), t_start=np.array(cols[4], np.int32), t_len=np.array(cols[5], np.int32),
             reverse=np.array(cols[6], np.uint8))
    refs = [ref]
    pats, txts = materialise(reads, refs, W)
    o = loader.run(loader.oracle(), loader.make_config(**EDGE_KW), datagen.from_strings(pats, txts, upper=True))
    return Case(refs, reads, W, o, pats, 29, EDGE_KW)


def edge_ops(case, core_index):
    """The op strings of the four pairs of core `core_index` of the edge list."""
    return [bytes(case.o["cigars"][4 * core_index + k]) for k in range(4)]
