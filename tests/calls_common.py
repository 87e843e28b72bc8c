"""Shared by the tests of the calls and sites reductions of a pileup: the two rules restated in plain Python, straight from the text of
include/wfa_hip.h ("calls and sites"), and a corpus with planted variants whose expected pileup comes from the ORACLE's op strings."""
import functools

import numpy as np

from oracle import loader
from pywfa_amd import datagen
from reduce_common import expected_tables
from test_windows_gpu import LETTERS, as_list, materialise, mutate, revcomp

KW = dict(span="ends-free", text_begin_free=20, text_end_free=20)
REF_COL = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}


# ---- the rules --------------------------------------------------------------------------------------------------------------------

def py_calls(counts, ref, min_depth):
    """One call byte per row of `counts` (rows of 8 counters) over the reference bytes `ref`."""
    out = np.zeros(len(counts), np.uint8)
    for g in range(len(counts)):
        c = [int(x) for x in counts[g]]
        depth = sum(c[:6])
        if depth < min_depth:
            out[g] = 6
            continue
        r = REF_COL.get(ref[g], 4)
        top = max(c[:6])
        tied = [x for x in range(6) if c[x] == top]
        code = r if r in tied else tied[0]
        if 2 * c[6] > depth:
            code |= 8
        out[g] = code
    return out


def py_sites(counts, ref, seq, start, min_depth, min_permille):
    """The site rows (int32, n x 8) of the rows of `counts`, numbered j = seq, pos = start + row."""
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
        if snv or ins:
            rows.append([seq, start + g, r, alt if snv else -1, depth, c[r], a if snv else 0, c[6]])
    return np.array(rows, np.int64).reshape(-1, 8).astype(np.int32)


def py_sites_all(tables, refs, min_depth, min_permille):
    """Every sequence: the rows in ascending (j, pos)."""
    return np.concatenate([py_sites(t, refs[j].encode(), j, 0, min_depth, min_permille) for j, t in enumerate(tables)])


# ---- the corpus -------------------------------------------------------------------------------------------------------------------

N_RUNS = [(0, 7), (500, 501), (1200, 1216), (2000, 2100), (4000, 4011)]   # of reference 3
BARE = (1, 2000, 2400)                                                      # reference 1 keeps [2000, 2400) without a read


def _free_positions(rng, n, length, taken, want_gap=12):
    """`n` positions of [40, length - 40), at least `want_gap` from each other and from every (lo, hi) of `taken`."""
    out = []
    while len(out) < n:
        p = int(rng.integers(40, length - 40))
        if all(p + 4 + want_gap <= lo or p - want_gap >= hi for lo, hi in taken):
            out.append(p)
            taken.append((p, p + 4))
    return out


def corpus(seed=5, nreads=2400):
    """The shape of test_pileup_gpu.corpus(): four references of 3-6 kb, the last with N runs, ~20x of 100-200 base reads at 3 %, every
    second one stored reverse-complemented — but the reads are cut from a DONOR copy that carries planted events: homozygous SNVs,
    1-3 base deletions and insertions (placed where the gap cannot slide), heterozygous SNVs in every second pair of reads (also under
    the long N run), an SNV under a reference N.  Reference 1 keeps a stretch no read covers; the set ends with a sequence shorter than
    64 bases and an empty one.  Returns refs, reads, the window list and the planted events per kind."""
    rng = np.random.default_rng(seed)
    bases = [rng.integers(0, 4, n) for n in (3000, 4500, 6000, 4011)]
    refs = ["".join(LETTERS[b]) for b in bases]
    last = list(refs[3])
    for a, b in N_RUNS:
        last[a:b] = "N" * (b - a)
    refs[3] = "".join(last)
    planted = dict(snv=[], dele=[], ins=[], het=[], under_n=[])
    donors, maps, het_at = [], [], []
    for r, f in enumerate(bases):
        L = len(f)
        taken = [(a - 1, b + 1) for a, b in N_RUNS] if r == 3 else []
        if r == BARE[0]:
            taken.append((BARE[1] - 220, BARE[2] + 220))
        ins_before, deleted, sub, het = {}, set(), {}, {}
        for p in _free_positions(rng, 10, L, taken):
            sub[p] = int((f[p] + rng.integers(1, 4)) % 4)
            planted["snv"].append((r, p, sub[p]))
        for p in _free_positions(rng, 10, L, taken):
            het[p] = int((f[p] + rng.integers(1, 4)) % 4)
            planted["het"].append((r, p, het[p]))
        k = 0
        while k < 5:                                   # deletions of [p, p + n) that cannot slide either way
            p, n = int(rng.integers(40, L - 40)), int(rng.integers(1, 4))
            if f[p] == f[p + n] or f[p - 1] == f[p + n - 1] or not all(p + 4 + 12 <= lo or p - 12 >= hi for lo, hi in taken):
                continue
            deleted.update(range(p, p + n))
            taken.append((p, p + 4))
            planted["dele"].append((r, p, n))
            k += 1
        k = 0
        while k < 5:                                   # insertions in front of p that cannot slide either way
            p, n = int(rng.integers(40, L - 40)), int(rng.integers(1, 4))
            s = rng.integers(0, 4, n)
            if s[0] == f[p] or s[-1] == f[p - 1] or not all(p + 4 + 12 <= lo or p - 12 >= hi for lo, hi in taken):
                continue
            ins_before[p] = s
            taken.append((p, p + 4))
            planted["ins"].append((r, p, n))
            k += 1
        if r == 3:                                     # under the Ns: an SNV, and heterozygous ones along the long run
            sub[1207] = int((f[1207] + 1) % 4)
            planted["under_n"].append((r, 1207, sub[1207]))
            for p in range(2004, 2100, 8):
                het[p] = int((f[p] + 2) % 4)
                planted["under_n"].append((r, p, het[p]))
        donor, start_of, het_donor = [], np.zeros(L + 1, np.int64), {}
        for p in range(L):
            start_of[p] = len(donor)
            if p in ins_before:
                donor.extend(int(x) for x in ins_before[p])
            if p in deleted:
                continue
            if p in het:
                het_donor[len(donor)] = het[p]
            donor.append(sub.get(p, int(f[p])))
        start_of[L] = len(donor)
        donors.append(np.array(donor))
        maps.append(start_of)
        het_at.append(het_donor)
    reads, rows = [], []
    k = 0
    while k < nreads:
        r = int(rng.integers(0, 4))
        n = int(rng.integers(100, 201))
        pos = int(rng.integers(0, len(donors[r]) - n + 1))
        lo = int(np.searchsorted(maps[r], pos, side="right")) - 1          # the reference bases the cut spans
        hi = int(np.searchsorted(maps[r], pos + n, side="left"))
        if r == BARE[0] and lo < BARE[2] + 25 and hi > BARE[1] - 25:
            continue
        cut = donors[r][pos:pos + n].copy()
        if (k // 2) % 2 == 1:
            for d, alt in het_at[r].items():
                if pos <= d < pos + n:
                    cut[d - pos] = alt
        s = "".join(LETTERS[mutate(rng, cut, 0.03)])
        if k % 37 == 0:
            s = s[:50] + "N" + s[51:]
        rev = k % 2 == 1
        reads.append(revcomp(s) if rev else s)
        t0, t1 = max(0, lo - int(rng.integers(0, 21))), min(len(refs[r]), hi + int(rng.integers(0, 21)))
        rows.append((k, r, 0, len(s), t0, t1 - t0, int(rev)))
        k += 1
    refs = refs + ["".join(LETTERS[rng.integers(0, 4, 41)]), ""]
    return refs, reads, as_list(rows), planted


@functools.lru_cache(maxsize=None)
def expectation():
    """The corpus and, computed once, the oracle's results of its pairs and the pileup tables they give (reduce_common)."""
    refs, reads, W, planted = corpus()
    pats, txts = materialise(reads, refs, W)
    o = loader.run(loader.oracle(), loader.make_config(**KW), datagen.from_strings(pats, txts, upper=True))
    tables, cover = expected_tables([len(r) for r in refs], o, pats, W["j"], W["t_start"], W["t_len"])
    for t in tables:
        t.setflags(write=False)
    return dict(refs=refs, reads=reads, W=W, planted=planted, o=o, tables=tables, cover=cover)


@functools.lru_cache(maxsize=None)
def expected_sites(min_depth, min_permille):
    e = expectation()
    rows = py_sites_all(e["tables"], e["refs"], min_depth, min_permille)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def expected_calls(min_depth):
    e = expectation()
    out = [py_calls(t, r.encode(), min_depth) for t, r in zip(e["tables"], e["refs"])]
    for a in out:
        a.setflags(write=False)
    return out
