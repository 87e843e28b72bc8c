"""Shared by the tests of the deletion log of a pileup: the rule restated in plain Python, straight from the text of include/wfa_hip.h
("deletions"), and a corpus whose reads carry planted deletions of known start and length.  Expected records, planes and rows come from
the ORACLE's op strings, never from the device."""
import collections
import functools

import numpy as np

from oracle import loader
from pywfa_amd import datagen
from reduce_common import LETTER_COL, core_of, expected_tables
from test_windows_gpu import LETTERS, as_list, materialise, mutate, revcomp

KW = dict(span="ends-free", text_begin_free=20, text_end_free=20)
MAX_READS = 4096


# ---- the rule ---------------------------------------------------------------------------------------------------------------------

def py_ops_deletions(ops):
    """The records of one pair: (h, n) per maximal I run of the aligned core, h the window-relative row of its first deleted base."""
    ops = bytes(ops)
    core = core_of(ops)
    out = []
    if core is None:
        return out
    h = k = 0
    while k <= core[1]:
        c = ops[k]
        if c == ord("I"):
            e = k
            while ops[e] == ord("I"):
                e += 1
            if k > core[0]:
                out.append((h, e - k))
            h += e - k
            k = e
        else:
            h += c in b"MX"
            k += 1
    return out


def py_deletions(counts, starts, lens_at, seq, start, min_depth, min_permille, max_reads=MAX_READS):
    """The rows (int32, n x 8) of the rows of `counts` / `starts`; `lens_at`: row -> list of the lengths of the records that start there."""
    rows = []
    for g in range(len(counts)):
        depth = sum(int(x) for x in counts[g][:6])
        S = int(starts[g])
        if depth < min_depth:
            continue
        if min_permille > 0:
            if not (S >= 1 and 1000 * S >= min_permille * depth):
                continue
        elif not 2 * S > depth:
            continue
        if S > max_reads:
            rows.append([seq, start + g, depth, S, 0, 0, 0, 1])
            continue
        alleles = collections.Counter(lens_at.get(g, []))
        n, count = min(alleles.items(), key=lambda kv: (-kv[1], kv[0])) if alleles else (0, 0)
        rows.append([seq, start + g, depth, S, count, n, len(alleles), 0])
    return np.array(rows, np.int64).reshape(-1, 8).astype(np.int32)


# ---- the corpus -------------------------------------------------------------------------------------------------------------------

STAGE = 3            # the reference only hand-made, unmutated reads cover: every record at its sites is known by construction
N_RUN = (2, 1200, 1216)
# (h) an I run directly followed by a D run, and the reverse: under the corpus's penalties (mismatch 4, gap 6 + 2 per base) the oracle
# never produces one inside an aligned core — a ops of an I run beside b of a D run always cost 6 more than min(a, b) mismatches and
# one run of |a - b| — so such strings go to the host statement only (test_deletions_abi.py); test_corpus_holds_what_it_is_for
# checks the oracle's strings.
ADJACENT = (b"MMMIIIDDMMM", b"MMDDIIIMXIM", b"MIDIDIM", b"IIMMIIDMIIMDD")


def _cannot_slide(f, p, n):
    """A deletion of f[p .. p + n) has one best place: its first base differs from the base after it, its last from the one before."""
    return f[p] != f[p + n] and f[p + n - 1] != f[p - 1]


def _site(f, p, lens):
    """The first position at or behind p where deletions of every length of `lens` cannot slide."""
    while not all(_cannot_slide(f, p, n) for n in lens):
        p += 1
    return p


def corpus(seed=23, depth=20):
    """Three references of 2.5-3.5 kb (the third with an N run) under ~20x of 100-200 base reads at 3 %, cut from a donor that lacks
    1-3 base stretches where the deletion cannot slide (a; every second read is stored reverse-complemented); the STAGE reference,
    covered only by unmutated hand-made reads whose windows start at t_start > 0, with the sites b-g; a reference shorter than 64 bases
    and an empty one.  Returns refs, reads, the window list and the planted sites name -> (reference, first deleted base, length)."""
    rng = np.random.default_rng(seed)
    refs = ["".join(LETTERS[rng.integers(0, 4, n)]) for n in (2500, 3500, 3000, 3200)]
    j, a, b = N_RUN
    under_n = refs[j]
    refs[j] = under_n[:a] + "N" * (b - a) + under_n[b:]
    planted = {}
    reads, rows = [], []

    def add(read, j, t0, t_len):
        k = len(reads)
        rev = k % 2 == 1
        reads.append(revcomp(read) if rev else read)
        rows.append((k, j, 0, len(read), t0, t_len, int(rev)))

    # (a): the random part
    for r in range(3):
        f = under_n if r == j else refs[r]
        L = len(f)
        sites = {}
        while len(sites) < 6:
            p, n = int(rng.integers(200, L - 200)), int(rng.integers(1, 4))
            if all(abs(p - q) > 40 for q in sites) and not (r == j and a - 40 < p < b + 40) and _cannot_slide(f, p, n):
                sites[p] = n
                planted[f"a{r}_{len(sites)}"] = (r, p, n)
        gone = np.zeros(L, bool)
        for p, n in sites.items():
            gone[p:p + n] = True
        ref_of = np.flatnonzero(~gone)               # donor position -> reference position
        donor = np.array([LETTER_COL[ord(x)] for x in f])[ref_of]
        for _ in range(L * depth // 150):
            n = int(rng.integers(100, 201))
            pos = int(rng.integers(0, len(donor) - n + 1))
            lo, hi = int(ref_of[pos]), int(ref_of[pos + n - 1]) + 1
            s = "".join(LETTERS[mutate(rng, donor[pos:pos + n], 0.03)])
            t0, t1 = max(0, lo - int(rng.integers(0, 21))), min(L, hi + int(rng.integers(0, 21)))
            add(s, r, t0, t1 - t0)

    # the stage: read = left flank + right flank around the deleted stretch, its window the flanks and the stretch, so its ops are
    # L x M, n x I, R x M
    f = refs[STAGE]

    def stage(name, p, carriers, winner):
        planted[name] = (STAGE, p, winner)
        for n, left, right in carriers:
            add(f[p - left:p] + f[p + n:p + n + right], STAGE, p - left, left + n + right)

    p = _site(f, 300, (2, 4))                          # (b) two lengths, 5 reads against 4
    stage("b", p, [(2, 50 + k, 60) for k in range(5)] + [(4, 45 + k, 70) for k in range(4)], 2)
    p = _site(f, 600, (3, 2))                          # (c) an exact tie of two lengths: the shorter
    stage("c", p, [(3, 50 + k, 60) for k in range(4)] + [(2, 45 + k, 70) for k in range(4)], 2)
    # (d) 70 bases, longer than one 64-op round: from ops 30, 35, .. 65, and from op 64, which fills a round; one read deletes 69
    p = _site(f, 900, (70, 69))
    stage("d", p, [(70, 30 + 5 * k, 90 - 5 * k) for k in range(8)] + [(70, 64, 60), (69, 64, 60)], 70)
    p = _site(f, 1400, (5,))                           # (e) runs over op index 63/64 and 127/128, and at the boundaries' sides
    stage("e", p, [(5, left, 40) for left in (59, 60, 61, 62, 63, 64, 123, 124, 125, 126, 127, 128)], 5)
    p = _site(f, 1800, (3,))                           # (f) an N beside the gap: a flagged pair, aligned on its bytes
    planted["f"] = (STAGE, p, 3)
    for k in range(6):
        add(f[p - 40 - k:p] + f[p + 3:p + 53], STAGE, p - 40 - k, 40 + k + 3 + 50)
    for k in range(3):
        add(f[p - 45 - k:p - 2] + "N" + f[p - 1] + f[p + 3:p + 58], STAGE, p - 45 - k, 45 + k + 3 + 55)
    p = _site(f, 2200, (12,))                          # (g) a deletion nested inside the longer deletion of other reads: two rows
    q = _site(f, p + 4, (3,))
    assert p + 4 <= q and q + 3 <= p + 10
    stage("g", p, [(12, 50 + k, 60) for k in range(6)], 12)
    stage("g_in", q, [(3, 55 + k, 66) for k in range(5)], 3)

    refs = refs + ["".join(LETTERS[rng.integers(0, 4, 41)]), ""]
    return refs, reads, as_list(rows), planted


@functools.lru_cache(maxsize=None)
def expectation():
    """The corpus and, computed once from the ORACLE's op strings: the pileup tables (reduce_common), every pair's records
    (`per_pair[q]`: list of (h, n)), per reference `records[j]`: row -> the lengths of the records that start there, and the starts
    planes.  Asserts that every planted site comes back with its planted length at min_depth 8, min_frac 0.5."""
    refs, reads, W, planted = corpus()
    pats, txts = materialise(reads, refs, W)
    o = loader.run(loader.oracle(), loader.make_config(**KW), datagen.from_strings(pats, txts, upper=True))
    tables, cover = expected_tables([len(r) for r in refs], o, pats, W["j"], W["t_start"], W["t_len"])
    for t in tables:
        t.setflags(write=False)
    per_pair = [py_ops_deletions(ops) if o["status"][q] == 0 else [] for q, ops in enumerate(o["cigars"])]
    records = records_of(per_pair, W, len(refs))
    starts = starts_of(records, refs)
    e = dict(refs=refs, reads=reads, W=W, planted=planted, o=o, pats=pats, tables=tables, cover=cover, per_pair=per_pair, records=records,
             starts=starts)
    for name, (j, p, n) in planted.items():
        if name == "g_in":       # (a minority at its row: it comes back under a lower min_frac)
            continue
        got = py_deletions(tables[j][p:p + 1], starts[j][p:p + 1], {0: records[j].get(p, [])}, j, p, 8, 500)
        assert len(got) == 1 and got[0][5] == n, (name, j, p, n, got)
    return e


def records_of(per_pair, W, nrefs, keep=None):
    """Per reference: row -> the list of the lengths of the records of the pairs `keep` selects (None: all) that start there."""
    out = [collections.defaultdict(list) for _ in range(nrefs)]
    for q, recs in enumerate(per_pair):
        if keep is None or keep[q]:
            for h, n in recs:
                out[int(W["j"][q])][int(W["t_start"][q]) + h].append(n)
    return out


def starts_of(records, refs):
    """The starts plane of every reference."""
    out = []
    for j, r in enumerate(refs):
        s = np.zeros(len(r), np.int32)
        for g, lens in records[j].items():
            s[g] = len(lens)
        out.append(s)
    return out


def all_rows(tables, starts, records, min_depth, min_permille, max_reads=MAX_READS):
    """Every sequence: the rows in ascending (j, pos)."""
    return np.concatenate([py_deletions(t, starts[j], records[j], j, 0, min_depth, min_permille, max_reads) for j, t in enumerate(tables)])


@functools.lru_cache(maxsize=None)
def expected_deletions(min_depth, min_permille, max_reads=MAX_READS):
    e = expectation()
    rows = all_rows(e["tables"], e["starts"], e["records"], min_depth, min_permille, max_reads)
    rows.setflags(write=False)
    return rows


def in_range(rows, seq, start, length):
    return rows[(rows[:, 0] == seq) & (rows[:, 1] >= start) & (rows[:, 1] < start + length)]
