"""Shared by the tests of the insertion log of a pileup: the rule restated in plain Python, straight from the text of include/wfa_hip.h
("insertions"), and a corpus whose reads carry planted insertions with known letters.  Expected records, rows and letters come from
the ORACLE's op strings, never from the device."""
import collections
import functools

import numpy as np

from oracle import loader
from pywfa_amd import datagen
from reduce_common import LETTER_COL, core_of, expected_tables
from test_windows_gpu import LETTERS, as_list, materialise, mutate, revcomp

KW = dict(span="ends-free", text_begin_free=20, text_end_free=20)
ASCII = "ACGTN"
MAX_READS = 4096


# ---- the rule ---------------------------------------------------------------------------------------------------------------------

def py_ops_insertions(ops, pattern):
    """The records of one pair: (h, n, columns) per maximal D run of the aligned core, h window-relative."""
    ops, pattern = bytes(ops), bytes(pattern)
    core = core_of(ops)
    out = []
    if core is None:
        return out
    v = h = k = 0
    while k <= core[1]:
        c = ops[k]
        if c == ord("D"):
            e = k
            while ops[e] == ord("D"):
                e += 1
            if k > core[0]:
                out.append((h, e - k, tuple(LETTER_COL.get(x, 4) for x in pattern[v:v + e - k])))
            v += e - k
            k = e
        else:
            v += c in b"MX"
            h += c in b"MXI"
            k += 1
    return out


def py_insertions(counts, records_at, seq, start, min_depth, min_permille, max_reads=MAX_READS):
    """The rows (int32, n x 8) and the letters (str per row) of the rows of `counts`; `records_at`: row -> list of (n, columns)."""
    rows, seqs = [], []
    for g in range(len(counts)):
        c = [int(x) for x in counts[g]]
        depth = sum(c[:6])
        if depth < min_depth:
            continue
        if min_permille > 0:
            if not (c[6] >= 1 and 1000 * c[6] >= min_permille * depth):
                continue
        elif not 2 * c[6] > depth:
            continue
        if c[6] > max_reads:
            rows.append([seq, start + g, depth, c[6], 0, 0, 0, 1])
            seqs.append("")
            continue
        alleles = collections.Counter(records_at.get(g, []))
        (n, cols), count = min(alleles.items(), key=lambda kv: (-kv[1], kv[0][0], kv[0][1]))
        rows.append([seq, start + g, depth, c[6], count, n, len(alleles), 0])
        seqs.append("".join(ASCII[x] for x in cols))
    return np.array(rows, np.int64).reshape(-1, 8).astype(np.int32), seqs


def py_splice(calls, rows, seqs, start):
    """consensus(insertions=True) from the call bytes of [start, start + len(calls)) and the rows / letters of that range under the
    majority rule."""
    at = {int(r[1]): s for r, s in zip(rows, seqs)}
    out = []
    for g, code in enumerate(calls):
        if code & 8:
            out.append(at[start + g])
        if code & 7 != 5:
            out.append("ACGTN-N"[code & 7])
    return "".join(out)


# ---- the corpus -------------------------------------------------------------------------------------------------------------------

STAGE = 3            # the reference only hand-made, unmutated reads cover: every record at its sites is known by construction
N_RUN = (2, 1200, 1216)


def _cannot_slide(f, p, s):
    """An insertion of the letters `s` in front of base p of `f` has one best place: its ends differ from their neighbours."""
    return s[0] != f[p] and s[-1] != f[p - 1]


def _allele(rng, f, p, n, avoid=()):
    while True:
        s = "".join(LETTERS[rng.integers(0, 4, n)])
        if _cannot_slide(f, p, s) and s not in avoid:
            return s


def corpus(seed=11, depth=20):
    """Three references of 2.5-3.5 kb (the third with an N run) under ~20x of 100-200 base reads at 3 %, cut from a donor that carries
    homozygous 1-3 base insertions where they cannot slide (a, and g: every second read is stored reverse-complemented); the STAGE
    reference, covered only by unmutated hand-made reads whose windows start at t_start > 0 (h), with the sites b-f; a reference
    shorter than 64 bases and an empty one (i).  Returns refs, reads, the window list and the planted sites
    name -> (reference, position, the allele the rule must recover)."""
    rng = np.random.default_rng(seed)
    refs = ["".join(LETTERS[rng.integers(0, 4, n)]) for n in (2500, 3500, 3000, 2600)]
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

    # (a), (g): the random part
    for r in range(3):
        f = under_n if r == j else refs[r]
        L = len(f)
        sites = {}
        while len(sites) < 6:
            p = int(rng.integers(60, L - 60))
            if all(abs(p - q) > 40 for q in sites) and not (r == j and a - 40 < p < b + 40):
                sites[p] = _allele(rng, f, p, int(rng.integers(1, 4)))
                planted[f"a{r}_{len(sites)}"] = (r, p, sites[p])
        donor, start_of = [], np.zeros(L + 1, np.int64)
        for p in range(L):
            start_of[p] = len(donor)
            donor.extend(sites.get(p, ""))
            donor.append(f[p])
        start_of[L] = len(donor)
        donor = np.array([LETTER_COL[ord(x)] for x in donor])
        for _ in range(L * depth // 150):
            n = int(rng.integers(100, 201))
            pos = int(rng.integers(0, len(donor) - n + 1))
            lo = int(np.searchsorted(start_of, pos, side="right")) - 1
            hi = int(np.searchsorted(start_of, pos + n, side="left"))
            s = "".join(LETTERS[mutate(rng, donor[pos:pos + n], 0.03)])
            t0, t1 = max(0, lo - int(rng.integers(0, 21))), min(L, hi + int(rng.integers(0, 21)))
            add(s, r, t0, t1 - t0)

    # the stage: read = left flank + allele + right flank, its window exactly the flanks, so its ops are L x M, n x D, R x M
    f = refs[STAGE]

    def stage(name, p, carriers, winner):
        planted[name] = (STAGE, p, winner)
        for allele, left, right in carriers:
            add(f[p - left:p] + allele + f[p:p + right], STAGE, p - left, left + right)

    p = 300                                            # (b) two alleles of different length, 5 against 4
    x = _allele(rng, f, p, 2)
    y = _allele(rng, f, p, 4)
    stage("b", p, [(x, 50 + k, 60) for k in range(5)] + [(y, 45 + k, 70) for k in range(4)], x)
    p = 600                                            # (c) an exact tie of two lengths: the shorter
    x = _allele(rng, f, p, 3)
    y = _allele(rng, f, p, 2)
    stage("c_len", p, [(x, 50 + k, 60) for k in range(4)] + [(y, 45 + k, 70) for k in range(4)], y)
    p = 900                                            # (c) an exact tie of two letter sequences of one length: the smaller
    x = _allele(rng, f, p, 3)
    y = _allele(rng, f, p, 3, avoid=(x,))
    stage("c_let", p, [(x, 50 + k, 60) for k in range(4)] + [(y, 45 + k, 70) for k in range(4)],
          min(x, y, key=lambda s: [ASCII.index(c) for c in s]))
    p = 1200                                           # (d) 70 bases, longer than one 64-op round; one read differs in one letter
    x = _allele(rng, f, p, 70)
    y = x[:33] + LETTERS[(ASCII.index(x[33]) + 1) % 4] + x[34:]
    stage("d", p, [(x, 30 + 5 * k, 90 - 5 * k) for k in range(8)] + [(y, 64, 60)], x)
    p = 1600                                           # (e) runs over op index 63/64 and 127/128, and at the boundaries' sides
    x = _allele(rng, f, p, 5)
    stage("e", p, [(x, left, 40) for left in (59, 60, 61, 62, 63, 64, 123, 124, 125, 126, 127, 128)], x)
    p = 2000                                           # (f) an N inside: a flagged pair, aligned on its bytes
    x = _allele(rng, f, p, 1) + "N" + _allele(rng, f, p, 1)
    stage("f", p, [(x, 40 + k, 50) for k in range(8)], x)

    refs = refs + ["".join(LETTERS[rng.integers(0, 4, 41)]), ""]
    return refs, reads, as_list(rows), planted


@functools.lru_cache(maxsize=None)
def expectation():
    """The corpus and, computed once from the ORACLE's op strings: the pileup tables (reduce_common) and every pair's records —
    `records[j]`: row -> list of (n, columns); `per_pair[q]`: the pair's list of (h, n, columns)."""
    refs, reads, W, planted = corpus()
    pats, txts = materialise(reads, refs, W)
    o = loader.run(loader.oracle(), loader.make_config(**KW), datagen.from_strings(pats, txts, upper=True))
    tables, cover = expected_tables([len(r) for r in refs], o, pats, W["j"], W["t_start"], W["t_len"])
    for t in tables:
        t.setflags(write=False)
    per_pair = [py_ops_insertions(ops, pats[q].encode()) if o["status"][q] == 0 else [] for q, ops in enumerate(o["cigars"])]
    return dict(refs=refs, reads=reads, W=W, planted=planted, o=o, pats=pats, tables=tables, cover=cover, per_pair=per_pair,
                records=records_of(per_pair, W, len(refs)))


def records_of(per_pair, W, nrefs, keep=None):
    """Per reference: row -> the list of (n, columns) of the pairs `keep` selects (None: all)."""
    out = [collections.defaultdict(list) for _ in range(nrefs)]
    for q, recs in enumerate(per_pair):
        if keep is None or keep[q]:
            for h, n, cols in recs:
                out[int(W["j"][q])][int(W["t_start"][q]) + h].append((n, cols))
    return out


@functools.lru_cache(maxsize=None)
def expected_insertions(min_depth, min_permille, max_reads=MAX_READS):
    """Every sequence: (rows in ascending (j, pos), the letters of the rows)."""
    e = expectation()
    rows, seqs = [], []
    for j, t in enumerate(e["tables"]):
        r, s = py_insertions(t, e["records"][j], j, 0, min_depth, min_permille, max_reads)
        rows.append(r)
        seqs += s
    rows = np.concatenate(rows)
    rows.setflags(write=False)
    return rows, tuple(seqs)


def in_range(rows, seqs, seq, start, length):
    keep = (rows[:, 0] == seq) & (rows[:, 1] >= start) & (rows[:, 1] < start + length)
    return rows[keep], tuple(s for s, k in zip(seqs, keep) if k)
