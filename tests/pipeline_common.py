"""Shared by the end-to-end tests of the paired-read pipeline (test_pipeline_truth.py, test_pipeline_gpu.py): a tiny genome with
engineered loci, a diploid sample with planted variants, simulated paired reads with PCR copies and planted truth, and the expected
output of EVERY call of the README's pipeline, composed without the device: each stage is the project's restated rule applied to the
ORACLE's alignments (oracle.loader.run) of the materialised windows of the stage before, never to a device output.

    seed_index(G, k=11) -> seeds(R, n=4)                           seed_common.py_index / py_seeds
    place_pairs(rescue, duplicates, unclipped, by quality)         place_common.py_place through pair_common.py_pair, rescue_common.py_rescue,
                                                                   dup_ends_common.py_duplicates_ex with py_clips and py_qsum
    pileup(left_align, insertions, deletions, strands, qualities)  leftalign_common.py_left_align, qual_common.tables_q,
                                                                   insertions_common.py_ops_insertions, deletions_common.py_ops_deletions
    genotypes / sites / insertions / deletions / consensus         qual_common.py_genotypes_quals, genotype_common.py_genotypes,
                                                                   calls_common.py_sites / py_calls, insertions_common.py_insertions /
                                                                   py_splice, deletions_common.py_deletions
    align_windows(left_align, sam)                                 sam_common.py_sam

Every stage has a Python restatement, so no expectation comes from a host C++ statement (`_native.*_host`).

The rescue hop takes two oracle runs (as rescue_common does): the listed windows under the aligner's configuration (KW), the rescue
windows under KW_RESCUE.  A third run gives the alignments of the piled-up primaries: a primary that is a rescue hit (hit >= n0) comes
from res["rescue"], and because a rescue window is as wide as the insert range while the aligner's own free ends are the seed pad, the
hand-off narrows it to the primary's interval (reads["text_start"], reads["text_end"]) padded by the free ends — README, "Mate rescue".

What the corpus adds to the planted sample so that every hand-off of the pipeline occurs: START fragments that begin within 30 bases
of the start of reference 2 (their seed windows are clipped by the text's end and they give the SNV at base 40 its depth), and ORPHAN
fragments whose mate 2 is a failed read (all N) and whose mate 1 is a forward read so near the end of its text that the rule makes no rescue
window for mate 2 (a kept read whose fragment's other mate is unplaced)."""
import functools

import numpy as np

from calls_common import py_calls, py_sites_all
from deletions_common import all_rows as deletion_rows, py_ops_deletions, records_of as deletion_records, starts_of
from dup_ends_common import BY_QUALITY, UNCLIPPED, py_clips, py_duplicates_ex, py_qsum
from genotype_common import py_genotypes_all
from insertions_common import py_insertions, py_ops_insertions, py_splice, records_of as insertion_records
from leftalign_common import py_left_align
from oracle import loader
from pair_common import PAIR_COLUMNS, py_pair
from place_common import COLUMNS, INT32_MIN, hits_of
from pywfa_amd import datagen
from qual_common import fastq, py_genotypes_quals_all, tables_q
from reduce_common import py_summary
from rescue_common import join_hits, py_rescue, window_list
from sam_common import py_sam
from chain_common import py_chains
from seed_common import mutate as mutate_bytes, py_index, py_seeds
from test_windows_gpu import LETTERS, materialise, revcomp

K, NSEEDS, PAD, ROOM = 11, 4, 16, 2
# gap-affine 4/6/2, scope full (the defaults); the text's ends free by the seed pad plus ROOM, the longest planted insertion: the window
# of `seeds` is wider than the read plus 2 * pad by the spread of the cluster's diagonals, which is what an insertion of n bases adds
# on either side (README, "No index of your own")
ENDS = PAD + ROOM
KW = dict(span="ends-free", text_begin_free=ENDS, text_end_free=ENDS)
MIN_INSERT, MAX_INSERT, RESCUE_PAD, GAP = 200, 500, 16, 24
FREE = (MAX_INSERT - MIN_INSERT) + 2 * RESCUE_PAD
KW_RESCUE = dict(KW, text_begin_free=FREE, text_end_free=FREE)
PY = dict(min_score=INT32_MIN, full_gap=GAP, min_insert=MIN_INSERT, max_insert=MAX_INSERT, unpaired=GAP)
MIN_MAPQ, MBQ, QCAP, DUP_MINQ = 20, 13, 40, 15
GENO_Q, GENO_STRAND, SITES, INDELS, CONS_DEPTH = (8, 200, 20, 0), (8, 200, 20, 2), (8, 500), (8, 200), 4
L, NFRAG, COPY_EVERY, DROP_EVERY, NSTART, NORPHAN = 100, 1200, 10, 15, 16, 6
SEGMENT = ((0, 1000), (1, 2000), 400)                                        # reference 0 [1000, 1400) copied to reference 1 [2000, 2400)
N_AT = (350, 1000, 1650, 2700, 3650)                                         # the single Ns of reference 1


def _other(c, k=1):
    return "ACGT"[("ACGT".index(c) + k) % 4]


# ---- the genome and the sample --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def genome(seed=2025):
    """(refs, haps, maps, variants, zones).  haps[j][h]: the sample's two sequences of reference j; maps[j][h][x]: the reference base
    under haplotype base x (an inserted base: the reference base behind it); variants: dicts with j, pos (VCF style: the leftmost
    place, for an indel the base in front of the event), ref, alt, gt (1 het: haplotype 1 alone carries it; 2 hom), kind and row (the
    first table row the event shows at: the base itself, the first deleted base, the base behind an insertion); zones: per reference
    the intervals round the indels that no read may start or end in."""
    rng = np.random.default_rng(seed)
    refs = [list("".join(LETTERS[rng.integers(0, 4, n)])) for n in (6000, 4000, 3000)]
    (ja, a), (jb, b), n = SEGMENT
    refs[jb][b:b + n] = refs[ja][a:a + n]

    def plant(j, p, s, before, behind):
        """the repeat `s` at p, between letters that do not extend it"""
        refs[j][p:p + len(s)] = s
        if refs[j][p - 1] == before:
            refs[j][p - 1] = _other(before)
        if refs[j][p + len(s)] == behind:
            refs[j][p + len(s)] = _other(behind)

    for j, p in ((0, 2000), (2, 800)):
        plant(j, p, "A" * 8, "A", "A")
    for j, p in ((0, 2600), (2, 1500)):
        plant(j, p, "CA" * 5, "A", "C")
    for p in N_AT:
        refs[1][p] = "N"
    if refs[2][1199] == refs[2][1202]:                                       # the 3-base deletion at 1200 cannot slide
        refs[2][1199] = _other(refs[2][1202])
    ins2 = _other(refs[0][4999]) + _other(refs[0][5000], 2)                  # ... nor the 2-base insertion in front of 5000
    if ins2[1] == refs[0][4999]:
        ins2 = ins2[0] + _other(ins2[1])
    if ins2[0] == ins2[1]:
        ins2 = ins2[0] + next(c for c in "ACGT" if c not in (ins2[0], refs[0][4999], refs[0][5000]))
    refs = ["".join(r) for r in refs]
    snv = lambda j, p, gt, k=1: dict(kind="snv", j=j, pos=p, row=p, ref=refs[j][p], alt=_other(refs[j][p], k), gt=gt)   # noqa: E731
    dele = lambda j, p, n, gt: dict(kind="del", j=j, pos=p - 1, row=p, ref=refs[j][p - 1:p + n], alt=refs[j][p - 1], gt=gt, n=n)   # noqa: E731
    ins = lambda j, p, s, gt: dict(kind="ins", j=j, pos=p - 1, row=p, ref=refs[j][p - 1], alt=refs[j][p - 1] + s, gt=gt, seq=s)   # noqa: E731
    variants = [snv(0, p, 1, 1 + p % 3) for p in (400, 1700, 3000, 3400, 5400)] + [snv(0, p, 2, 1 + p % 3) for p in (700, 1012, 4200, 4600, 5700)]
    variants += [snv(1, p, 1, 1 + p % 3) for p in (650, 1300)] + [snv(1, p, 2, 1 + p % 3) for p in (3000, 3350)]
    variants += [dele(0, 2000, 1, 1), ins(0, 5000, ins2, 1)]
    variants += [snv(2, p, 2, 1 + p % 3) for p in (40, 400, 1900, 2600)] + [dele(2, 800, 1, 2), dele(2, 1200, 3, 2), ins(2, 1500, "CA", 2)]
    haps, maps = [], []
    for j, ref in enumerate(refs):
        hj, mj = [], []
        for h in (0, 1):
            mine = sorted((v for v in variants if v["j"] == j and (v["gt"] == 2 or h == 1)), key=lambda v: v["row"])
            out, at, x = [], [], 0
            for v in mine:
                p = v["row"]
                out += ref[x:p]
                at += range(x, p)
                if v["kind"] == "snv":
                    out.append(v["alt"])
                    at.append(p)
                    x = p + 1
                elif v["kind"] == "del":
                    x = p + v["n"]
                else:
                    out += v["seq"]
                    at += [p] * len(v["seq"])
                    x = p
            out += ref[x:]
            at += range(x, len(ref))
            hj.append("".join(out))
            mj.append(np.array(at))
        haps.append(hj)
        maps.append(mj)
    zones = [[], [], []]
    for j, lo, hi in ((0, 2000, 2008), (0, 2600, 2610), (0, 5000, 5000), (2, 800, 808), (2, 1200, 1203), (2, 1500, 1510)):
        zones[j].append((lo - 12, hi + 12))
    return refs, haps, maps, variants, zones


def consensus_truth():
    """The sample's sequence of reference 2 (both haplotypes are equal there) and the reference base under each of its bases."""
    _, haps, maps, _, _ = genome()
    assert haps[2][0] == haps[2][1]
    return haps[2][0], maps[2][0]


# ---- the reads ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def corpus(seed=7):
    """(reads, quals, frags).  Fragment f is reads 2 f (mate 1) and 2 f + 1 (mate 2); quals: a uint8 array per read.  frags[f]: dict
    with kind ("plain", "copy", "start", "orphan"), j, hap, flip (mate 1 is the right-hand, reverse mate), copy_of (the fragment it
    copies, or None), drop (its mate-2 windows are removed before place_pairs), first_base (the copy carries a substitution in the
    first stored base of that mate, or None) and per mate (m1, m2) its true place on the reference [start, end) and strand.

    NFRAG plain fragments: haplotype and place drawn per fragment, insert 250 .. 450, the forward mate stored as it is and the reverse
    mate reverse-complemented, every second fragment with mate 1 as the reverse mate; 1 % substitutions with quality 5, every other
    base 30 .. 40; no indels.  No mate starts or ends within 12 bases of a planted indel or its repeat, no error falls there (left
    alignment does not move a gap through a mismatch), a mate on an edge of the copied segment has 12 bases outside it, and no two fragments share reference, start and end.  Every COPY_EVERY-th is followed by a PCR copy: the same ends, its own errors, every quality but an
    error's 10 lower, and for every third copy a substitution in the first stored base of mate 1 or mate 2 in turn.  Every
    DROP_EVERY-th plain fragment (marked `drop` unless it has a copy or touches the copied segment) lies at least 520 bases from both ends of its text, so that a rescue window for it is never clipped
    away.  Then the START and ORPHAN fragments of the module docstring."""
    refs, haps, maps, _, zones = genome()
    rng = np.random.default_rng(seed)
    reads, quals, frags, taken = [], [], [], set()
    weights = np.array([len(r) for r in refs], float) / sum(len(r) for r in refs)

    def sequenced(s, quiet, lower=0, force_first=False):
        err = (rng.random(len(s)) < 0.01) & ~quiet
        if force_first:
            err[0] = True
        out = [_other(c, 1 + int(rng.integers(0, 3))) if e and c != "N" else c for c, e in zip(s, err)]
        q = np.where(err, 5, rng.integers(30, 41, len(s)) - lower).astype(np.uint8)
        return "".join(out), q

    def emit(kind, j, h, x0, x1, flip, copy_of=None, drop=False, first_base=None):
        hap, m = haps[j][h], maps[j][h]
        left, right = hap[x0:x0 + L], revcomp(hap[x1 - L:x1])
        place_l, place_r = (int(m[x0]), int(m[x0 + L - 1]) + 1, 0), (int(m[x1 - L]), int(m[x1 - 1]) + 1, 1)
        (s1, t1), (s2, t2) = ((right, place_r), (left, place_l)) if flip else ((left, place_l), (right, place_r))
        for k, (s, (lo, hi, rev)) in enumerate(((s1, t1), (s2, t2))):
            at = m[x1 - L:x1][::-1] if rev else m[x0:x0 + L]
            quiet = np.zeros(L, bool)
            for zlo, zhi in zones[j]:
                quiet |= (at >= zlo) & (at <= zhi)
            r, q = sequenced(s, quiet, 10 if kind == "copy" else 0, first_base == k)
            reads.append(r)
            quals.append(q)
        touches = any(js == j and lo < s0 + SEGMENT[2] and hi > s0 for js, s0 in SEGMENT[:2] for lo, hi, _ in (place_l, place_r))
        frags.append(dict(kind=kind, j=j, hap=h, flip=flip, copy_of=copy_of, drop=drop and not touches, first_base=first_base, m1=t1, m2=t2, x=(x0, x1)))

    def clear(j, h, x0, x1):
        m = maps[j][h]
        ends = (int(m[x0]), int(m[x0 + L - 1]), int(m[x1 - L]), int(m[x1 - 1]))
        key = (j, ends[0], ends[3])
        if key in taken or any(lo <= e <= hi for e in ends for lo, hi in zones[j]):
            return False
        for lo, hi in ((ends[0], ends[1] + 1), (ends[2], ends[3] + 1)):    # a mate on an edge of the copied segment: 12 bases outside it
            for js, s0 in SEGMENT[:2]:
                if js == j and lo < s0 + SEGMENT[2] and hi > s0 and 0 < max(s0 - lo, 0) + max(hi - s0 - SEGMENT[2], 0) < 12:
                    return False
        taken.add(key)
        return True

    ncopies = 0
    for f in range(NFRAG):
        drop = f % DROP_EVERY == 0
        while True:
            j, h, ins = int(rng.choice(3, p=weights)), int(rng.integers(0, 2)), int(rng.integers(250, 451))
            margin = 520 if drop else 0
            x0 = int(rng.integers(margin, len(haps[j][h]) - ins - margin + 1))
            if clear(j, h, x0, x0 + ins):
                break
        emit("plain", j, h, x0, x0 + ins, f % 2 == 1, drop=drop and f % COPY_EVERY != 0)
        if f % COPY_EVERY == 0:
            emit("copy", j, h, x0, x0 + ins, f % 2 == 1, copy_of=len(frags) - 1, first_base=(ncopies // 3) % 2 if ncopies % 3 == 0 else None)
            ncopies += 1
    for x0 in rng.permutation(31)[:NSTART]:
        ins = int(rng.integers(250, 451))
        assert clear(2, 0, int(x0), int(x0) + ins)
        emit("start", 2, int(rng.integers(0, 2)), int(x0), int(x0) + ins, len(frags) % 2 == 1)
    for k in range(NORPHAN):
        j = k % 3
        n = len(haps[j][0])
        x0 = int(rng.integers(n - 400, n - L - 120))
        assert clear(j, 0, x0, x0 + L + 100)
        emit("orphan", j, 0, x0, x0 + L + 100, False)
        reads[-1] = "N" * L                                                   # mate 2: a failed read, no k-mer of it is in the index
        quals[-1] = np.full(L, 2, np.uint8)
        frags[-1]["m2"] = None
    for q in quals:
        q.setflags(write=False)
    return tuple(reads), tuple(quals), tuple(frags)


def fastq_quals():
    return [fastq(q) for q in corpus()[1]]


# ---- the hand-offs, as the README writes them (used by the expectation AND by the GPU test, on its own arrays) ------------------------

def windows_of_seeds(s):
    """The window list of a seed result: the rows with j >= 0 (the padding is filtered), `reverse` as uint8."""
    keep = s["j"] >= 0
    return dict(i=np.nonzero(keep)[0], j=s["j"][keep], text_start=s["text_start"][keep], text_len=s["text_len"][keep],
                reverse=s["reverse"][keep].astype(np.uint8))


def without_dropped(w):
    """The list without the windows of mate 2 that overlap its true place, for the fragments marked `drop`."""
    frags = corpus()[2]
    keep = np.ones(len(w["i"]), bool)
    for f, fr in enumerate(frags):
        if fr["drop"]:
            lo, hi, _ = fr["m2"]
            keep &= ~((w["i"] == 2 * f + 1) & (w["j"] == fr["j"]) & (w["text_start"] < hi) & (w["text_start"] + w["text_len"] > lo))
    return {k: v[keep] for k, v in w.items()}


def kept_reads(reads):
    """The README's filter: placed, no duplicate, confidently mapped."""
    return np.nonzero((reads["hit"] >= 0) & (reads["dup"] == 0) & (reads["mapq"] >= MIN_MAPQ))[0]


def primaries(w, res, i):
    """The windows of the primaries of the reads `i`: hit h < n0 is window h of the caller's list `w`; hit n0 + q is window q of
    res["rescue"], narrowed to the primary's interval padded by PAD (a rescue window is as wide as the insert range, the aligner's
    own free ends are ENDS)."""
    n0 = len(w["i"])
    h = res["reads"]["hit"][i].astype(np.int64)
    own, q = np.minimum(h, n0 - 1), np.maximum(h - n0, 0)
    rs = res["rescue"]
    if len(rs["i"]) == 0:
        assert (h < n0).all()
        rs = {k: np.zeros(1, np.int32) for k in rs}
    lo = np.maximum(rs["text_start"][q], res["reads"]["text_start"][i] - ENDS)
    hi = np.minimum(rs["text_start"][q] + rs["text_len"][q], res["reads"]["text_end"][i] + ENDS)
    pick = lambda a, b: np.where(h < n0, a[own], b)   # noqa: E731
    out = dict(i=pick(w["i"], rs["i"][q]), j=pick(w["j"], rs["j"][q]).astype(np.int32), text_start=pick(w["text_start"], lo).astype(np.int32),
               text_len=pick(w["text_len"], hi - lo).astype(np.int32), reverse=pick(w["reverse"], rs["reverse"][q]).astype(np.uint8))
    assert np.array_equal(out["i"], i)
    return out


def as_rig_list(w, read_len):
    """The window list in the keys of the rigs (test_windows_gpu.as_list): the pattern window is the whole read."""
    i = np.asarray(w["i"], np.int64)
    return dict(i=i, j=np.asarray(w["j"], np.int32), p_start=np.zeros(len(i), np.int32), p_len=np.asarray(read_len, np.int64)[i],
                t_start=np.asarray(w["text_start"], np.int64), t_len=np.asarray(w["text_len"], np.int32), reverse=np.asarray(w["reverse"], np.uint8))


# ---- the composed expectation -----------------------------------------------------------------------------------------------------------

def kw_of(free=ENDS, rescue=False):
    """The aligner's configuration with `free` text bases free at either end; rescue: the free ends of the rescue alignments."""
    f = FREE if rescue else free
    return dict(KW, text_begin_free=f, text_end_free=f)


def oracle_list(kw, Wl):
    reads, refs = corpus()[0], genome()[0]
    pats, txts = materialise(reads, refs, Wl)
    o = loader.run(loader.oracle(), loader.make_config(**kw), datagen.from_strings(pats, txts, upper=True))
    return o, pats, txts


def clips_of(o, Wl):
    n = len(o["cigars"])
    c = np.array([py_clips(o["cigars"][q], int(Wl["p_len"][q]), int(Wl["t_len"][q])) for q in range(n)], np.int32).reshape(-1, 2)
    return c[:, 0], c[:, 1]


@functools.lru_cache(maxsize=None)
def expected_seeds():
    reads, refs = corpus()[0], genome()[0]
    texts = [r.encode() for r in refs]
    index = py_index(texts, K, 1)
    rows = [py_seeds(r.encode(), texts, index, k=K, n=NSEEDS) for r in reads]
    out = {k: np.array([row[k] for row in rows], np.int32).reshape(len(reads), NSEEDS) for k in ("j", "reverse", "text_start", "text_len", "hits")}
    out["overflow"] = np.array([row["overflow"] for row in rows], np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def expected_placement(dup_flags=UNCLIPPED | BY_QUALITY, free=ENDS):
    """The result of place_pairs(..., rescue=True, duplicates=True, ...) as a dict of the same keys, plus `w` (the caller's list) and
    `hits` / `lead` / `trail` (the hit list of both window lists with the clips)."""
    reads, quals, frags = corpus()
    refs = genome()[0]
    nr, nf = len(reads), len(frags)
    read_len, text_len = [len(r) for r in reads], [len(r) for r in refs]
    w = without_dropped(windows_of_seeds(expected_seeds()))
    W0 = as_rig_list(w, read_len)
    o0, _, _ = oracle_list(kw_of(free), W0)
    hits0 = hits_of(o0, W0, True)
    found = py_rescue(hits0, nr, nf, PY, read_len, text_len, RESCUE_PAD, FREE, 0)
    W1 = window_list(found, read_len)
    o1, _, _ = oracle_list(kw_of(rescue=True), W1)
    hits = join_hits(hits0, hits_of(o1, W1, True))
    rows, flags, pair_rows, pair_flags = py_pair(hits, nr, nf, *PY.values())
    lead, trail = (np.concatenate(x) for x in zip(clips_of(o0, W0), clips_of(o1, W1)))
    qsum = np.array([py_qsum(q, DUP_MINQ) for q in quals], np.int64)
    dup_reads, dup_pairs = py_duplicates_ex(hits, nr, nf, PY, text_len, lead, trail, dup_flags, qsum)
    n0 = len(W0["i"])
    out = dict(score=np.concatenate([o0["score"], o1["score"]]).astype(np.int32), status=np.concatenate([o0["status"], o1["status"]]).astype(np.int32),
               flag=flags, pair_flag=pair_flags, reads={k: rows[:, c].copy() for c, k in enumerate(COLUMNS)},
               pairs={k: pair_rows[:, c].copy() for c, k in enumerate(PAIR_COLUMNS)})
    out["pairs"]["rescued"] = ((pair_rows[:, 2] == 1) & ((pair_rows[:, 0] >= n0) | (pair_rows[:, 1] >= n0))).astype(np.int32)
    for part, d in (("reads", dup_reads), ("pairs", dup_pairs)):
        out[part].update(dup=d[:, 2].copy(), dup_rep=d[:, 0].copy(), dup_size=d[:, 1].copy(), dup_overflow=d[:, 3].copy())
    out["rescue"] = {k: found[:, c].copy() for c, k in enumerate(("i", "j", "text_start", "text_len", "reverse", "fragment", "anchor"))}
    out.update(w=w, hits=hits, lead=lead, trail=trail, n0=n0)
    return out


@functools.lru_cache(maxsize=None)
def expected_pile(left_align=True, free=ENDS):
    """The piled-up list and everything the pileup, its reductions and align_windows(sam=True) return for it: dict with `w` (the
    window list), `i` (the kept reads), score, status, ops (after the rewrite), counts / qsums / fwd / depth / starts per reference,
    geno_q, geno_strand, sites, insertions (rows, letters), deletions, consensus (of reference 2) and sam (rows, cigars, mds)."""
    reads, quals, _ = corpus()
    refs = genome()[0]
    res = expected_placement(free=free)
    i = kept_reads(res["reads"])
    w = primaries(res["w"], res, i)
    Wl = as_rig_list(w, [len(r) for r in reads])
    o, pats, txts = oracle_list(kw_of(free), Wl)
    ops = [py_left_align(c, pats[q].encode(), txts[q].encode())[0] if left_align and o["status"][q] == 0 else bytes(c) for q, c in enumerate(o["cigars"])]
    oo = dict(score=o["score"], status=o["status"], cigars=ops)
    lens = [len(r) for r in refs]
    counts, qsums, fwd = tables_q(lens, oo, pats, Wl, quals, MBQ, QCAP)
    ok = [st == 0 for st in o["status"]]
    del_rec = deletion_records([py_ops_deletions(c) if ok[q] else [] for q, c in enumerate(ops)], Wl, len(refs))
    ins_rec = insertion_records([py_ops_insertions(c, pats[q].encode()) if ok[q] else [] for q, c in enumerate(ops)], Wl, len(refs))
    starts = starts_of(del_rec, refs)
    ins_rows, ins_seqs = [], []
    for j, t in enumerate(counts):
        r, s = py_insertions(t, ins_rec[j], j, 0, *INDELS)
        ins_rows.append(r)
        ins_seqs += s
    cons_rows, cons_seqs = py_insertions(counts[2], ins_rec[2], 2, 0, CONS_DEPTH, 0)
    calls = py_calls(counts[2], refs[2].encode(), CONS_DEPTH)
    sam = [py_sam(c, txts[q].encode(), 0, int(o["status"][q])) for q, c in enumerate(ops)]
    sam_rows = np.array([s[0] for s in sam], np.int64).reshape(-1, 8)
    sam_rows[:, 0] = np.where(sam_rows[:, 0] >= 0, sam_rows[:, 0] + Wl["t_start"], sam_rows[:, 0])
    return dict(w=w, i=i, Wl=Wl, pats=pats, score=np.asarray(o["score"], np.int32), status=np.asarray(o["status"], np.int32), ops=ops, counts=counts,
                qsums=qsums, fwd=fwd, depth=[t[:, :6].sum(axis=1, dtype=np.int32) for t in counts], starts=starts,
                geno_q=py_genotypes_quals_all(counts, qsums, fwd, refs, GENO_Q), geno_strand=py_genotypes_all(counts, fwd, refs, GENO_STRAND),
                sites=py_sites_all(counts, refs, *SITES), insertions=(np.concatenate(ins_rows), tuple(ins_seqs)),
                deletions=deletion_rows(counts, starts, del_rec, *INDELS), consensus=py_splice(calls, cons_rows, cons_seqs, 0), calls=calls,
                sam=(sam_rows.astype(np.int32), [s[1].decode() for s in sam], [s[2].decode() for s in sam]))


# ---- the long-read route ----------------------------------------------------------------------------------------------------------------

NLONG, LONG_SPAN, LONG_DIV, LONG_STRIDE, LONG_N = 24, 1500, 0.06, 4, 2
KW_LONG = dict(span="ends-free", text_begin_free=200, text_end_free=200, heuristic="adaptive")


@functools.lru_cache(maxsize=None)
def long_reads(seed=31):
    """(reads, origin): NLONG reads that span LONG_SPAN bases of a reference, mutated at 6 % (substitutions, deletions and insertions
    in equal parts), every second one stored reverse-complemented; origin: (reference, position, span, reversed).  No read touches the
    copied segment or an N."""
    refs = genome()[0]
    rng = np.random.default_rng(seed)
    code = np.zeros(256, np.int64)
    code[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4)
    reads, origin = [], []
    while len(reads) < NLONG:
        j = int(rng.integers(0, 3))
        pos = int(rng.integers(0, len(refs[j]) - LONG_SPAN + 1))
        piece = refs[j][pos:pos + LONG_SPAN]
        if "N" in piece or any(js == j and pos < s0 + SEGMENT[2] and pos + LONG_SPAN > s0 for js, s0 in SEGMENT[:2]):
            continue
        s = np.frombuffer(b"ACGT", np.uint8)[mutate_bytes(rng, code[np.frombuffer(piece.encode(), np.uint8)], LONG_DIV)].tobytes().decode()
        rev = len(reads) % 2 == 1
        reads.append(revcomp(s) if rev else s)
        origin.append((j, pos, LONG_SPAN, int(rev)))
    return tuple(reads), tuple(origin)


def windows_of_chains(c):
    """The window list of a chain result: the rows with j >= 0, the whole read against the chain's window."""
    keep = c["j"] >= 0
    return dict(i=np.nonzero(keep)[0], j=c["j"][keep], text_start=c["text_start"][keep], text_len=c["text_len"][keep],
                reverse=c["reverse"][keep].astype(np.uint8))


@functools.lru_cache(maxsize=None)
def expected_long():
    """dict(chains=the arrays of chains(R, n=2) over seed_index(G, k=11, stride=4), w=the window list, score=, status=, summary=(n, 10)
    rows of align_windows(summary=True) under KW_LONG)."""
    refs = genome()[0]
    reads = long_reads()[0]
    texts = [r.encode() for r in refs]
    index = py_index(texts, K, LONG_STRIDE)
    rows = [py_chains(r.encode(), texts, index, k=K, stride=LONG_STRIDE, n=LONG_N) for r in reads]
    keys = ("j", "reverse", "text_start", "text_len", "hits", "score", "pattern_start", "pattern_len")
    chains = {k: np.array([row[k] for row in rows], np.int32).reshape(len(reads), LONG_N) for k in keys}
    chains["overflow"] = np.array([row["overflow"] for row in rows], np.uint8)
    w = windows_of_chains(chains)
    Wl = as_rig_list(w, [len(r) for r in reads])
    pats, txts = materialise(reads, refs, Wl)
    o = loader.run(loader.oracle(), loader.make_config(**KW_LONG), datagen.from_strings(pats, txts, upper=True))
    summary = np.array([py_summary(c, len(pats[q]), len(txts[q])) if o["status"][q] == 0 else np.zeros(10, np.int32) for q, c in enumerate(o["cigars"])],
                       np.int32).reshape(-1, 10)
    return dict(chains=chains, w=w, score=np.asarray(o["score"], np.int32), status=np.asarray(o["status"], np.int32), summary=summary)
