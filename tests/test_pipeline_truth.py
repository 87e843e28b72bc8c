"""The composed reference of the paired-read pipeline (pipeline_common) recovers the planted truth, without a GPU: placement, rescue,
duplicates, genotypes, indel rows, consensus and SAM fields, and the long-read route's loci.  This tests the RULES — every expectation
here is the oracle's alignments under the restated rules, and the answer is what was planted — and it is the guard that the corpus is
decisive for test_pipeline_gpu.py.  Every condition is asserted under the configuration the GPU test runs: the text's ends free by the
seed pad plus the longest planted insertion (pipeline_common.ENDS says why the pad alone is not enough)."""
import numpy as np

import pipeline_common as pc
from dup_ends_common import BY_QUALITY
from sam_common import ref_from
from test_windows_gpu import revcomp

REFS, HAPS, MAPS, VARIANTS, ZONES = pc.genome()
READS, QUALS, FRAGS = pc.corpus()
NF = len(FRAGS)
(JA, A0), (JB, B0), SEG = pc.SEGMENT


def in_segment(place, j):
    lo, hi, _ = place
    return any(jj == j and lo >= s and hi <= s + SEG for jj, s in ((JA, A0), (JB, B0)))


def touches_segment(place, j):
    lo, hi, _ = place
    return any(jj == j and lo < s + SEG and hi > s for jj, s in ((JA, A0), (JB, B0)))


def unclipped(res, h):
    """(text, strand, unclipped start, unclipped end) of hit h of the expected placement."""
    hits = res["hits"]
    return int(hits["j"][h]), int(hits["reverse"][h]), int(hits["text_start"][h]) - int(res["lead"][h]), int(hits["text_end"][h]) + int(res["trail"][h])


def test_the_corpus_is_what_it_says():
    kinds = [f["kind"] for f in FRAGS]
    assert kinds.count("plain") == pc.NFRAG and kinds.count("copy") == pc.NFRAG // pc.COPY_EVERY and kinds.count("start") == pc.NSTART
    assert kinds.count("orphan") == pc.NORPHAN and len(READS) == 2 * NF and all(len(r) == pc.L for r in READS)
    het = [v for v in VARIANTS if v["j"] < 2 and v["kind"] == "snv" and v["gt"] == 1]
    hom = [v for v in VARIANTS if v["j"] < 2 and v["kind"] == "snv" and v["gt"] == 2]
    assert len(het) >= 6 and len(hom) >= 6 and all(v["gt"] == 2 for v in VARIANTS if v["j"] == 2)
    assert REFS[JA][A0:A0 + SEG] == REFS[JB][B0:B0 + SEG] and REFS[1].count("N") == 5
    for j in (0, 2):
        assert "A" * 8 in REFS[j] and "CA" * 5 in REFS[j]
    rows = sorted((v["j"], v["row"]) for v in VARIANTS)
    loci = rows + [(JA, A0), (JB, B0)] + [(1, p) for p in pc.N_AT]
    for j, p in loci:                                                      # 300 bases from every other locus and from the text ends
        if (j, p) == (2, 40):
            continue
        assert 300 <= p <= len(REFS[j]) - 300, (j, p)
        near = [q for jj, q in loci if jj == j and q != p and abs(q - p) < 300 and {p, q} != {A0, 1012}]   # (the SNV INSIDE the copied segment)
        assert not near, (j, p, near)
    for f, fr in enumerate(FRAGS):                                         # the reads are the sample's, on the strands the truth says
        if fr["kind"] == "copy":
            src = FRAGS[fr["copy_of"]]
            assert (src["j"], src["m1"], src["m2"], src["flip"]) == (fr["j"], fr["m1"], fr["m2"], fr["flip"])
            assert all(int(QUALS[2 * f + k].astype(int).sum()) < int(QUALS[2 * fr["copy_of"] + k].astype(int).sum()) for k in (0, 1))
    assert sum(fr["first_base"] is not None for fr in FRAGS) == pc.NFRAG // pc.COPY_EVERY // 3
    # every 15th plain fragment, but for those with a copy (every 30th) and those that touch the copied segment
    plain = [fr for fr in FRAGS if fr["kind"] == "plain"]
    want_drop = [k % pc.DROP_EVERY == 0 and k % pc.COPY_EVERY != 0 and not any(touches_segment(fr[m], fr["j"]) for m in ("m1", "m2")) for k, fr in enumerate(plain)]
    assert [fr["drop"] for fr in plain] == want_drop and sum(want_drop) == 34 and not any(fr["drop"] for fr in FRAGS if fr["kind"] != "plain")
    s = pc.expected_seeds()
    assert not s["overflow"].any()
    w = pc.windows_of_seeds(s)
    clipped = (w["j"] == 2) & (w["text_start"] == 0) & (w["text_len"] < pc.L + 2 * pc.PAD)
    assert clipped.sum() >= 4                                              # windows that the start of reference 2 clips
    assert (np.array([set(REFS[j][a:a + n]) > set("ACGT") for j, a, n in zip(w["j"], w["text_start"], w["text_len"])])).sum() >= 20   # byte-kernel windows


def test_placement_and_rescue():
    res = pc.expected_placement()
    pairs, reads, n0 = res["pairs"], res["reads"], res["n0"]
    assert (res["status"] == 0).all()
    lone = 0
    for f, fr in enumerate(FRAGS):
        if fr["kind"] == "orphan":
            assert pairs["proper"][f] == 0 and reads["hit"][2 * f + 1] == -1 and reads["hit"][2 * f] >= 0 and reads["mapq"][2 * f] == 60, f
            assert unclipped(res, reads["hit"][2 * f])[:3] == (fr["j"], 0, fr["m1"][0])
            continue
        inside = [in_segment(fr[m], fr["j"]) for m in ("m1", "m2")]
        if all(inside):
            continue                                                       # both mates in the copy: the two places are equal
        assert pairs["proper"][f] == 1, (f, fr)
        for m, h in (("m1", pairs["hit1"][f]), ("m2", pairs["hit2"][f])):
            lo, hi, strand = fr[m]
            assert unclipped(res, h) == (fr["j"], strand, lo, hi), (f, m, fr, unclipped(res, h))
        if any(inside):
            lone += 1
            r = 2 * f + inside.index(True)
            assert reads["mapq"][r] == 0 and pairs["mapq"][f] >= pc.MIN_MAPQ, (f, reads["mapq"][r], pairs["mapq"][f])
        elif fr["kind"] != "copy" and not any(touches_segment(fr[m], fr["j"]) for m in ("m1", "m2")):
            assert pairs["mapq"][f] == 60, (f, pairs["mapq"][f])
        if fr["drop"]:
            assert pairs["rescued"][f] == 1 and pairs["hit2"][f] >= n0, f      # (the single-end primary too, unless a listed hit ties it)
        else:
            assert pairs["rescued"][f] == 0, f
    assert lone >= 5 and pairs["rescued"].sum() == sum(fr["drop"] for fr in FRAGS)


def test_duplicates():
    res = pc.expected_placement()
    pairs = res["pairs"]
    copies = {f: fr["copy_of"] for f, fr in enumerate(FRAGS) if fr["kind"] == "copy"}
    for f, src in copies.items():
        assert pairs["dup"][f] == 1 and pairs["dup_rep"][f] == src and pairs["dup_size"][f] == 2, (f, src)
        assert pairs["dup"][src] == 0 and pairs["dup_rep"][src] == src and pairs["dup_size"][src] == 2, (f, src)
        assert res["reads"]["dup"][2 * f] == 1 and res["reads"]["dup"][2 * f + 1] == 1
    assert pairs["dup"].sum() == len(copies) and res["reads"]["dup"].sum() == 2 * len(copies) and not pairs["dup_overflow"].any()
    core = pc.expected_placement(dup_flags=BY_QUALITY)["pairs"]["dup"]
    missed = [f for f in copies if core[f] == 0 and core[copies[f]] == 0]
    # every copy the core rule misses carries a substitution in a first or last base: the planted one, or an error of its own
    for f in missed:
        ends = [READS[2 * f + k][x] != READS[2 * copies[f] + k][x] for k in (0, 1) for x in (0, -1)]
        assert FRAGS[f]["first_base"] is not None or any(ends), f
    assert any(FRAGS[f]["first_base"] is not None for f in missed)         # the option is exercised


def planted_rows():
    """(j, row) -> (variant, alt code or "ins") for every table row a planted variant shows at."""
    out = {}
    for v in VARIANTS:
        if v["kind"] == "snv":
            out[(v["j"], v["row"])] = (v, "ACGT".index(v["alt"]))
        elif v["kind"] == "del":
            for k in range(v["n"]):
                out[(v["j"], v["row"] + k)] = (v, 5)
        else:
            out[(v["j"], v["row"])] = (v, "ins")
    return out


def check_genotypes(rows, p, both_strands=0):
    """Every row is a planted one with the planted alt and genotype, and every planted row is there — under min_alt_strand but for the
    events that the expected tables themselves show on fewer than that many reads of a strand."""
    want = planted_rows()
    seen = {}
    for r in rows:
        key = (int(r[0]), int(r[1]))
        assert key in want, ("an unplanted row", r.tolist())
        seen[key] = r
    for key, (v, alt) in want.items():
        j, g = key
        assert p["depth"][j][g] >= 8, ("a planted variant below depth 8: a corpus defect", v)
        r = seen.get(key)
        col = 6 if alt == "ins" else alt
        total, fwd = int(p["counts"][j][g, col]), int(p["fwd"][j][g, col])
        if both_strands and min(fwd, total - fwd) < both_strands:
            assert r is None, (v, total, fwd)
            continue
        assert r is not None, ("a planted variant is not reported", v)
        if alt == "ins":
            assert r[7] >= 1 and r[10] == v["gt"] and r[3] == -1, (v, r.tolist())
        else:
            assert r[3] == alt and r[8] == v["gt"], (v, r.tolist())
    return len(seen)


def test_genotypes():
    p = pc.expected_pile()
    assert check_genotypes(p["geno_q"], p) == len(planted_rows())
    assert check_genotypes(p["geno_strand"], p, pc.GENO_STRAND[3]) >= 12      # (at least the hom SNVs: both strands carry them)
    # without the rewrite the homopolymer deletions are reported elsewhere: left_align=True is not a silent no-op
    plain = pc.expected_pile(left_align=False)
    for v in (v for v in VARIANTS if v["kind"] == "del" and v["n"] == 1):
        at = lambda rows: {int(r[1]) for r in rows if r[0] == v["j"] and r[3] == 5 and v["row"] - 2 <= r[1] <= v["row"] + 10}   # noqa: E731
        assert at(p["geno_q"]) == {v["row"]} and v["row"] not in at(plain["geno_q"]) and at(plain["geno_q"]), (v, at(plain["geno_q"]))
    assert not np.array_equal(plain["counts"][2], p["counts"][2])


def test_indel_rows_and_consensus():
    p = pc.expected_pile()
    rows, seqs = p["insertions"]
    got = {(int(r[0]), int(r[1])): s for r, s in zip(rows, seqs)}
    for v in (v for v in VARIANTS if v["kind"] == "ins"):
        assert got.get((v["j"], v["row"])) == v["seq"], (v, got)
    assert len(got) == 2
    dels = {(int(r[0]), int(r[1])): int(r[5]) for r in p["deletions"]}
    for v in (v for v in VARIANTS if v["kind"] == "del"):
        assert dels.get((v["j"], v["pos"] + 1)) == v["n"], (v, dels)
    assert set(dels) == {(v["j"], v["pos"] + 1) for v in VARIANTS if v["kind"] == "del"} and set(dels.values()) == {1, 3}
    # the consensus of reference 2 over the bases of depth >= 4 is the sample's sequence
    sample, at = pc.consensus_truth()
    deep = p["depth"][2] >= pc.CONS_DEPTH
    assert deep.sum() >= len(deep) - 60
    want = "".join(c if deep[at[x]] else "N" for x, c in enumerate(sample))
    got = p["consensus"]
    lo = int(np.flatnonzero(deep)[0])
    assert len(got) == len(want) and got[lo:len(got) - 40] == want[lo:len(want) - 40], [(x, got[x], want[x]) for x in range(len(want)) if got[x] != want[x]][:5]
    assert all(a == b for a, b, d in zip(got, want, [deep[at[x]] for x in range(len(sample))]) if d)


def test_sam_fields_rebuild_the_reference_at_the_true_place():
    p = pc.expected_pile()
    rows, cigars, mds = p["sam"]
    w = p["w"]
    assert (rows[:, 0] >= 0).all()
    for q, r in enumerate(p["i"]):
        fr = FRAGS[r // 2]
        lo, hi, strand = fr["m1"] if r % 2 == 0 else fr["m2"]
        read = revcomp(READS[r]) if w["reverse"][q] else READS[r]
        pos, ref_len = int(rows[q, 0]), int(rows[q, 1])
        assert ref_from(read, cigars[q], mds[q]) == REFS[w["j"][q]][pos:pos + ref_len], (q, r, cigars[q], mds[q])
        if in_segment((lo, hi, strand), fr["j"]):
            continue       # (a read wholly inside the copied segment: its single-end place is one of two equal ones, by design)
        assert (int(w["j"][q]), int(w["reverse"][q]), pos - int(rows[q, 2])) == (fr["j"], strand, lo), (q, r, fr, pos, cigars[q])


def test_long_reads_find_their_loci():
    """chains(n=2) over the stride-4 index: every read's true locus lies inside a returned window on the right strand, and the
    adaptive alignment of that window completes with more than half of the span's bases matched, which no other place gives."""
    e = pc.expected_long()
    reads, origin = pc.long_reads()
    assert len(reads) == pc.NLONG and not e["chains"]["overflow"].any() and {o[3] for o in origin} == {0, 1}
    w = e["w"]
    for r, (j, pos, span, rev) in enumerate(origin):
        mine = np.flatnonzero(w["i"] == r)
        inside = [q for q in mine if w["j"][q] == j and w["reverse"][q] == rev and w["text_start"][q] <= pos and pos + span <= w["text_start"][q] + w["text_len"][q]]
        assert inside, (r, origin[r], [(int(w["j"][q]), int(w["text_start"][q]), int(w["text_len"][q])) for q in mine])
        assert e["status"][inside[0]] == 0 and 2 * e["summary"][inside[0], 0] > span, (r, e["summary"][inside[0]].tolist())


def test_the_three_hand_off_traps_occur():
    """What test_pipeline_gpu.py asserts on the device, on the expectation: a kept read whose primary is a rescue window, a kept read
    whose fragment's other mate is unplaced, and a piled-up window that `seeds` clipped at the start of reference 2 over the SNV."""
    res, p = pc.expected_placement(), pc.expected_pile()
    hit = res["reads"]["hit"]
    assert (hit[p["i"]] >= res["n0"]).sum() >= 30
    assert sum(1 for r in p["i"] if hit[r ^ 1] < 0) == pc.NORPHAN
    w = p["w"]
    assert ((w["j"] == 2) & (w["text_start"] == 0) & (w["text_len"] < pc.L + 2 * pc.PAD) & (w["text_len"] > 40)).sum() >= 4
