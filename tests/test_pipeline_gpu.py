"""The paired-read pipeline of the README on the GPU, every option on, against the composed plain reference of pipeline_common: exact
equality, array by array and string by string, at every call — seeds, place_pairs (rescue, duplicates on unclipped ends, the
representative by base quality), the pileup with its five tracks and every reduction of it, and the SAM fields.  The device's outputs
are handed from call to call exactly as a user hands them on (pipeline_common.windows_of_seeds, kept_reads, primaries); the expectation
never sees a device output."""
import numpy as np
import pytest

import pipeline_common as pc
from pywfa_amd import WavefrontAligner
from pywfa_amd.align import Pileup

pytestmark = pytest.mark.gpu

REFS = pc.genome()[0]
READS = list(pc.corpus()[0])
# what this module hands the oracle (through pipeline_common): tests/oracle_configs.py pins the oracle to the real library on them
ORACLE_KWS = [pc.kw_of(), pc.kw_of(rescue=True), pc.KW_LONG]
HOW = dict(min_insert=pc.MIN_INSERT, max_insert=pc.MAX_INSERT, rescue=True, duplicates=True, dup_ends="unclipped")


def same(got, want, ctx):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    assert bad.size == 0, (ctx, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist(), bad.size)


def same_columns(got, rows, names, ctx):
    assert tuple(got)[:len(names)] == tuple(names), (ctx, tuple(got))
    for c, name in enumerate(names):
        assert got[name].dtype == np.int32, (ctx, name)
        same(got[name], rows[:, c], (ctx, name))


def run_pipeline(wa, R, G, Q, idx):
    """The README's pipeline on the device, asserted against the expectation at every call; returns the bytes of everything it got."""
    seen = []

    def keep(x):
        seen.append(np.ascontiguousarray(x).tobytes() if not isinstance(x, (str, list, tuple)) else repr(x).encode())
        return x

    s = idx.seeds(R, n=pc.NSEEDS)
    want = pc.expected_seeds()
    for k in want:
        assert s[k].dtype == want[k].dtype, k
        same(keep(s[k]), want[k], ("seeds", k))
    w = pc.without_dropped(pc.windows_of_seeds(s))
    res = wa.place_pairs(R, G, dup_qualities=Q, **HOW, **w)
    e = pc.expected_placement()
    n0 = len(w["i"])
    assert n0 == e["n0"] and tuple(res) == ("score", "status", "flag", "reads", "pair_flag", "pairs", "rescue")
    for k in ("score", "status", "flag", "pair_flag"):
        same(keep(res[k]), e[k], ("place_pairs", k))
    for part in ("reads", "pairs", "rescue"):
        assert set(res[part]) == set(e[part]), (part, set(res[part]) ^ set(e[part]))
        for k in res[part]:
            assert res[part][k].dtype == np.int32, (part, k)
            same(keep(res[part][k]), e[part][k], ("place_pairs", part, k))
    i = pc.kept_reads(res["reads"])
    pw = pc.primaries(w, res, i)
    p = pc.expected_pile()
    with wa.pileup(R, G, left_align=True, insertions=True, deletions=True, strands=True, qualities=Q, min_base_quality=pc.MBQ, **pw) as pile:
        same(keep(pile.score), p["score"], "pileup score")
        same(keep(pile.status), p["status"], "pileup status")
        for j in range(len(REFS)):
            same(keep(pile.counts(j)), p["counts"][j], ("counts", j))
            same(keep(pile.depth(j)), p["depth"][j], ("depth", j))
            same(keep(pile.counts(j, strand="+")), p["fwd"][j], ("forward counts", j))
            same(keep(pile.quality_sums(j)), p["qsums"][j], ("quality sums", j))
            same(keep(pile.deletion_starts(j)), p["starts"][j], ("deletion starts", j))
        d, f, eq, strand = pc.GENO_Q
        same_columns(pile.genotypes(G, min_depth=d, min_frac=f / 1000, qualities=True), p["geno_q"], Pileup.GENOTYPE_COLUMNS, "genotypes by quality")
        d, f, eq, strand = pc.GENO_STRAND
        same_columns(pile.genotypes(G, min_depth=d, min_frac=f / 1000, min_alt_strand=strand), p["geno_strand"], Pileup.GENOTYPE_COLUMNS, "genotypes by strand")
        same_columns(pile.sites(G, min_depth=pc.SITES[0], min_frac=pc.SITES[1] / 1000), p["sites"], Pileup.SITE_COLUMNS, "sites")
        ins = pile.insertions(G, min_depth=pc.INDELS[0], min_frac=pc.INDELS[1] / 1000)
        same_columns(ins, p["insertions"][0], Pileup.INSERTION_COLUMNS, "insertions")
        assert tuple(keep(ins["seq"])) == p["insertions"][1]
        same_columns(pile.deletions(G, min_depth=pc.INDELS[0], min_frac=pc.INDELS[1] / 1000), p["deletions"], Pileup.DELETION_COLUMNS, "deletions")
        assert keep(pile.consensus(G, 2, min_depth=pc.CONS_DEPTH, insertions=True)) == p["consensus"]
    sam = wa.align_windows(R, G, left_align=True, sam=True, **pw)["sam"]
    rows, cigars, mds = p["sam"]
    for name, c in (("pos", 0), ("ref_len", 1), ("clip_left", 2), ("clip_right", 3), ("nm", 4), ("query_len", 7)):
        assert sam[name].dtype == np.int32
        same(keep(sam[name]), rows[:, c], ("sam", name))
    assert keep(list(sam["cigar"])) == cigars and keep(list(sam["md"])) == mds
    return b"".join(seen), w, res, i, pw


@pytest.fixture()
def aligner(gpu):
    wa = WavefrontAligner(**pc.KW)
    yield wa
    wa.close()


def with_handles(wa):
    with wa.sequence_set(READS) as R, wa.sequence_set(REFS) as G, wa.quality_set(R, pc.fastq_quals()) as Q, wa.seed_index(G, k=pc.K) as idx:
        return run_pipeline(wa, R, G, Q, idx)


def test_handles_held_open_and_the_three_hand_off_traps(aligner):
    _, w, res, i, pw = with_handles(aligner)
    n0, hit = len(w["i"]), res["reads"]["hit"]
    # a primary that is a rescue window is piled up from res["rescue"], not from the caller's list
    rescued = np.flatnonzero(hit[i] >= n0)
    assert rescued.size >= 30
    q = hit[i][rescued] - n0
    assert np.array_equal(pw["j"][rescued], res["rescue"]["j"][q]) and np.array_equal(pw["reverse"][rescued], res["rescue"]["reverse"][q])
    assert np.array_equal(pw["i"][rescued], res["rescue"]["i"][q]) and (pw["text_start"][rescued] >= res["rescue"]["text_start"][q]).all()
    # a read kept by dup == 0 whose fragment's other mate is unplaced
    assert sum(1 for r in i if hit[r ^ 1] < 0) == pc.NORPHAN
    # a window that seeds clipped at the start of reference 2, over the SNV at base 40
    assert ((pw["j"] == 2) & (pw["text_start"] == 0) & (pw["text_len"] < pc.L + 2 * pc.PAD) & (pw["text_len"] > 40)).sum() >= 4


def test_lists_of_str(aligner):
    with aligner.seed_index(REFS, k=pc.K) as idx:
        run_pipeline(aligner, READS, REFS, pc.fastq_quals(), idx)


def test_chunked_lists(aligner, monkeypatch):
    """Groups and buckets straddle the chunks: several placer adds, several pileup adds."""
    monkeypatch.setenv("WFA_HIP_PAIRS_BAND", "97")
    monkeypatch.setenv("WFA_HIP_CALLS_CHUNK", "64")
    with_handles(aligner)


def test_twice_on_one_aligner_gives_the_same_bytes(aligner):
    first = with_handles(aligner)[0]
    assert with_handles(aligner)[0] == first


def test_long_reads_chains_to_adaptive_windows(gpu):
    """seed_index(stride=4) -> chains(n=2) -> align_windows(heuristic="adaptive", summary=True), against chain_common.py_chains and the
    oracle under the same heuristic."""
    e = pc.expected_long()
    reads = list(pc.long_reads()[0])
    wa = WavefrontAligner(**pc.KW_LONG)
    try:
        with wa.sequence_set(reads) as R, wa.sequence_set(REFS) as G, wa.seed_index(G, k=pc.K, stride=pc.LONG_STRIDE) as idx:
            c = idx.chains(R, n=pc.LONG_N)
            for k, want in e["chains"].items():
                assert c[k].dtype == want.dtype, k
                same(c[k], want, ("chains", k))
            w = pc.windows_of_chains(c)
            out = wa.align_windows(R, G, summary=True, **w)
        same(out["score"], e["score"], "score")
        same(out["status"], e["status"], "status")
        ok = e["status"] == 0
        for c_, name in enumerate(("M", "X", "I", "D", "I_runs", "D_runs")):
            same(out["summary"][name][ok], e["summary"][ok, c_], ("summary", name))
        same(out["summary"]["locations"][ok], e["summary"][ok, 6:], "locations")
    finally:
        wa.close()
