"""Left alignment on the GPU (wfa_hip_batch_left_align; left_align=True of align_windows, align_pairs and pileup): the device must return
exactly the Python restatement of the rule (leftalign_common) applied to the ORACLE's op strings, at the smallest shapes where the
kernel can go wrong — a run at either side of a 64-op round, shifts of more than one round, a run longer than a round, periods 1 to 3,
several runs of one pair, byte pairs beside 2-bit pairs, reversed windows, pairs that did not finish, a list cut into chunks, and the
merges of the one-component metrics — and the pileups, sites and insertion rows that follow from the rewritten strings."""
import ctypes
import json
import os

import numpy as np
import pytest

from calls_common import py_sites_all
from common import GOLD, configs_pair, rle
from leftalign_common import KW, METRICS, gpu_expectation, py_left_align
from oracle import loader
from pywfa_amd import WavefrontAligner, _native, datagen
from reduce_common import expected_tables, py_summary
from test_windows_gpu import as_list, cigars_of, materialise, native_set, native_windows

pytestmark = pytest.mark.gpu


def window_kw(W):
    return dict(i=W["i"], j=W["j"], pattern_start=W["p_start"], pattern_len=W["p_len"], text_start=W["t_start"], text_len=W["t_len"], reverse=W["reverse"])


def assert_strings(out, e, want, ctx):
    assert np.array_equal(out["score"], e["o"]["score"]) and np.array_equal(out["status"], e["o"]["status"]), ctx   # the scores stay WFA's
    for q, w in enumerate(want):
        got = bytes(out["cigar_ops"][q])
        assert got == w, (ctx, q, [k for k, v in e["names"].items() if v == q], rle(e["o"]["cigars"][q]), rle(w), rle(got))
        assert out["cigarstrings"][q] == rle(w), (ctx, q)


def first_gap(ops):
    return min(k for k in range(len(ops)) if ops[k] in b"ID")


def test_the_list_holds_the_shapes():
    """From the oracle's strings and the rule alone: the list is what the tests below say it is."""
    e = gpu_expectation()
    o, want, names = e["o"], e["want"], e["names"]
    assert (o["status"] == 0).all() and 200 <= len(want) <= 4000
    for start in (63, 64):                                   # a gap run that starts at op 63, and one at op 64
        for kind in "ID":
            q = names[f"round_{start}_{kind}"]
            assert first_gap(o["cigars"][q]) == start and first_gap(want[q][0]) == start - 8, (start, kind)
    for n in (65, 100, 130):                                 # shifts of 65 - 130 ops
        q = names[f"shift_{n}_D"]
        assert first_gap(o["cigars"][q]) - first_gap(want[q][0]) == n, n
    for name, kind in (("long_I", b"I"), ("long_D", b"D")):  # a run longer than 64, moved by more than 64
        q = names[name]
        assert kind * 70 in o["cigars"][q] and kind * 70 in want[q][0] and first_gap(o["cigars"][q]) - first_gap(want[q][0]) == 130
    assert sum(w[1] >= 2 for w in want) >= 20                # pairs with several runs that move
    assert sum(w[1] for w in want) > 200 and all(w[2] == 0 for w in want)
    assert e["W"]["reverse"].sum() > 50 and any("N" in p for p in e["pats"])
    for metric in ("levenshtein", "indel"):                  # the merges of the one-component metrics
        assert sum(w[2] > 0 for w in gpu_expectation(metric)["want"]) >= 20, metric


@pytest.mark.parametrize("metric", list(METRICS))
def test_align_windows_and_align_pairs(gpu, monkeypatch, metric):
    monkeypatch.delenv("WFA_HIP_PAIRS_BAND", raising=False)
    e = gpu_expectation(metric)
    want = [w[0] for w in e["want"]]
    wa = WavefrontAligner(**e["kw"])
    try:
        assert_strings(wa.align_windows(e["reads"], e["refs"], left_align=True, **window_kw(e["W"])), e, want, (metric, "windows"))
        idx = np.arange(len(want))
        assert_strings(wa.align_pairs(e["pats"], e["txts"], i=idx, j=idx, left_align=True), e, want, (metric, "pairs"))
        # without the keyword: what it returns today
        assert_strings(wa.align_windows(e["reads"], e["refs"], **window_kw(e["W"])), e, e["o"]["cigars"], (metric, "left_align=False"))
        assert_strings(wa.align_pairs(e["pats"], e["txts"], i=idx, j=idx, left_align=False), e, e["o"]["cigars"], (metric, "pairs, False"))
        # the summary of the rewritten strings
        s = wa.align_windows(e["reads"], e["refs"], summary=True, left_align=True, **window_kw(e["W"]))
        rows = np.stack([py_summary(w, len(p), len(t)) for w, p, t in zip(want, e["pats"], e["txts"])])
        got = np.column_stack([s["summary"][k] for k in ("M", "X", "I", "D", "I_runs", "D_runs")] + [s["summary"]["locations"]])
        assert np.array_equal(got, rows) and np.array_equal(s["score"], e["o"]["score"]), metric
        if metric != "affine":   # a merge shows in the run counts
            plain = wa.align_windows(e["reads"], e["refs"], summary=True, **window_kw(e["W"]))["summary"]
            assert (plain["I_runs"] + plain["D_runs"] > s["summary"]["I_runs"] + s["summary"]["D_runs"]).sum() >= 20
    finally:
        wa.close()


def test_chunks_and_pairs_that_did_not_finish(gpu, monkeypatch):
    """The list cut into chunks of 64 pairs (the run-length route), under a step limit that leaves some pairs unfinished: their bytes
    are the oracle's."""
    monkeypatch.setenv("WFA_HIP_PAIRS_BAND", "64")
    e = gpu_expectation("affine", 12)
    done = e["o"]["status"] == 0
    assert 20 <= done.sum() <= len(done) - 20 and sum(w[1] for w in e["want"]) >= 10
    want = [w[0] for w in e["want"]]
    wa = WavefrontAligner(**e["kw"])
    try:
        assert_strings(wa.align_windows(e["reads"], e["refs"], left_align=True, **window_kw(e["W"])), e, want, "chunks, max_steps")
    finally:
        wa.close()
    e = gpu_expectation("levenshtein")
    wa = WavefrontAligner(**e["kw"])
    try:
        assert_strings(wa.align_windows(e["reads"], e["refs"], left_align=True, **window_kw(e["W"])), e, [w[0] for w in e["want"]], "chunks")
    finally:
        wa.close()


def test_scope_score_is_refused(gpu):
    wa = WavefrontAligner(scope="score", **KW)
    try:
        for call in (lambda: wa.align_pairs(["ACGT"], ["ACGT"], i=[0], j=[0], left_align=True),
                     lambda: wa.align_windows(["ACGT"], ["ACGT"], i=[0], j=[0], left_align=True)):
            with pytest.raises(ValueError, match="needs scope='full'"):
                call()
        assert list(wa.align_pairs(["ACGT"], ["ACGT"], i=[0], j=[0])["score"]) == [0]
    finally:
        wa.close()


def test_pileup_counts(gpu):
    for metric in ("affine", "indel"):
        e = gpu_expectation(metric)
        W = e["W"]
        rewritten = dict(cigars=[w[0] for w in e["want"]], status=e["o"]["status"])
        lens = [len(r) for r in e["refs"]]
        tables, _ = expected_tables(lens, rewritten, e["pats"], W["j"], W["t_start"], W["t_len"])
        plain, _ = expected_tables(lens, e["o"], e["pats"], W["j"], W["t_start"], W["t_len"])
        assert any(not np.array_equal(a, b) for a, b in zip(tables, plain))
        wa = WavefrontAligner(**e["kw"])
        try:
            with wa.pileup(e["reads"], e["refs"], left_align=True, **window_kw(W)) as p, wa.pileup(e["reads"], e["refs"], **window_kw(W)) as q:
                for j in range(len(lens)):
                    assert np.array_equal(p.counts(j), tables[j]), (metric, j)
                    assert np.array_equal(q.counts(j), plain[j]), (metric, j)
                assert np.array_equal(p.score, e["o"]["score"])
        finally:
            wa.close()


# ---- what the feature is for: one site where the reads had several -------------------------------------------------------------------

LEFT = "TGCATCGATTCGAGCTAGCTTGACCGTATCGGATCCGTAGCTTGCAAGTCCGTTAGCGTC"     # 60 bases, no A at its end
RIGHT = "CTGGATCCTAGGCTTAGCGATCGTAGGCTAACGTTAGCGTTCAGGCTTAACGGATTCGCT"   # 60 bases, no A at its start


def test_a_deletion_in_a_homopolymer_is_one_site_at_its_first_base(gpu):
    """Twelve reads over a one-base deletion in A8 at [60, 68): seven plain ones, three with a substitution inside the run, two that end
    inside it."""
    ref = LEFT + "A" * 8 + RIGHT
    reads, rows = [], []

    def add(read, t0, t_len):
        rows.append((len(reads), 0, 0, len(read), t0, t_len, 0))
        reads.append(read)

    for k in range(7):
        add(LEFT[3 * k:] + "A" * 7 + RIGHT[:30 + 4 * k], 3 * k, 60 - 3 * k + 8 + 30 + 4 * k)
    for k, mid in enumerate(("AATAAAA", "AAAACAA", "AAAAAGA")):
        add(LEFT[5 + k:] + mid + RIGHT[:40 + k], 5 + k, 60 - 5 - k + 8 + 40 + k)
    for k, n in enumerate((3, 5)):                     # n As of the read against n + 1 of the run: the window ends inside the run
        add(LEFT[10 + k:] + "A" * n, 10 + k, 60 - 10 - k + n + 1)
    W = as_list(rows)
    pats, txts = materialise(reads, [ref], W)
    o = loader.run(loader.oracle(), loader.make_config(**KW), datagen.from_strings(pats, txts, upper=True))
    assert (o["status"] == 0).all()
    moved = dict(cigars=[py_left_align(ops, p.encode(), t.encode())[0] for ops, p, t in zip(o["cigars"], pats, txts)], status=o["status"])
    want = {}
    for name, res in (("left", moved), ("wfa", o)):
        tables, _ = expected_tables([len(ref)], res, pats, W["j"], W["t_start"], W["t_len"])
        want[name] = tables[0], py_sites_all(tables, [ref], 1, 500)
    # the rule puts every read that spans the run at the left of its own obstacle: the seven plain reads and whoever else reaches base 60
    assert want["left"][0][60, 5] >= 7 and want["left"][0][61:68, 5].max() <= 1 and want["wfa"][0][67, 5] >= 7
    wa = WavefrontAligner(**KW)
    try:
        with wa.pileup(reads, [ref], left_align=True, **window_kw(W)) as p, wa.pileup(reads, [ref], **window_kw(W)) as q:
            assert np.array_equal(p.counts(0), want["left"][0]) and np.array_equal(q.counts(0), want["wfa"][0])
            s, t = p.sites([ref]), q.sites([ref])
            for got, (_, rows_) in ((s, want["left"]), (t, want["wfa"])):
                assert np.array_equal(np.stack([got[k] for k in p.SITE_COLUMNS], axis=1), rows_)
            dels = lambda x: [(int(pos), int(n)) for pos, alt, n in zip(x["pos"], x["alt"], x["alt_count"]) if alt == 5]   # noqa: E731
            assert dels(s) == [(60, int(want["left"][0][60, 5]))]        # one `del` site, at the first A
            assert dels(t) == [(67, int(want["wfa"][0][67, 5]))]         # ... which WFA's own strings put at the last A
    finally:
        wa.close()


def test_an_inserted_unit_comes_out_in_front_of_the_repeat(gpu):
    ref = LEFT + "CA" * 5 + "G" + RIGHT
    reads, rows = [], []
    for k in range(8):
        read = LEFT[2 * k:] + "CA" * 6 + "G" + RIGHT[:20 + 3 * k]
        rows.append((k, 0, 0, len(read), 2 * k, len(read) - 2, 0))
        reads.append(read)
    W = as_list(rows)
    wa = WavefrontAligner(**KW)
    try:
        with wa.pileup(reads, [ref], insertions=True, left_align=True, **window_kw(W)) as p, \
                wa.pileup(reads, [ref], insertions=True, **window_kw(W)) as q:
            s, t = p.insertions([ref]), q.insertions([ref])
            assert (list(s["pos"]), list(s["ins_count"]), list(s["allele_count"]), s["seq"]) == ([60], [8], [8], ["CA"])
            assert (list(t["pos"]), t["seq"]) == ([70], ["CA"])
            spliced = LEFT + "CA" * 6 + "G" + RIGHT[:20]     # (over the bases every read covers)
            assert p.consensus([ref], 0, 0, 91, insertions=True) == spliced == q.consensus([ref], 0, 0, 91, insertions=True)
    finally:
        wa.close()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------

def test_c_abi_stats_second_call_and_a_new_run(gpu):
    e = gpu_expectation("levenshtein")
    n = len(e["want"])
    _, nc = configs_pair(**e["kw"])
    al = _native.Aligner(nc)
    try:
        ps, ts = native_set(al, e["reads"]), native_set(al, e["refs"])
        rb = native_windows(al, ps, ts, e["W"])
        rb.run()
        before = rb.rle()
        assert cigars_of(rb.results(True)[2], n) == e["o"]["cigars"]
        assert rb.left_align() == (sum(w[1] for w in e["want"]), sum(w[2] for w in e["want"]))
        first = rb.results(True)
        assert cigars_of(first[2], n) == [w[0] for w in e["want"]] and np.array_equal(first[0], e["o"]["score"])
        # the run-length encoding is made again from the rewritten strings
        off, code, rlen, locs = rb.rle()
        assert np.array_equal(locs, before[3]) and not (np.array_equal(off, before[0]) and np.array_equal(rlen, before[2]))
        chars = np.frombuffer(b"MIDNSHP=X", np.uint8)
        for q in range(n):
            assert np.repeat(chars[code[off[q]:off[q + 1]]], rlen[off[q]:off[q + 1]]).tobytes() == e["want"][q][0], q
        # a second call changes nothing and reports zeros
        assert rb.left_align() == (0, 0)
        second = rb.results(True)
        assert second[2][0].tobytes() == first[2][0].tobytes() and np.array_equal(second[2][1], first[2][1]) and np.array_equal(second[2][2], first[2][2])
        assert _native.lib().wfa_hip_batch_left_align(rb._h, None) == _native.OK      # stats is optional
        # a new run brings WFA's own strings back
        rb.run()
        assert cigars_of(rb.results(True)[2], n) == e["o"]["cigars"]
        empty = native_windows(al, ps, ts, {k: v[:0] for k, v in e["W"].items()})
        empty.run()
        assert empty.left_align() == (0, 0)
    finally:
        al.close()


def test_refusals(gpu):
    """tests/golden/leftalign_refusals.json: the code and wfa_hip_last_error of every refused call; the stats are not written."""
    with open(os.path.join(GOLD, "leftalign_refusals.json")) as f:
        golden = json.load(f)
    L = _native.lib()
    seqs = ["ACGTTGCATGCCATGA", "GATTACAGATTACA"]
    idx = np.arange(2, dtype=np.int32)
    handles = {}
    aligners = []
    for scope in ("score", "full"):
        _, nc = configs_pair(scope=scope, **KW)
        al = _native.Aligner(nc)
        aligners.append(al)
        s = native_set(al, seqs)
        handles[scope] = (al, al.batch_indexed(s, None, idx, idx))
    try:
        handles["score"][1].run()
        stats = np.full(2, -5, np.int64)
        calls = {"null batch": (None, None), "scope = score": handles["score"], "a batch that has not run": handles["full"]}
        assert [c["case"] for c in golden["cases"]] == list(calls) and golden["entry"] == "wfa_hip_batch_left_align"
        for c in golden["cases"]:
            al, rb = calls[c["case"]]
            assert L.wfa_hip_batch_left_align(rb._h if rb is not None else None, stats.ctypes.data) == c["rc"] == _native.EINVAL, c
            assert (stats == -5).all(), c
            if c["last_error"] is not None:
                assert al.error() == c["last_error"], c
        with pytest.raises(ValueError, match="left alignment needs a finished run"):
            handles["full"][1].left_align()
    finally:
        for al in aligners:
            al.close()
    assert ctypes.sizeof(ctypes.c_int64) == 8
