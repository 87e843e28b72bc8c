"""The SAM fields on the GPU (wfa_hip_batch_sam_counts / _sam_strings; sam=True of align_windows and align_pairs): the device must return
exactly the Python restatement of the rule (sam_common.py) applied to the ORACLE's op strings, at the smallest shapes where the kernels
can go wrong — strings of every length around one and two rounds of 64 ops, runs that end at, start at and cross a round, runs over
three rounds, numbers of one to four digits, clips and positions from free ends, byte pairs beside 2-bit pairs, reversed windows, pairs
that did not finish, pairs without an anchor, a list cut into chunks, and the strings a left alignment rewrote."""
import ctypes
import re

import numpy as np
import pytest

from common import configs_pair
from leftalign_common import expand
from pywfa_amd import WavefrontAligner, _native
from sam_common import CORE, EQX, FLAGS, KW, MAX_STEPS, MD_FORM, UNMAPPED, gpu_expectation, py_sam, ref_from
from test_windows_gpu import native_set, native_windows

pytestmark = pytest.mark.gpu

METRIC_NAMES = ("affine", "levenshtein", "indel")


def window_kw(W):
    return dict(i=W["i"], j=W["j"], pattern_start=W["p_start"], pattern_len=W["p_len"], text_start=W["t_start"], text_len=W["t_len"], reverse=W["reverse"])


def flag_kw(flags):
    return dict(sam=True, eqx=bool(flags & EQX), clip_mismatches=bool(flags & CORE))


def assert_sam(out, e, flags, ctx, t_start=None):
    """`out` of a sam=True call against the rule applied to the oracle's strings of `e`"""
    want = e["want"][flags]
    assert np.array_equal(out["score"], e["o"]["score"]) and np.array_equal(out["status"], e["o"]["status"]), ctx
    assert "cigar_ops" not in out and "cigarstrings" not in out, ctx
    s = out["sam"]
    assert sorted(s) == sorted(("pos", "ref_len", "clip_left", "clip_right", "nm", "query_len", "cigar", "md")), ctx
    assert len(s["cigar"]) == len(s["md"]) == len(want), ctx
    for q, (row, cigar, md) in enumerate(want):
        where = (ctx, q, [k for k, v in e["names"].items() if v == q], e["strings"][q])
        pos = row[0] + (int(t_start[q]) if t_start is not None and row[0] >= 0 else 0)
        got = tuple(int(s[k][q]) for k in ("pos", "ref_len", "clip_left", "clip_right", "nm", "query_len"))
        assert got == (pos, row[1], row[2], row[3], row[4], row[7]), where
        assert (s["cigar"][q], s["md"][q]) == (cigar.decode(), md.decode()), where


def runs_of(ops):
    """(letter, first op, last op) of the maximal runs"""
    return [(m.group(1), m.start(), m.end() - 1) for m in re.finditer(rb"(.)\1*", ops)]


def test_the_list_holds_the_shapes():
    """From the oracle's strings and the rule alone: the list is what the tests below say it is."""
    e = gpu_expectation()
    ops, names, want = e["strings"], e["names"], e["want"][0]
    assert (e["o"]["status"] == 0).all()
    free = gpu_expectation(part="free")
    assert (free["o"]["status"] == 0).all() and 200 <= len(ops) + len(free["strings"]) <= 4000
    for metric in METRIC_NAMES[1:]:
        assert (gpu_expectation(metric)["o"]["status"] == 0).all() and (gpu_expectation(metric, "free")["o"]["status"] == 0).all()
    assert {0, 1, 63, 64, 65, 127, 128, 129} <= {len(o) for o in ops}
    runs = [r for o in ops for r in runs_of(o)]
    for kind in (b"M", b"I", b"D"):
        ends = {last for c, first, last in runs if c == kind}
        assert {63, 64} <= ends, (kind, sorted(ends)[:40])                                       # a run that ends at op 63, one at op 64
        assert any(first <= 63 and last >= 64 for c, first, last in runs if c == kind), kind      # one that straddles 63 / 64
        assert any(last - first + 1 > 128 and first // 64 + 2 <= last // 64 for c, first, last in runs if c == kind), kind   # three rounds
    assert any(o[63:64] == b"X" for o in ops) and any(o[64:65] == b"X" for o in ops)
    assert any(b"XX" in o for o in ops) and any(re.search(rb"[^I]I+X", o) for o in ops)         # X X; X directly after an I run
    # WFA's backtrace never leaves an X in front of an I run, nor a D inside one: both arise when the left alignment (the Python rule on
    # the oracle's strings) moves a run up to an X or merges two runs around a D; test_left_align_then_sam_and_summary_beside_sam runs these strings
    assert any(re.search(rb"XI+[^I]", o) for o in gpu_expectation("affine", left_align=True)["strings"])   # X directly before an I run
    assert any(re.search(rb"I+DI+", o) for o in gpu_expectation("indel", left_align=True)["strings"])      # I run, D, I run
    assert any(o[:1] == b"X" for o in ops) and any(o[-1:] == b"X" for o in ops)                  # a span that starts / ends with X
    numbers = {int(n) for _, cigar, md in want for n in re.findall(rb"\d+", cigar + b" " + md)}
    md_numbers = {int(n) for _, _, md in want for n in re.findall(rb"\d+", md)}
    cigar_numbers = {int(n) for _, cigar, _ in want for n in re.findall(rb"\d+", cigar)}
    assert {9, 10, 99, 100, 999, 1000} <= md_numbers and {9, 10, 99, 100, 999, 1000, 1100} <= numbers, sorted(md_numbers)
    assert {9, 10, 99, 100, 999, 1000} <= {int(n) for _, cigar, _ in e["want"][EQX] for n in re.findall(rb"(\d+)=", cigar)}
    assert want[names["exact_1100"]] == ((0, 1100, 0, 0, 0, 5, 4, 1100), b"1100M", b"1100") and 1100 in cigar_numbers
    # the ends-free sub-list: leading and trailing I ops (pos > 0), leading and trailing D ops (soft clips on both sides)
    fo, fw = free["strings"], free["want"][0]
    assert sum(o[:1] == b"I" and o[-1:] == b"I" and w[0][0] > 0 for o, w in zip(fo, fw)) >= 3
    assert sum(o[:1] == b"D" and o[-1:] == b"D" and w[0][2] > 0 and w[0][3] > 0 for o, w in zip(fo, fw)) >= 3
    assert e["W"]["reverse"].sum() >= 50
    # the byte path: an N in the read, an N in the text under an X, an N in the text inside a deleted run
    pats, txts = e["pats"], e["txts"]
    assert sum("N" in p or "N" in t for p, t in zip(pats, txts)) >= 10 and sum("N" in p for p in pats) >= 2
    assert sum(b"N" in md and b"^" not in md for _, _, md in want) >= 2 and sum(bool(re.search(rb"\^[A-Z]*N", md)) for _, _, md in want) >= 2
    # pairs that do not finish: a copy under a step limit
    cut = gpu_expectation(max_steps=MAX_STEPS)
    assert (cut["o"]["status"] != 0).sum() >= 5 and (cut["o"]["status"] == 0).sum() >= 5
    assert all(w == UNMAPPED for w, st in zip(cut["want"][0], cut["o"]["status"]) if st != 0)
    # an empty pattern window, an empty text window, a pair with no M at all
    assert pats[names["empty_pattern"]] == "" and txts[names["empty_text"]] == "" and pats[names["len_0"]] == txts[names["len_0"]] == ""
    for name in ("empty_pattern", "empty_text", "len_0"):
        assert want[names[name]] == UNMAPPED, name
    q = names["all_x"]
    assert ops[q] == b"XXXX" and want[q] == ((0, 4, 0, 0, 4, 2, 9, 4), b"4M", b"0A0C0G0T0") and e["want"][CORE][q] == UNMAPPED
    # what the other three flag combinations change
    assert sum(a != b for a, b in zip(want, e["want"][EQX])) > 100 and sum(a != b for a, b in zip(want, e["want"][CORE])) >= 4


@pytest.mark.parametrize("metric", METRIC_NAMES)
def test_align_windows_and_align_pairs(gpu, monkeypatch, metric):
    monkeypatch.delenv("WFA_HIP_PAIRS_BAND", raising=False)
    for part in ("main", "free"):
        e = gpu_expectation(metric, part)
        idx = np.arange(len(e["pats"]))
        wa = WavefrontAligner(**e["kw"])
        try:
            for flags in FLAGS:
                out = wa.align_windows(e["reads"], e["refs"], **flag_kw(flags), **window_kw(e["W"]))
                assert_sam(out, e, flags, (metric, part, flags, "windows"), e["W"]["t_start"])
                assert_sam(wa.align_pairs(e["pats"], e["txts"], i=idx, j=idx, **flag_kw(flags)), e, flags, (metric, part, flags, "pairs"))
        finally:
            wa.close()


def test_the_device_output_rebuilds_the_reference(gpu):
    """For every mapped pair of the device's own output: read + CIGAR + MD give the reference string the test built."""
    for part in ("main", "free"):
        e = gpu_expectation("affine", part)
        W = e["W"]
        wa = WavefrontAligner(**e["kw"])
        try:
            for flags in FLAGS:
                s = wa.align_windows(e["reads"], e["refs"], **flag_kw(flags), **window_kw(W))["sam"]
                mapped = 0
                for q, read in enumerate(e["pats"]):
                    pos, ref_len = int(s["pos"][q]), int(s["ref_len"][q])
                    if pos < 0:
                        continue
                    assert s["clip_left"][q] + s["query_len"][q] + s["clip_right"][q] == len(read)
                    assert W["t_start"][q] <= pos and pos + ref_len <= W["t_start"][q] + W["t_len"][q]
                    assert MD_FORM.fullmatch(s["md"][q].encode()), (q, s["md"][q])
                    assert ref_from(read, s["cigar"][q], s["md"][q]) == e["refs"][W["j"][q]][pos:pos + ref_len], (part, flags, q)
                    mapped += 1
                assert mapped >= len(e["pats"]) - 4
        finally:
            wa.close()


def test_chunks_and_pairs_that_did_not_finish(gpu, monkeypatch):
    """The list cut into chunks of 37 pairs gives the same bytes; under a step limit the unfinished pairs are UNMAPPED."""
    monkeypatch.setenv("WFA_HIP_PAIRS_BAND", "37")
    for e in (gpu_expectation("levenshtein"), gpu_expectation(max_steps=MAX_STEPS)):
        wa = WavefrontAligner(**e["kw"])
        try:
            for flags in (0, EQX | CORE):
                out = wa.align_windows(e["reads"], e["refs"], **flag_kw(flags), **window_kw(e["W"]))
                assert_sam(out, e, flags, ("chunks", e["kw"], flags), e["W"]["t_start"])
        finally:
            wa.close()


def test_left_align_then_sam_and_summary_beside_sam(gpu, monkeypatch):
    monkeypatch.delenv("WFA_HIP_PAIRS_BAND", raising=False)
    for metric in ("affine", "indel"):
        e, plain = gpu_expectation(metric, left_align=True), gpu_expectation(metric)
        assert sum(a != b for a, b in zip(e["want"][0], plain["want"][0])) >= 20      # the rewrite shows in the fields
        wa = WavefrontAligner(**e["kw"])
        try:
            out = wa.align_windows(e["reads"], e["refs"], left_align=True, summary=True, sam=True, **window_kw(e["W"]))
            assert_sam(out, e, 0, (metric, "left_align"), e["W"]["t_start"])
            both = wa.align_windows(e["reads"], e["refs"], left_align=True, summary=True, **window_kw(e["W"]))
            assert sorted(out) == ["sam", "score", "status", "summary"] and sorted(both) == ["score", "status", "summary"]
            for k, v in both["summary"].items():
                assert np.array_equal(out["summary"][k], v), k
            idx = np.arange(len(e["pats"]))
            assert_sam(wa.align_pairs(e["pats"], e["txts"], i=idx, j=idx, left_align=True, sam=True, eqx=True), e, EQX, (metric, "pairs"))
        finally:
            wa.close()
    # the golden pair of the left-alignment tests: the library's 41M1I49M is a deletion from the reference in SAM
    left, right = "TGCATCGATTCGAGCTAGCTTGACCGTATCGGATCCGTAGC", "CTGGATCCTAGGCTTAGCGATCGTAGGCTAACGTTAGCGTTCAGGCTTA"
    text, read = left + "A" * 8 + right[:42], left + "A" * 7 + right[:42]
    wa = WavefrontAligner(**KW)
    try:
        ops = wa.align_pairs([read], [text], i=[0], j=[0], left_align=True)["cigarstrings"][0]
        assert ops == "41M1I49M"
        s = wa.align_pairs([read], [text], i=[0], j=[0], left_align=True, sam=True)["sam"]
        assert (s["cigar"][0], s["md"][0], int(s["nm"][0]), int(s["pos"][0])) == ("41M1D49M", "41^A49", 1, 0)
        assert (s["cigar"][0].encode(), s["md"][0].encode()) == py_sam(expand(ops), text.encode())[1:]
        plain = wa.align_pairs([read], [text], i=[0], j=[0], sam=True)["sam"]
        assert (plain["cigar"][0], plain["md"][0]) == ("48M1D42M", "48^A42")
    finally:
        wa.close()


def test_keys_without_sam_and_keyword_refusals(gpu):
    wa = WavefrontAligner(**KW)
    try:
        assert sorted(wa.align_pairs(["ACGT"], ["ACGT"], i=[0], j=[0])) == ["cigar_ops", "cigarstrings", "score", "status"]
        assert sorted(wa.align_windows(["ACGT"], ["ACGT"], i=[0], j=[0])) == ["cigar_ops", "cigarstrings", "score", "status"]
        assert sorted(wa.align_windows(["ACGT"], ["ACGT"], i=[0], j=[0], summary=True)) == ["score", "status", "summary"]
        for kw in (dict(eqx=True), dict(clip_mismatches=True)):
            for call in (wa.align_pairs, wa.align_windows):
                with pytest.raises(ValueError, match="needs sam=True"):
                    call(["ACGT"], ["ACGT"], i=[0], j=[0], **kw)
        empty = wa.align_pairs(["ACGT"], ["ACGT"], i=[], j=[], sam=True)
        assert len(empty["sam"]["cigar"]) == 0 and len(empty["sam"]["pos"]) == 0 and list(empty["sam"]["md"]) == []
    finally:
        wa.close()
    wa = WavefrontAligner(scope="score", **KW)
    try:
        for call in (wa.align_pairs, wa.align_windows):
            with pytest.raises(ValueError, match="sam=True needs scope='full'"):
                call(["ACGT"], ["ACGT"], i=[0], j=[0], sam=True)
    finally:
        wa.close()


def test_c_abi_two_steps_refusals_and_a_new_run(gpu):
    e = gpu_expectation("affine")
    n = len(e["pats"])
    want = e["want"][EQX]
    L = _native.lib()
    _, nc = configs_pair(**e["kw"])
    _, nc_score = configs_pair(scope="score", **KW)
    al, al_score = _native.Aligner(nc), _native.Aligner(nc_score)
    try:
        ps, ts = native_set(al, e["reads"]), native_set(al, e["refs"])
        rb = native_windows(al, ps, ts, e["W"])
        rows = np.full((n, 8), -9, np.int32)
        nbytes = np.full(2, -9, np.int64)
        blob = np.full(16, 0x2e, np.uint8)
        i64p = ctypes.POINTER(ctypes.c_int64)
        nc_p, nm_p = nbytes.ctypes.data_as(i64p), nbytes[1:].ctypes.data_as(i64p)
        counts = lambda flags=EQX: L.wfa_hip_batch_sam_counts(rb._h, flags, rows.ctypes.data, nc_p, nm_p)   # noqa: E731
        strings = lambda: L.wfa_hip_batch_sam_strings(rb._h, blob.ctypes.data, blob.ctypes.data)   # noqa: E731
        # refused, nothing written: a batch that has not run, strings before counts, unknown flags, missing outputs, scope score
        assert counts() == _native.EINVAL and "finished run" in al.error()
        rb.run()
        assert strings() == _native.EINVAL and "wfa_hip_batch_sam_counts first" in al.error()
        for flags in (4, 8 | EQX, -1):
            assert counts(flags) == _native.EINVAL and "flag" in al.error(), flags
        assert L.wfa_hip_batch_sam_counts(rb._h, 0, None, nc_p, nm_p) == _native.EINVAL
        assert L.wfa_hip_batch_sam_counts(rb._h, 0, rows.ctypes.data, None, nm_p) == _native.EINVAL
        assert L.wfa_hip_batch_sam_counts(None, 0, rows.ctypes.data, nc_p, nm_p) == _native.EINVAL
        assert L.wfa_hip_batch_sam_strings(None, blob.ctypes.data, blob.ctypes.data) == _native.EINVAL
        assert (rows == -9).all() and (nbytes == -9).all() and (blob == 0x2e).all()
        ss = native_set(al_score, ["ACGT"])
        rs = al_score.batch_indexed(ss, None, np.zeros(1, np.int32), np.zeros(1, np.int32))
        rs.run()
        assert L.wfa_hip_batch_sam_counts(rs._h, 0, rows.ctypes.data, nc_p, nm_p) == _native.EINVAL
        assert "scope=full" in al_score.error() and L.wfa_hip_batch_sam_strings(rs._h, blob.ctypes.data, blob.ctypes.data) == _native.EINVAL
        with pytest.raises(ValueError, match="needs scope=full"):
            rs.sam()
        # the two steps
        assert counts() == _native.OK
        assert [tuple(r) for r in rows.tolist()] == [w[0] for w in want]
        assert tuple(nbytes) == (sum(w[0][5] for w in want), sum(w[0][6] for w in want))
        cigar, md = np.full(nbytes[0] + 3, 0x2e, np.uint8), np.full(nbytes[1] + 3, 0x2e, np.uint8)
        assert L.wfa_hip_batch_sam_strings(rb._h, cigar.ctypes.data, md.ctypes.data) == _native.OK
        assert cigar.tobytes() == b"".join(w[1] for w in want) + b"..." and md.tobytes() == b"".join(w[2] for w in want) + b"..."
        assert rb.sam_kernel_ms() > 0
        # the wrapper; other flags; after a left alignment the rows are gone and come back from the rewritten strings
        for flags in FLAGS:
            r, c, m = rb.sam(flags)
            assert [tuple(x) for x in r.tolist()] == [w[0] for w in e["want"][flags]]
            assert c.tobytes() == b"".join(w[1] for w in e["want"][flags]) and m.tobytes() == b"".join(w[2] for w in e["want"][flags])
        rb.left_align()
        assert strings() == _native.EINVAL
        moved = gpu_expectation("affine", left_align=True)["want"][0]
        r, c, m = rb.sam()
        assert [tuple(x) for x in r.tolist()] == [w[0] for w in moved] and c.tobytes() == b"".join(w[1] for w in moved)
        # a new run: counts again
        rb.run()
        assert strings() == _native.EINVAL
        r, c, m = rb.sam(CORE)
        assert m.tobytes() == b"".join(w[2] for w in e["want"][CORE])
        # no pairs at all
        empty = native_windows(al, ps, ts, {k: v[:0] for k, v in e["W"].items()})
        empty.run()
        r, c, m = empty.sam()
        assert r.shape == (0, 8) and c.size == 0 and m.size == 0
    finally:
        al.close()
        al_score.close()
