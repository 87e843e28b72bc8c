"""Duplicates on unclipped ends and the representative by base quality, the part that needs no GPU: the new C entries are declared,
exported and bound; wfa_hip_duplicates_host_ex equals the Python restatement (dup_ends_common.py_duplicates_ex) on random cases in which
every new clause occurs, and wfa_hip_duplicates_host with flags 0; wfa_hip_ops_clips and wfa_hip_qsum_host against plain loops and on
hand cases; every refusal.  (tools/dup_host_check.cpp is the stand-alone program for the sanitizers.)"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from dup_common import as_arrays
from dup_ends_common import BY_QUALITY, CLIP_MAX, INT32_MAX, NEW_CLAUSES, UNCLIPPED, py_clips, py_duplicates_ex, py_qsum, random_ends_case
from pair_common import INT32_MIN
from pywfa_amd import _native

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRIES = ("wfa_hip_placer_add_hits_clips", "wfa_hip_placer_read_clips", "wfa_hip_ops_clips", "wfa_hip_placer_duplicates_ex",
           "wfa_hip_duplicates_host_ex", "wfa_hip_qsum_host")
PAR = dict(min_score=INT32_MIN, full_gap=24, min_insert=0, max_insert=1000, unpaired=0)
NO = [-1, 0, 0, 0]


def H(*hits):
    """A hit list from tuples (i, j, reverse, score, status, text_start, text_end)."""
    cols = list(zip(*hits)) if hits else [[]] * 7
    return dict(zip(("i", "j", "reverse", "score", "status", "text_start", "text_end"), cols))


def host(hits, nreads, mates, par, text_len, **ex):
    return _native.duplicates_host(nreads, *as_arrays(hits), mates, text_len, **par, **ex)


def test_header_binding_and_shim_declare_the_entries():
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", raw, flags=re.S))
    pxd = open(os.path.join(ROOT, "pywfa_amd", "cython_shim", "wfa_hip.pxd")).read()
    L = _native.lib()
    for name in ENTRIES:
        assert name + "(" in txt and name in _native.SYMBOLS and hasattr(L, name) and name + "(" in pxd, name
    assert "#define WFA_HIP_CLIP_MAX 65535 " in txt and "#define WFA_HIP_DUP_UNCLIPPED 1 " in txt and "#define WFA_HIP_DUP_BY_QUALITY 2 " in txt
    assert (_native.CLIP_MAX, _native.DUP_UNCLIPPED, _native.DUP_BY_QUALITY) == (CLIP_MAX, UNCLIPPED, BY_QUALITY) == (65535, 1, 2)
    place = raw[raw.index("---- placement:"):raw.index("---- pairing:")]
    assert "CLIPS." in place and "UNCLIPPED INTERVAL" in place and "us = ts - lead" in place
    dup = raw[raw.index("---- duplicates:"):raw.index("---- seed finder:")]
    for phrase in ("UNCLIPPED ENDS", "REPRESENTATIVE BY BASE QUALITY", "WHAT IT DOES NOT DO", "NOT MEASURED HERE"):
        assert phrase in dup, phrase
    assert "No unclipped coordinates: under scope full" not in dup            # the limitation this lifts is gone from the list
    assert L.wfa_hip_abi_version() == _native.ABI_VERSION == 4               # additive: the version stays
    import pywfa_amd
    for fn in (pywfa_amd.WavefrontAligner.place_pairs, pywfa_amd.WavefrontAligner.place_windows):
        par = inspect.signature(fn).parameters
        assert (par["dup_ends"].default, par["dup_qualities"].default, par["dup_min_quality"].default) == ("core", None, 15), fn
    par = inspect.signature(_native.Placer.duplicates).parameters
    assert (par["unclipped"].default, par["qualities"].default, par["min_quality"].default) == (False, None, 15)
    par = inspect.signature(_native.Placer.add_hits).parameters
    assert par["lead"].default is None and par["trail"].default is None and callable(_native.Placer.clips)


def test_host_statement_equals_the_restatement_on_random_cases():
    rng = np.random.default_rng(2031)
    seen = {}
    for k in range(2000):
        nreads, hits, mates, par, text_len, lead, trail, flags, qsum = random_ends_case(rng)
        assert nreads <= 64 and max(text_len) <= 256 and 0 <= lead.min(initial=0) and max(lead.max(initial=0), trail.max(initial=0)) <= 5
        q = qsum if flags & BY_QUALITY else None
        want_r, want_p = py_duplicates_ex(hits, nreads, mates, par, text_len, lead, trail, flags, q, seen)
        got_r, got_p = host(hits, nreads, mates, par, text_len, lead=lead, trail=trail, flags=flags, qsum=q)
        assert got_r.dtype == got_p.dtype == np.int32 and got_r.shape == want_r.shape and got_p.shape == want_p.shape, k
        assert np.array_equal(got_r, want_r) and np.array_equal(got_p, want_p), (k, flags, mates, par, text_len.tolist(), got_r.tolist(),
                                                                                 want_r.tolist(), got_p.tolist(), want_p.tolist())
        # flags 0, with or without clips: wfa_hip_duplicates_host byte for byte
        plain = host(hits, nreads, mates, par, text_len)
        for ex in (dict(flags=0), dict(lead=lead, trail=trail, flags=0), dict(lead=lead), dict(trail=trail)):
            again = host(hits, nreads, mates, par, text_len, **ex)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(plain, again)), (k, sorted(ex))
    # the generator itself: every new clause occurred somewhere
    assert set(seen) == set(NEW_CLAUSES) and all(seen[c] >= 5 for c in NEW_CLAUSES), sorted(seen.items())


def frag(f, ts, te, s1, s2):
    """Fragment f = reads (2 f, 2 f + 1): mate 1 forward from ts, mate 2 reverse up to te, 50 bases each."""
    return [(2 * f, 0, 0, s1, 0, ts, ts + 50), (2 * f + 1, 0, 1, s2, 0, te - 50, te)]


def test_edges_by_hand():
    for what in ("python", "host"):
        def run(hits, nreads, mates, text_len=(500,), **ex):
            if what == "python":
                r, p = py_duplicates_ex(hits, nreads, mates, PAR, list(text_len), ex.get("lead"), ex.get("trail"), ex.get("flags", 0), ex.get("qsum"))
            else:
                r, p = host(hits, nreads, mates, PAR, list(text_len), **ex)
            return r.tolist(), p.tolist()
        # a copy whose first base mismatches starts a base later: no group by core, one group unclipped; the better score represents it
        fwd = H((0, 0, 0, 0, 0, 100, 150), (1, 0, 0, -4, 0, 101, 150))
        assert run(fwd, 2, 0, lead=[0, 1]) == ([[0, 1, 0, 0], [1, 1, 0, 0]], []), what
        assert run(fwd, 2, 0, lead=[0, 1], flags=UNCLIPPED) == ([[0, 2, 0, 0], [0, 2, 1, 0]], []), what
        # ... and two reads with one core but different clips are a group by core only
        core = H((0, 0, 0, 0, 0, 100, 150), (1, 0, 0, -4, 0, 100, 150))
        assert run(core, 2, 0, lead=[0, 2], flags=0) == ([[0, 2, 0, 0], [0, 2, 1, 0]], []), what
        assert run(core, 2, 0, lead=[0, 2], flags=UNCLIPPED) == ([[0, 1, 0, 0], [1, 1, 0, 0]], []), what
        # reverse reads are joined through trail: p5 = te + trail - 1
        rev = H((0, 0, 1, 0, 0, 100, 150), (1, 0, 1, -4, 0, 110, 148))
        assert run(rev, 2, 0, trail=[0, 2], flags=UNCLIPPED) == ([[0, 2, 0, 0], [0, 2, 1, 0]], []), what
        assert run(rev, 2, 0, lead=[0, 2], flags=UNCLIPPED) == ([[0, 1, 0, 0], [1, 1, 0, 0]], []), what      # (a reverse read's lead plays no part)
        # pair units: lead of F and trail of R; trail of F and lead of R play no part
        two = H(*(frag(0, 100, 350, -4, -4) + frag(1, 101, 349, 0, 0)))
        assert run(two, 4, 2, lead=[0, 0, 1, 0], trail=[0, 0, 0, 1], flags=UNCLIPPED) == ([[-1, 0, 1, 0]] * 2 + [NO] * 2, [[1, 2, 1, 0], [1, 2, 0, 0]]), what
        assert run(two, 4, 2, lead=[0, 0, 0, 1], trail=[0, 0, 1, 0], flags=UNCLIPPED) == ([NO] * 4, [[0, 1, 0, 0], [1, 1, 0, 0]]), what
        assert run(two, 4, 2, lead=[0, 0, 1, 0], trail=[0, 0, 0, 1]) == ([NO] * 4, [[0, 1, 0, 0], [1, 1, 0, 0]]), what
        # b = -1 and b = tlen: alone with overflow 0, though two units share the place; b = 0 and b = tlen - 1 are inside
        edge = H((0, 0, 0, 0, 0, 0, 50), (1, 0, 0, 0, 0, 0, 50), (2, 0, 1, 0, 0, 450, 500), (3, 0, 1, 0, 0, 450, 500))
        assert run(edge, 4, 0, lead=[1, 1, 0, 0], trail=[0, 0, 1, 1], flags=UNCLIPPED) == ([[r, 1, 0, 0] for r in range(4)], []), what
        inside = H((0, 0, 0, 0, 0, 1, 50), (1, 0, 0, 0, 0, 0, 50), (2, 0, 1, 0, 0, 450, 499), (3, 0, 1, 0, 0, 450, 500))
        assert run(inside, 4, 0, lead=[1, 0, 0, 0], trail=[0, 0, 1, 0], flags=UNCLIPPED) == ([[0, 2, 0, 0], [0, 2, 1, 0], [2, 2, 0, 0], [2, 2, 1, 0]], []), what
        # clips saturate at 65 535: 65 535 and 65 536 are one value, 65 534 another
        far = H((0, 0, 0, 0, 0, 70000, 70050), (1, 0, 0, 0, 0, 70000, 70050), (2, 0, 0, 0, 0, 70000, 70050))
        assert run(far, 3, 0, (80000,), lead=[65535, 65536, 65534], flags=UNCLIPPED) == ([[0, 2, 0, 0], [0, 2, 1, 0], [2, 1, 0, 0]], []), what
        # a pair unit whose unclipped end does not fit int32: alone, its mates are no units
        huge = H(*[(2 * f + m, 0, m, 0, 0, 100 if m == 0 else INT32_MAX - 50, 150 if m == 0 else INT32_MAX) for f in range(2) for m in range(2)])
        big = dict(PAR, max_insert=INT32_MAX)
        for flags, want in ((0, [[0, 2, 0, 0], [0, 2, 1, 0]]), (UNCLIPPED, [[0, 1, 0, 0], [1, 1, 0, 0]])):
            if what == "python":
                got = py_duplicates_ex(huge, 4, 2, big, [500], None, [0, 1, 0, 1], flags)[1].tolist()
            else:
                got = host(huge, 4, 2, big, [500], trail=[0, 1, 0, 1], flags=flags)[1].tolist()
            assert got == want, (what, flags)
        # by quality: the representative is the unit of the greatest sum, a pair unit's sum is that of its two mates; ties: the number
        assert run(two, 4, 2, lead=[0, 0, 1, 0], trail=[0, 0, 0, 1], flags=3, qsum=[900, 900, 1000, 700]) == \
            ([NO] * 2 + [[-1, 0, 1, 0]] * 2, [[0, 2, 0, 0], [0, 2, 1, 0]]), what
        assert run(core, 2, 0, flags=BY_QUALITY, qsum=[10, 11]) == ([[1, 2, 1, 0], [1, 2, 0, 0]], []), what
        assert run(core, 2, 0, flags=BY_QUALITY, qsum=[11, 11]) == ([[0, 2, 0, 0], [0, 2, 1, 0]], []), what
        sat = H(*(frag(0, 100, 350, -4, -4) + frag(1, 100, 350, 0, 0)))
        assert run(sat, 4, 2, flags=BY_QUALITY, qsum=[INT32_MAX, 5, INT32_MAX, INT32_MAX]) == ([NO] * 2 + [[-1, 0, 1, 0]] * 2, [[0, 2, 0, 0], [0, 2, 1, 0]]), what


def test_ops_clips_against_a_loop():
    for ops, plen, tlen, want in ((b"XM", 2, 2, (1, 0)), (b"DXM", 3, 2, (2, 0)), (b"MX", 2, 2, (0, 1)), (b"MDD", 3, 1, (0, 2)), (b"XXDI", 3, 3, (0, 0)),
                                  (b"", 0, 0, (0, 0)), (b"IIXMIMDXI", 5, 7, (1, 2)), (b"M", 1, 1, (0, 0)), (b"XM", 0, 2, (0, 0)), (b"XM", 2, 0, (0, 0)),
                                  (b"D" * 65535 + b"M", 65536, 1, (65535, 0)), (b"D" * 65536 + b"M", 65537, 1, (65535, 0)),
                                  (b"M" + b"X" * 65534, 65535, 65535, (0, 65534)), (b"M" + b"X" * 70000, 70001, 70001, (0, 65535))):
        assert _native.ops_clips(ops, plen, tlen) == want == py_clips(ops, plen, tlen), ops[:12]
    rng = np.random.default_rng(3)
    letters = np.frombuffer(b"MXID", np.uint8)
    for k in range(2000):
        n = int(rng.integers(0, 40))
        ops = letters[rng.choice(4, n, p=[0.25, 0.3, 0.2, 0.25] if k % 2 else [0.02, 0.4, 0.28, 0.3])]
        plen, tlen = int(np.isin(ops, [77, 88, 68]).sum()), int(np.isin(ops, [77, 88, 73]).sum())
        assert _native.ops_clips(ops, plen, tlen) == py_clips(ops.tobytes(), plen, tlen), ops.tobytes()
    L = _native.lib()
    a, b = ctypes.c_int32(7), ctypes.c_int32(7)
    x = np.frombuffer(b"XM", np.uint8)
    for args in ((x.ctypes.data, 2, 2, 2, None, ctypes.byref(b)), (x.ctypes.data, 2, 2, 2, ctypes.byref(a), None), (None, 2, 2, 2, ctypes.byref(a), ctypes.byref(b)),
                 (x.ctypes.data, -1, 2, 2, ctypes.byref(a), ctypes.byref(b)), (x.ctypes.data, 2, -1, 2, ctypes.byref(a), ctypes.byref(b)),
                 (x.ctypes.data, 2, 2, -1, ctypes.byref(a), ctypes.byref(b))):
        assert L.wfa_hip_ops_clips(*args) == _native.EINVAL and (a.value, b.value) == (7, 7), args[1:4]


def test_qsum_host():
    rng = np.random.default_rng(4)
    for n in (0, 1, 15, 16, 17, 100, 1000):
        q = rng.integers(0, 94, n).astype(np.uint8)
        for minq in (0, 15, 93):
            assert _native.qsum_host(q, minq) == py_qsum(q, minq) == int(q[q >= minq].astype(np.int64).sum()), (n, minq)
    assert _native.qsum_host(np.array([14, 15, 16, 93], np.uint8)) == 124                     # (the default threshold is 15)
    # saturation: 93 * 24 000 000 is above 2^31 - 1; one byte less than the bound is exact
    long = np.full(24_000_000, 93, np.uint8)
    assert 93 * long.size > INT32_MAX and _native.qsum_host(long, 0) == INT32_MAX
    assert _native.qsum_host(long[:INT32_MAX // 93], 93) == 93 * (INT32_MAX // 93)
    assert _native.qsum_host(long[:INT32_MAX // 93 + 1], 93) == INT32_MAX
    for bad in (94, -1, 1000):
        with pytest.raises(ValueError, match="min_quality"):
            _native.qsum_host(long[:4], bad)
    L = _native.lib()
    out = ctypes.c_int32(7)
    assert L.wfa_hip_qsum_host(long.ctypes.data, 4, 15, None) == _native.EINVAL
    assert L.wfa_hip_qsum_host(None, 4, 15, ctypes.byref(out)) == _native.EINVAL and L.wfa_hip_qsum_host(long.ctypes.data, -1, 15, ctypes.byref(out)) == _native.EINVAL
    assert L.wfa_hip_qsum_host(long.ctypes.data, 4, 94, ctypes.byref(out)) == _native.EINVAL and out.value == 7
    assert L.wfa_hip_qsum_host(None, 0, 15, ctypes.byref(out)) == _native.OK and out.value == 0


def test_refusals_leave_the_outputs_untouched():
    ok = H((0, 0, 0, 0, 0, 100, 150), (1, 0, 0, -4, 0, 101, 150))

    def call(**ex):
        return host(ok, 2, 0, PAR, [500], **ex)

    assert call(lead=[0, 1], flags=1)[0].tolist() == [[0, 2, 0, 0], [0, 2, 1, 0]]
    for ex, msg in ((dict(flags=4), r"flags = 4: an unknown flag bit"), (dict(flags=-1), r"an unknown flag bit"),
                    (dict(flags=2), r"flags = 2: WFA_HIP_DUP_BY_QUALITY without qualities"), (dict(flags=3), r"without qualities"),
                    (dict(flags=0, qsum=[1, 2]), r"flags = 0: qualities without WFA_HIP_DUP_BY_QUALITY"), (dict(flags=1, qsum=[1, 2]), r"qualities without"),
                    (dict(flags=2, qsum=[1, -2]), r"a negative quality sum of read 1: qsum = -2"),
                    (dict(lead=[0, -1], flags=1), r"a negative clip at position 1 of the hit list: lead = -1, trail = 0"),
                    (dict(trail=[-3, 0]), r"a negative clip at position 0 of the hit list: lead = 0, trail = -3"),
                    (dict(lead=[0]), r"lead: one value per hit \(2\)"), (dict(flags=2, qsum=[1]), r"qsum: one value per read \(2\)")):
        with pytest.raises(ValueError, match=msg):
            call(**ex)
    # straight at the C entry: nothing is written; what wfa_hip_duplicates_host refuses is refused here too
    L = _native.lib()
    arrays = as_arrays(ok)
    ptrs = [a.ctypes.data for a in arrays]
    tlen = np.array([500], np.int32)
    reads = np.full((2, 4), 7, np.int32)
    neg, q = np.array([0, -1], np.int32), np.array([5, 5], np.int32)
    msg = ctypes.create_string_buffer(256)

    def raw(lead=None, trail=None, flags=0, qsum=None, ntexts=1, full_gap=24, reads_p=reads.ctypes.data):
        return L.wfa_hip_duplicates_host_ex(2, 2, *ptrs, INT32_MIN, full_gap, 0, 1000, 0, 0, None, None, ntexts, tlen.ctypes.data, reads_p, None,
                                            lead, trail, flags, qsum, msg, 256)

    for kw in (dict(flags=8), dict(flags=2), dict(qsum=q.ctypes.data), dict(lead=neg.ctypes.data), dict(trail=neg.ctypes.data), dict(ntexts=0),
               dict(full_gap=0), dict(reads_p=None), dict(flags=2, qsum=neg.ctypes.data)):
        assert raw(**kw) == _native.EINVAL and msg.value, kw
    assert (reads == 7).all()
    assert raw(flags=2, qsum=q.ctypes.data) == _native.OK and msg.value == b"" and reads.tolist() == [[0, 1, 0, 0], [1, 1, 0, 0]]
    assert L.wfa_hip_duplicates_host_ex(2, 2, *ptrs, INT32_MIN, 24, 0, 1000, 0, 0, None, None, 1, tlen.ctypes.data, reads.ctypes.data, None, None, None, 4,
                                        None, None, 0) == _native.EINVAL                      # (a message buffer is optional)
