"""Calls and sites of a pileup on the GPU (wfa_hip_pileup_calls / _sites, Pileup.calls / consensus / sites): the device must equal the
Python restatement of the rule (calls_common) applied to the tables built from the ORACLE's op strings — never to the device's own
counts() — exactly: through the C ABI with the sites' chunk at 64, 192 and its default, over ranges, capacities and parameters, after
a clear, after two adds, with the set reopened; the refusals; and from Python with handles and with lists."""
import ctypes

import numpy as np
import pytest

from calls_common import KW, expectation, expected_calls, expected_sites, py_calls, py_sites_all
from common import configs_pair
from pywfa_amd import WavefrontAligner, _native
from test_windows_gpu import native_set, native_windows

FILL = -7


class Rig:
    """An aligner, the two sets and a pileup of the corpus at the C ABI binding; `parts`: the list added in that many pieces."""

    def __init__(self, parts=1):
        e = expectation()
        self.e = e
        _, nc = configs_pair(**KW)
        self.al = _native.Aligner(nc)
        self.ps, self.ts = native_set(self.al, e["reads"]), native_set(self.al, e["refs"])
        self.pile = self.al.pileup(self.ts)
        n = len(e["W"]["i"])
        cuts = [n * k // parts for k in range(parts + 1)]
        self.batches = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = {k: v[lo:hi] for k, v in e["W"].items()}
            rb = native_windows(self.al, self.ps, self.ts, part)
            rb.run()
            self.pile.add(rb, part["j"], part["t_start"])
            self.batches.append((rb, part))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.al.close()
        return False

    def sites(self, seq=-1, start=0, length=-1, md=1, pm=500, cap=None, ts=None):
        """wfa_hip_pileup_sites on rows prefilled with FILL: (count, rows); cap None: the counting call first."""
        ts = self.ts if ts is None else ts
        count = ctypes.c_int64(-1)
        L = _native.lib()
        if cap is None:
            assert L.wfa_hip_pileup_sites(self.pile._h, ts._h, seq, start, length, md, pm, 0, ctypes.byref(count), None) == _native.OK, self.al.error()
            cap = count.value
        rows = np.full((cap, 8), FILL, np.int32)
        rc = L.wfa_hip_pileup_sites(self.pile._h, ts._h, seq, start, length, md, pm, cap, ctypes.byref(count), rows.ctypes.data if cap else None)
        assert rc == _native.OK, self.al.error()
        return count.value, rows


def in_range(rows, seq, start, length):
    return rows[(rows[:, 0] == seq) & (rows[:, 1] >= start) & (rows[:, 1] < start + length)]


RANGES = [(0, 13, 1000), (2, 1001, 2333), (3, 1999, 103), (1, 1960, 500), (4, 5, 30), (4, 0, 41), (1, 4500, 0), (3, 0, 0), (5, 0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", ["64", "192", None])
def test_c_abi_over_chunks_ranges_and_capacities(gpu, monkeypatch, chunk):
    """17 kb of references are one chunk's worth five times over at the default, tens of chunks at 192, hundreds at 64 (two rounds of
    the scan)."""
    if chunk is None:
        monkeypatch.delenv("WFA_HIP_CALLS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("WFA_HIP_CALLS_CHUNK", chunk)
    want, calls = expected_sites(1, 500), expected_calls(1)
    with Rig() as rig:
        for j, c in enumerate(calls):
            got = rig.pile.calls(rig.ts, j)
            assert got.dtype == np.uint8 and np.array_equal(got, c), (j, np.flatnonzero(got != c)[:5])
        count, rows = rig.sites()
        assert count == len(want) and np.array_equal(rows, want), (count, len(want))
        again = rig.sites()
        assert again[0] == count and np.array_equal(again[1], rows)                       # two calls, identical rows
        for seq, start, length in RANGES:
            assert np.array_equal(rig.pile.calls(rig.ts, seq, start, length), calls[seq][start:start + length]), (seq, start, length)
            count, rows = rig.sites(seq, start, length)
            w = in_range(want, seq, start, length)
            assert count == len(w) and np.array_equal(rows, w), (seq, start, length, count, len(w))
        n = len(want)
        for cap in (0, n - 1, n, n + 5):
            count, rows = rig.sites(cap=cap)
            k = min(cap, n)
            assert count == n and np.array_equal(rows[:k], want[:k]) and (rows[k:] == FILL).all(), cap
        w = in_range(want, 2, 1001, 2333)
        count, rows = rig.sites(2, 1001, 2333, cap=3)
        assert count == len(w) > 3 and np.array_equal(rows, w[:3])


@pytest.mark.gpu
def test_parameter_cross(gpu, monkeypatch):
    monkeypatch.setenv("WFA_HIP_CALLS_CHUNK", "192")
    with Rig() as rig:
        for md in (1, 8):
            for j, c in enumerate(expected_calls(md)):
                assert np.array_equal(rig.pile.calls(rig.ts, j, min_depth=md), c), (md, j)
            for pm in (200, 500, 1000):
                want = expected_sites(md, pm)
                count, rows = rig.sites(md=md, pm=pm)
                assert count == len(want) and np.array_equal(rows, want), (md, pm, count, len(want))
        # a depth nothing reaches: no site, every base a no-call
        big = 2**31 - 1
        count, rows = rig.sites(md=big, cap=4)
        assert count == 0 and (rows == FILL).all()
        for j, ref in enumerate(rig.e["refs"]):
            assert (rig.pile.calls(rig.ts, j, min_depth=big) == 6).all() and len(rig.pile.calls(rig.ts, j, min_depth=big)) == len(ref)


@pytest.mark.gpu
def test_two_adds_a_clear_and_a_reopened_set(gpu, monkeypatch):
    monkeypatch.setenv("WFA_HIP_CALLS_CHUNK", "64")
    with Rig(parts=2) as rig:
        e = rig.e
        want = expected_sites(1, 500)
        count, rows = rig.sites()
        assert count == len(want) and np.array_equal(rows, want)
        # the set closed, and opened again from the same strings: the pileup keeps no letters of its own
        rig.ts.close()
        again = native_set(rig.al, e["refs"])
        count, rows = rig.sites(ts=again)
        assert count == len(want) and np.array_equal(rows, want)
        assert np.array_equal(rig.pile.calls(again, 3), expected_calls(1)[3])
        # cleared: nothing is covered
        rig.pile.clear()
        count, rows = rig.sites(ts=again, cap=4)
        assert count == 0 and (rows == FILL).all()
        for j in range(len(e["refs"])):
            assert (rig.pile.calls(again, j) == 6).all()
        # the first half once, the second half twice: integer adds, the expectation from the oracle's tables of the halves
        from reduce_common import expected_tables
        from test_windows_gpu import materialise
        pats, _ = materialise(e["reads"], e["refs"], e["W"])
        n = len(pats)
        second = np.arange(n) >= n // 2
        lens = [len(r) for r in e["refs"]]
        twice, _ = expected_tables(lens, e["o"], pats, e["W"]["j"], e["W"]["t_start"], e["W"]["t_len"], second)
        tables = [a + b for a, b in zip(e["tables"], twice)]
        for k in (1, 0, 1):
            rb, part = rig.batches[k]
            rig.pile.add(rb, part["j"], part["t_start"])
        want = py_sites_all(tables, e["refs"], 8, 200)
        count, rows = rig.sites(md=8, pm=200, ts=again)
        assert count == len(want) and np.array_equal(rows, want)
        assert len(want) != len(expected_sites(8, 200))
        assert np.array_equal(rig.pile.calls(again, 0, min_depth=8), py_calls(tables[0], e["refs"][0].encode(), 8))


@pytest.mark.gpu
def test_refusals_write_nothing(gpu):
    with Rig() as rig:
        e, L, pile, ts = rig.e, _native.lib(), rig.pile, rig.ts
        _, nc = configs_pair(**KW)
        al2 = _native.Aligner(nc)
        try:
            out = np.full(64, 99, np.uint8)
            rows = np.full((4, 8), FILL, np.int32)
            count = ctypes.c_int64(-1)

            def calls(tset, seq, start, length, md, outp=out.ctypes.data):
                return L.wfa_hip_pileup_calls(pile._h, tset._h, seq, start, length, md, outp)

            def sites(tset, seq, start, length, md, pm, cap, cnt=ctypes.byref(count), rowp=rows.ctypes.data):
                return L.wfa_hip_pileup_sites(pile._h, tset._h, seq, start, length, md, pm, cap, cnt, rowp)

            def refused(rc, pattern):
                assert rc == _native.EINVAL and pattern in rig.al.error(), (rc, rig.al.error())
                assert (out == 99).all() and (rows == FILL).all() and count.value == -1

            foreign = native_set(al2, e["refs"])
            refused(calls(foreign, 0, 0, 10, 1), "sequence set of another aligner")
            refused(sites(foreign, -1, 0, -1, 1, 500, 4), "sequence set of another aligner")
            changed = list(e["refs"])
            changed[2] = changed[2][:-1]
            other = native_set(rig.al, changed)
            refused(calls(other, 0, 0, 10, 1), "sequence 2 of the set has 5999 bases, the pileup was made over 6000")
            refused(sites(other, -1, 0, -1, 1, 500, 4), "sequence 2 of the set has 5999 bases, the pileup was made over 6000")
            fewer = native_set(rig.al, e["refs"][:5])
            refused(sites(fewer, -1, 0, -1, 1, 500, 4), "the set holds 5 sequences, the pileup was made over 6")
            refused(calls(rig.ps, 0, 0, 10, 1), "the set holds 2400 sequences")
            for bad in ((6, 0, 1), (-1, 0, 1), (0, -1, 5), (0, 2990, 11), (4, 0, 42), (5, 0, 1)):
                refused(calls(ts, *bad, 1), f"rows [{bad[1]}, {bad[1]} + {bad[2]}) of sequence {bad[0]} are out of range")
            refused(sites(ts, 0, 2990, 11, 1, 500, 4), "rows [2990, 2990 + 11) of sequence 0 are out of range (6 sequences; sequence length 3000)")
            refused(sites(ts, -1, 5, -1, 1, 500, 4), "seq = -1 (every sequence) goes with start = 0 and len = -1, got start = 5, len = -1")
            refused(sites(ts, -1, 0, 100, 1, 500, 4), "got start = 0, len = 100")
            refused(sites(ts, -2, 0, -1, 1, 500, 4), "out of range")
            refused(calls(ts, 0, 0, 10, 0), "min_depth = 0 is out of range")
            refused(sites(ts, -1, 0, -1, -3, 500, 4), "min_depth = -3 is out of range")
            refused(sites(ts, -1, 0, -1, 1, 0, 4), "min_permille = 0 is out of range (1 .. 1000)")
            refused(sites(ts, -1, 0, -1, 1, 1001, 4), "min_permille = 1001 is out of range (1 .. 1000)")
            refused(sites(ts, -1, 0, -1, 1, 500, -1), "cap = -1 is negative")
            refused(calls(ts, 0, 0, 10, 1, None), "null output")
            refused(sites(ts, -1, 0, -1, 1, 500, 4, None), "null count")
            refused(sites(ts, -1, 0, -1, 1, 500, 4, ctypes.byref(count), None), "null rows")
            # usable afterwards
            assert calls(ts, 0, 0, 64, 1) == _native.OK and np.array_equal(out, expected_calls(1)[0][:64])
        finally:
            al2.close()


def letters(code):
    return "".join("ACGTN-N"[c] for c in code if c != 5)


@pytest.mark.gpu
def test_python_handles_and_lists(gpu):
    e = expectation()
    refs, W = e["refs"], e["W"]
    kw = dict(i=W["i"], j=W["j"], pattern_start=W["p_start"], pattern_len=W["p_len"], text_start=W["t_start"], text_len=W["t_len"], reverse=W["reverse"])
    wa = WavefrontAligner(**KW)
    want = expected_sites(1, 500)
    with wa.sequence_set(refs) as G:
        p = wa.pileup(e["reads"], G, **kw)
        for texts in (G, refs):
            for j in (0, 3, 4, 5):
                c = p.calls(texts, j)
                assert set(c) == {"code", "ins"} and c["code"].dtype == np.uint8 and c["ins"].dtype == bool
                assert np.array_equal(c["code"] | (c["ins"].astype(np.uint8) << 3), expected_calls(1)[j]), j
                assert p.consensus(texts, j) == letters(expected_calls(1)[j] & 7)
            assert p.consensus(texts, 2, 1001, 3334, min_depth=8) == letters(expected_calls(8)[2][1001:3334] & 7)
            s = p.sites(texts)
            assert tuple(s) == p.SITE_COLUMNS and all(v.dtype == np.int32 for v in s.values())
            assert np.array_equal(np.stack([s[k] for k in p.SITE_COLUMNS], axis=1), want)
            s = p.sites(texts, 2, 1001, 3334, min_depth=8, min_frac=0.2)
            w = in_range(expected_sites(8, 200), 2, 1001, 2333)
            assert len(w) > 0 and np.array_equal(np.stack([s[k] for k in p.SITE_COLUMNS], axis=1), w)
            assert len(p.sites(texts, 5)["pos"]) == 0 and p.consensus(texts, 5) == ""
    # the deleted bases are left out, N stands for another letter and for no call
    assert len(p.consensus(refs, 1)) < len(refs[1]) and "N" in p.consensus(refs, 1)
    with pytest.raises(ValueError, match="sequence set is closed"):
        p.calls(G, 0)
    for bad, pattern in ((dict(j=6), "j = 6 is out of range for 6 text sequences"), (dict(j=0, start=5, stop=3001), r"rows \[5, 3001\) are out of range"),
                         (dict(j=0, min_depth=0), "min_depth = 0 is out of range")):
        with pytest.raises(ValueError, match=pattern):
            p.calls(refs, **bad)
        with pytest.raises(ValueError, match=pattern):
            p.sites(refs, **bad)
    for frac in (0, 0.0004, 1.2, "0.5"):
        with pytest.raises(ValueError, match="min_frac"):
            p.sites(refs, min_frac=frac)
    with pytest.raises(ValueError, match="start and stop go with one text"):
        p.sites(refs, start=3)
    with pytest.raises(ValueError, match=r"texts\[2\] has 5999 bases, the pileup was made over 6000"):
        p.sites(refs[:2] + [refs[2][:-1]] + refs[3:])
    with pytest.raises(ValueError, match="texts holds 5 sequences"):
        p.calls(refs[:5], 0)
    p.close()
    with pytest.raises(ValueError, match="pileup is closed"):
        p.sites(refs)
    with pytest.raises(ValueError, match="pileup is closed"):
        p.consensus(refs, 0)
