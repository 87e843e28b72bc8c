"""The insertion log of a pileup on the GPU (wfa_hip_pileup_track_insertions / _insertion_stats / _insertions, Pileup.insertions,
Pileup.consensus(insertions=True)): the device must equal the Python restatement of the rule (insertions_common) applied to the records
and tables built from the ORACLE's op strings — never to the device's own output — exactly: through the C ABI over ranges, parameters,
capacities and chunk sizes, with the list added in pieces and in reversed order, after a clear, with the limit lowered, with tracking
off; and from Python with handles and with lists."""
import ctypes

import numpy as np
import pytest

from calls_common import py_calls, py_sites_all
from common import configs_pair
from insertions_common import (KW, STAGE, expectation, expected_insertions, in_range, py_insertions, py_splice, records_of)
from pywfa_amd import WavefrontAligner, _native
from test_windows_gpu import native_set, native_windows

FILL = -7
RANGES = [(0, 13, 1000), (2, 1001, 1999), (STAGE, 250, 700), (STAGE, 1200, 401), (1, 1960, 500), (4, 5, 30), (4, 0, 41), (1, 3500, 0), (3, 0, 0), (5, 0, 0)]


class Rig:
    """An aligner, the two sets and a pileup of the corpus at the C ABI binding; `order`: the pieces of the list (of `parts`) in the
    order they are added; `track`: whether the pileup tracks insertions."""

    def __init__(self, parts=1, order=None, track=True):
        e = expectation()
        self.e = e
        _, nc = configs_pair(**KW)
        self.al = _native.Aligner(nc)
        self.ps, self.ts = native_set(self.al, e["reads"]), native_set(self.al, e["refs"])
        self.pile = self.al.pileup(self.ts)
        if track:
            self.pile.track_insertions(True)
        n = len(e["W"]["i"])
        cuts = [n * k // parts for k in range(parts + 1)]
        self.batches = []
        for k in (range(parts) if order is None else order):
            part = {key: v[cuts[k]:cuts[k + 1]] for key, v in e["W"].items()}
            rb = native_windows(self.al, self.ps, self.ts, part)
            rb.run()
            self.pile.add(rb, part["j"], part["t_start"])
            self.batches.append((rb, part))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.al.close()
        return False

    def raw(self, seq, start, length, md, pm, cap, bases_cap, count, rows, nbases, bases, ts=None):
        ts = self.ts if ts is None else ts
        return _native.lib().wfa_hip_pileup_insertions(self.pile._h, ts._h, seq, start, length, md, pm, cap, count, rows, bases_cap, nbases, bases)

    def ins(self, seq=-1, start=0, length=-1, md=1, pm=500, cap=None, bases_cap=None):
        """wfa_hip_pileup_insertions on arrays prefilled with FILL / 99: (count, rows, bases_count, bases); a capacity of None: the
        counting call first."""
        count, nbases = ctypes.c_int64(-1), ctypes.c_int64(-1)
        if cap is None or bases_cap is None:
            assert self.raw(seq, start, length, md, pm, 0, 0, ctypes.byref(count), None, ctypes.byref(nbases), None) == _native.OK, self.al.error()
            cap = count.value if cap is None else cap
            bases_cap = nbases.value if bases_cap is None else bases_cap
        rows, bases = np.full((cap, 8), FILL, np.int32), np.full(bases_cap, 99, np.uint8)
        rc = self.raw(seq, start, length, md, pm, cap, bases_cap, ctypes.byref(count), rows.ctypes.data if cap else None, ctypes.byref(nbases),
                      bases.ctypes.data if bases_cap else None)
        assert rc == _native.OK, self.al.error()
        return count.value, rows, nbases.value, bases

    def check(self, want, ctx, **kw):
        rows, seqs = want
        count, got, nbases, bases = self.ins(**kw)
        assert count == len(rows) and np.array_equal(got, rows), (ctx, count, len(rows))
        assert nbases == sum(map(len, seqs)) and bases.tobytes().decode() == "".join(seqs), ctx
        return got, bases


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", ["64", None])
def test_c_abi_over_parameters_ranges_and_capacities(gpu, monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("WFA_HIP_CALLS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("WFA_HIP_CALLS_CHUNK", chunk)
    monkeypatch.delenv("WFA_HIP_INS_MAX_READS", raising=False)
    with Rig() as rig:
        e = rig.e
        for md in (1, 8):
            for pm in (0, 1, 200, 500, 1000):
                want = expected_insertions(md, pm)
                got, bases = rig.check(want, (md, pm), md=md, pm=pm)
                again = rig.ins(md=md, pm=pm)
                assert again[1].tobytes() == got.tobytes() and again[3].tobytes() == bases.tobytes()          # two calls, identical bytes
                if pm > 0:     # the rows are the sites whose ins condition holds
                    sites = py_sites_all(e["tables"], e["refs"], md, pm)
                    sites = sites[(sites[:, 7] >= 1) & (1000 * sites[:, 7].astype(np.int64) >= pm * sites[:, 4].astype(np.int64))]
                    count, dev_sites = rig.pile.sites(rig.ts, min_depth=md, min_permille=pm)
                    dev_sites = dev_sites[(dev_sites[:, 7] >= 1) & (1000 * dev_sites[:, 7].astype(np.int64) >= pm * dev_sites[:, 4].astype(np.int64))]
                    assert np.array_equal(got[:, :4], sites[:, [0, 1, 4, 7]]) and np.array_equal(got[:, :4], dev_sites[:, [0, 1, 4, 7]]), (md, pm)
                else:          # ... the positions where calls sets bit 3
                    at = [(j, g) for j, (t, r) in enumerate(zip(e["tables"], e["refs"])) for g in np.flatnonzero(py_calls(t, r.encode(), md) & 8)]
                    dev = [(j, g) for j in range(len(e["refs"])) for g in np.flatnonzero(rig.pile.calls(rig.ts, j, min_depth=md) & 8)]
                    assert [(int(r[0]), int(r[1])) for r in got] == at == dev, (md, pm)
        want = expected_insertions(1, 500)
        for seq, start, length in RANGES:
            rig.check(in_range(*want, seq, start, length), (seq, start, length), seq=seq, start=start, length=length)
        rows, seqs = want
        n, nb, text = len(rows), sum(map(len, seqs)), "".join(seqs).encode()
        ends = np.cumsum(rows[:, 5])
        mid = int(ends[n // 2])
        assert n > 12 and 0 < mid < nb
        for cap in (0, 1, n - 1, n, n + 5):
            for bases_cap in (0, 1, mid - 1, mid, nb - 1, nb, nb + 7):
                count, got, nbases, bases = rig.ins(cap=cap, bases_cap=bases_cap)
                k = min(cap, n)
                fit = max([int(x) for x in ends[:k] if x <= bases_cap], default=0)
                assert count == n and nbases == nb, (cap, bases_cap)
                assert np.array_equal(got[:k], rows[:k]) and (got[k:] == FILL).all(), (cap, bases_cap)
                assert bases[:fit].tobytes() == text[:fit] and (bases[fit:] == 99).all(), (cap, bases_cap)
        w = in_range(*want, STAGE, 250, 1400)
        count, got, nbases, bases = rig.ins(STAGE, 250, 1400, cap=3, bases_cap=6)
        assert count == len(w[0]) > 3 and np.array_equal(got, w[0][:3]) and nbases == sum(map(len, w[1])) > 70


@pytest.mark.gpu
@pytest.mark.parametrize("parts,order", [(1, None), (2, None), (3, None), (3, (2, 1, 0))])
def test_pieces_orders_stats_and_a_clear(gpu, monkeypatch, parts, order):
    monkeypatch.setenv("WFA_HIP_CALLS_CHUNK", "192")
    with Rig(parts, order) as rig:
        e = rig.e
        total = (sum(len(r) for r in e["per_pair"]), sum(n for r in e["per_pair"] for _, n, _ in r))
        assert rig.pile.insertion_stats() == total and total[0] > 500
        for md, pm in ((1, 500), (8, 0), (1, 1)):
            rig.check(expected_insertions(md, pm), (parts, order, md, pm), md=md, pm=pm)
        # column 6 is the records per row
        for j, recs in enumerate(e["records"]):
            at = np.zeros(len(e["refs"][j]), np.int32)
            for g, r in recs.items():
                at[g] = len(r)
            assert np.array_equal(rig.pile.read(j)[:, 6], at), j
        if parts != 2:
            return
        # cleared: the log is dropped, the setting kept; the second half added twice and the first once
        rig.pile.clear()
        assert rig.pile.insertion_stats() == (0, 0)
        assert rig.ins(cap=4, bases_cap=4)[0::2] == (0, 0)
        for k in (1, 0, 1):
            rb, part = rig.batches[k]
            rig.pile.add(rb, part["j"], part["t_start"])
        n = len(e["pats"])
        second = np.arange(n) >= n // 2
        from reduce_common import expected_tables
        twice, _ = expected_tables([len(r) for r in e["refs"]], e["o"], e["pats"], e["W"]["j"], e["W"]["t_start"], e["W"]["t_len"], second)
        more = records_of(e["per_pair"], e["W"], len(e["refs"]), second)
        rows, seqs = [], []
        for j, t in enumerate(e["tables"]):
            both = {g: e["records"][j].get(g, []) + more[j].get(g, []) for g in set(e["records"][j]) | set(more[j])}
            r, s = py_insertions(t + twice[j], both, j, 0, 8, 200)
            rows.append(r)
            seqs += s
        rows = np.concatenate(rows)
        rig.check((rows, seqs), "re-added", md=8, pm=200)
        assert len(rows) != len(expected_insertions(8, 200)[0])
        # ... and cleared again, the whole list once: as at first
        rig.pile.clear()
        for rb, part in rig.batches:
            rig.pile.add(rb, part["j"], part["t_start"])
        rig.check(expected_insertions(1, 500), "after a clear and a re-add")
        assert rig.pile.insertion_stats() == total


@pytest.mark.gpu
def test_the_limit_lowered(gpu, monkeypatch):
    with Rig() as rig:
        full = expected_insertions(1, 500)
        low = expected_insertions(1, 500, 8)
        over = low[0][:, 7] == 1
        assert over.sum() >= 8 and (~over).sum() >= 3 and (low[0][over][:, 4:7] == 0).all() and (low[0][over][:, 3] > 8).all()
        assert np.array_equal(low[0][~over], full[0][~over])
        monkeypatch.setenv("WFA_HIP_INS_MAX_READS", "8")
        rig.check(low, "limit 8")
        monkeypatch.setenv("WFA_HIP_INS_MAX_READS", "0")       # (at least 1)
        rig.check(expected_insertions(1, 500, 1), "limit 1")
        monkeypatch.delenv("WFA_HIP_INS_MAX_READS")
        rig.check(full, "limit back at its default")


@pytest.mark.gpu
def test_tracking_off_and_the_refusals(gpu):
    with Rig() as rig, Rig(track=False) as plain:
        for j in range(len(rig.e["refs"])):
            assert np.array_equal(rig.pile.read(j), plain.pile.read(j)) and np.array_equal(rig.pile.read(j), rig.e["tables"][j]), j
        rows, bases = np.full((4, 8), FILL, np.int32), np.full(16, 99, np.uint8)
        count, nbases = ctypes.c_int64(-1), ctypes.c_int64(-1)

        def refused(r, rc, pattern):
            assert rc == _native.EINVAL and pattern in r.al.error(), (rc, r.al.error())
            assert (rows == FILL).all() and (bases == 99).all() and count.value == -1 and nbases.value == -1

        def call(r, seq=-1, start=0, length=-1, md=1, pm=500, cap=4, bases_cap=16, cnt=ctypes.byref(count), rowp=rows.ctypes.data,
                 nb=ctypes.byref(nbases), basep=bases.ctypes.data, ts=None):
            return r.raw(seq, start, length, md, pm, cap, bases_cap, cnt, rowp, nb, basep, ts)

        refused(plain, call(plain), "was not made to track insertions")
        assert _native.lib().wfa_hip_pileup_insertion_stats(plain.pile._h, None, None) == _native.EINVAL
        L = _native.lib()
        for r in (rig, plain):       # after an add the setting stays
            for on in (0, 1):
                assert L.wfa_hip_pileup_track_insertions(r.pile._h, on) == _native.EINVAL and "while the pileup is empty" in r.al.error()
        refused(plain, call(plain), "was not made to track insertions")
        refused(rig, call(rig, bases_cap=-1), "bases_cap = -1 is negative")
        refused(rig, call(rig, cap=-1), "cap = -1 is negative")
        refused(rig, call(rig, md=0), "min_depth = 0 is out of range")
        refused(rig, call(rig, pm=-1), "min_permille = -1 is out of range (0 .. 1000)")
        refused(rig, call(rig, pm=1001), "min_permille = 1001 is out of range (0 .. 1000)")
        refused(rig, call(rig, start=5), "seq = -1 (every sequence) goes with start = 0 and len = -1")
        refused(rig, call(rig, seq=0, start=2490, length=11), "rows [2490, 2490 + 11) of sequence 0 are out of range")
        refused(rig, call(rig, seq=6, start=0, length=1), "out of range")
        refused(rig, call(rig, ts=rig.ps), "the set holds")
        refused(rig, call(rig, ts=plain.ts), "sequence set of another aligner")
        refused(rig, call(rig, cnt=None), "null count")
        refused(rig, call(rig, nb=None), "null count")
        refused(rig, call(rig, rowp=None), "null rows")
        refused(rig, call(rig, basep=None), "null bases")
        # sites keeps its own range of min_permille
        assert L.wfa_hip_pileup_sites(rig.pile._h, rig.ts._h, -1, 0, -1, 1, 0, 0, ctypes.byref(count), None) == _native.EINVAL
        assert "min_permille = 0 is out of range (1 .. 1000)" in rig.al.error() and count.value == -1
        # a cleared pileup takes the setting again: off, the list added, as the plain one; on again after another clear
        rig.pile.clear()
        rig.pile.track_insertions(False)
        rb, part = rig.batches[0]
        rig.pile.add(rb, part["j"], part["t_start"])
        refused(rig, call(rig), "was not made to track insertions")
        assert np.array_equal(rig.pile.read(STAGE), plain.pile.read(STAGE))
        rig.pile.clear()
        rig.pile.track_insertions(True)
        rig.pile.add(rb, part["j"], part["t_start"])
        rig.check(expected_insertions(1, 500), "tracking on again")


@pytest.mark.gpu
def test_python_handles_and_lists(gpu):
    e = expectation()
    refs, W = e["refs"], e["W"]
    kw = dict(i=W["i"], j=W["j"], pattern_start=W["p_start"], pattern_len=W["p_len"], text_start=W["t_start"], text_len=W["t_len"], reverse=W["reverse"])
    wa = WavefrontAligner(**KW)
    rows, seqs = expected_insertions(1, 500)
    major = expected_insertions(1, 0), expected_insertions(8, 0)
    calls = {md: [py_calls(t, r.encode(), md) for t, r in zip(e["tables"], refs)] for md in (1, 8)}
    d = e["planted"]["d"][1]
    with wa.sequence_set(refs) as G:
        p = wa.pileup(e["reads"], G, insertions=True, **kw)
        plain = wa.pileup(e["reads"], G, **kw)
        for texts in (G, refs):
            s = p.insertions(texts)
            assert tuple(s) == p.INSERTION_COLUMNS + ("seq",) and all(s[k].dtype == np.int32 for k in p.INSERTION_COLUMNS)
            assert np.array_equal(np.stack([s[k] for k in p.INSERTION_COLUMNS], axis=1), rows) and s["seq"] == list(seqs)
            s = p.insertions(texts, STAGE, 250, 1700, min_depth=8, min_frac=0.2)
            w = in_range(*expected_insertions(8, 200), STAGE, 250, 1450)
            assert len(w[0]) >= 4 and np.array_equal(np.stack([s[k] for k in p.INSERTION_COLUMNS], axis=1), w[0]) and s["seq"] == list(w[1])
            assert p.insertions(texts, 5)["seq"] == [] and p.consensus(texts, 5, insertions=True) == ""
            for j in range(len(refs)):
                got = p.consensus(texts, j, insertions=True)
                assert got == py_splice(calls[1][j], *in_range(*major[0], j, 0, len(refs[j])), 0), j
                assert p.consensus(texts, j) == plain.consensus(texts, j) == "".join("ACGTN-N"[c & 7] for c in calls[1][j] if c & 7 != 5), j
            # a range that starts at the 70-base insertion: it goes in front of `start`
            got = p.consensus(texts, STAGE, d, d + 300, min_depth=8, insertions=True)
            assert got == py_splice(calls[8][STAGE][d:d + 300], *in_range(*major[1], STAGE, d, 300), d) and got.startswith(e["planted"]["d"][2])
        for call in (lambda: plain.insertions(refs), lambda: plain.consensus(refs, 0, insertions=True), lambda: plain.insertions(G, 0)):
            with pytest.raises(ValueError, match="was not made to track insertions"):
                call()
    for bad, pattern in ((dict(j=6), "j = 6 is out of range for 6 text sequences"), (dict(j=0, start=5, stop=2501), r"rows \[5, 2501\) are out of range"),
                         (dict(j=0, min_depth=0), "min_depth = 0 is out of range"), (dict(min_frac=0), "min_frac"), (dict(min_frac=1.2), "min_frac"),
                         (dict(start=3), "start and stop go with one text")):
        with pytest.raises(ValueError, match=pattern):
            p.insertions(refs, **bad)
    p.close()
    plain.close()
    with pytest.raises(ValueError, match="pileup is closed"):
        p.insertions(refs)
    with pytest.raises(ValueError, match="pileup is closed"):
        p.consensus(refs, 0, insertions=True)
