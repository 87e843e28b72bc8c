"""Per-pair summaries reduced on the GPU (wfa_hip_batch_summary, ResidentBatch.summary, the summary=True forms): row for row the
host statement wfa_hip_ops_summary of the ORACLE's op string of the pair — never of the library's own —, for plain, packed2bits,
indexed and windowed batches of short (150 bp) and long (2 kb) reads under six configurations; exact equality."""
import numpy as np
import pytest

from common import assert_same, configs_pair
from oracle import loader
from pywfa_amd import WavefrontAligner, _native, datagen
from test_windows_gpu import cigars_of, native_set, revcomp

CONFIGS = [
    ("affine end-to-end", dict(span="end-to-end")),
    ("ends-free, free text ends", dict(span="ends-free", text_begin_free=10, text_end_free=10)),
    ("affine2p", dict(distance="affine2p", span="end-to-end")),
    ("edit", dict(distance="levenshtein", span="end-to-end")),
    ("wf-adaptive", dict(span="end-to-end", heuristic="adaptive")),
    ("max_steps", None),    # (the limit depends on the read length: STEP_LIMIT)
]
STEP_LIMIT = {"short": 50, "long": 280}
N_PURE = {"short": 640, "long": 10}


def pairs_of(kind):
    """The pairs of one length class as strings: ACGT-only pairs first (those a 2-bit batch can hold), then pairs whose pattern or
    text holds an N (aligned on their bytes)."""
    if kind == "short":
        b = datagen.generate(700, 150, 0.04, 9001, use_native=False)
    else:
        b = datagen.generate(12, 2000, 0.02, 9002, use_native=False)
    pats, txts = zip(*(datagen.pair_strings(b, q) for q in range(len(b["p_len"]))))
    pats, txts = list(pats), list(txts)
    for q in range(N_PURE[kind], len(pats)):
        s = pats[q] if q % 2 else txts[q]
        s = s[:17] + "N" + s[18:60] + "NN" + s[62:]
        if q % 2:
            pats[q] = s
        else:
            txts[q] = s
    return pats, txts


PAIRS = {kind: pairs_of(kind) for kind in ("short", "long")}


def config_for(name, kw, kind):
    return dict(span="end-to-end", max_steps=STEP_LIMIT[kind]) if kw is None else kw


def expected(kw, kind):
    pats, txts = PAIRS[kind]
    batch = datagen.from_strings(pats, txts, upper=True)
    o = loader.run(loader.oracle(), loader.make_config(**kw), batch)
    rows = np.stack([_native.ops_summary(c, len(p), len(t)) for c, p, t in zip(o["cigars"], pats, txts)])
    return o, batch, rows


@pytest.mark.parametrize("kind", ["short", "long"])
def test_step_limit_splits_the_pairs(kind):
    """No GPU: under the step limit between one pair and half of the pairs end with status -100 (the oracle's statuses)."""
    o, _, rows = expected(config_for("max_steps", None, kind), kind)
    stopped = int((np.asarray(o["status"]) == -100).sum())
    assert 1 <= stopped <= len(o["status"]) // 2, stopped
    assert not rows[np.asarray(o["status"]) == -100, :6].any()


def window_list(kind):
    """The same pairs as windows: every text inside a padded sequence, every second pattern stored reverse-complemented and padded."""
    pats, txts = PAIRS[kind]
    n = len(pats)
    pset = [("GATTACA" + revcomp(p) + "CC") if q % 2 else ("TT" + p + "ACGTTGCA") for q, p in enumerate(pats)]
    tset = ["ACGTAC"[:q % 7] + t + "TTGACC" for q, t in enumerate(txts)]
    W = dict(i=np.arange(n, dtype=np.int32), j=np.arange(n, dtype=np.int32),
             p_start=np.array([7 if q % 2 else 2 for q in range(n)], np.int32), p_len=np.array([len(p) for p in pats], np.int32),
             t_start=np.array([len("ACGTAC"[:q % 7]) for q in range(n)], np.int32), t_len=np.array([len(t) for t in txts], np.int32),
             reverse=np.array([q % 2 for q in range(n)], np.uint8))
    return pset, tset, W


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["short", "long"])
@pytest.mark.parametrize("name,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_summary_of_every_batch_kind(gpu, name, kw, kind):
    kw = config_for(name, kw, kind)
    o, batch, want = expected(kw, kind)
    pats, txts = PAIRS[kind]
    n, npure = len(pats), N_PURE[kind]
    _, nc = configs_pair(**kw)
    al = _native.Aligner(nc)
    try:
        def run(rb, lo, hi, what):
            rb.run()
            rb.sync()
            score, status, cig = rb.results(True)
            got = rb.summary()
            again = rb.summary()
            locs = rb.rle()[3]
            rb.close()
            sub = {k: (v[lo:hi] if v is not None else None) for k, v in o.items()}
            assert_same(sub, score, status, cigars_of(cig, hi - lo), datagen.subset(batch, np.arange(lo, hi)), (name, kind, what))
            assert got.dtype == np.int32 and got.shape == (hi - lo, 10)
            bad = np.flatnonzero((got != want[lo:hi]).any(axis=1))
            assert bad.size == 0, (name, kind, what, int(bad[0]), got[bad[0]], want[lo + bad[0]])
            assert np.array_equal(again, got) and np.array_equal(got[:, 6:], locs), (name, kind, what)

        run(al.batch(batch), 0, n, "plain")
        pure = datagen.subset(batch, np.arange(npure))
        run(al.batch(datagen.to_packed2bits(pure)), 0, npure, "packed2bits")
        ps, ts = native_set(al, pats), native_set(al, txts)
        idx = np.arange(n, dtype=np.int32)
        run(al.batch_indexed(ps, ts, idx, idx), 0, n, "indexed")
        ps.close()
        ts.close()
        pset, tset, W = window_list(kind)
        ps, ts = native_set(al, pset), native_set(al, tset)
        run(al.batch_windows(ps, ts, W["i"], W["j"], W["p_start"], W["p_len"], W["t_start"], W["t_len"], W["reverse"]), 0, n, "windows")
        ps.close()
        ts.close()
    finally:
        al.close()
    if "max_steps" in kw:
        stopped = np.asarray(o["status"]) == -100
        assert 1 <= stopped.sum() <= n // 2 and not want[stopped, :6].any()


def check_dict(out, o, want, ctx):
    assert set(out) == {"score", "status", "summary"}, (ctx, sorted(out))
    assert np.array_equal(out["score"], o["score"]) and np.array_equal(out["status"], o["status"]), ctx
    s = out["summary"]
    assert set(s) == {"M", "X", "I", "D", "I_runs", "D_runs", "locations"}, ctx
    for k, key in enumerate(("M", "X", "I", "D", "I_runs", "D_runs")):
        assert s[key].dtype == np.int32 and np.array_equal(s[key], want[:, k]), (ctx, key)
    assert s["locations"].dtype == np.int32 and np.array_equal(s["locations"], want[:, 6:]), ctx


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [CONFIGS[1], CONFIGS[5]], ids=[CONFIGS[1][0], CONFIGS[5][0]])
def test_python_forms(gpu, monkeypatch, name, kw):
    """summary=True through align_pairs / align_windows (a chunk boundary every 250 pairs), align_batch and wavefront_align_batch
    (700 pairs: below the 1 024 of the single-call form); summary=False is what it was."""
    kind = "short"
    kw = config_for(name, kw, kind)
    o, batch, want = expected(kw, kind)
    pats, txts = PAIRS[kind]
    n = len(pats)
    idx = np.arange(n)
    pset, tset, W = window_list(kind)
    wa = WavefrontAligner(**kw)
    wkw = dict(i=W["i"], j=W["j"], pattern_start=W["p_start"], pattern_len=W["p_len"], text_start=W["t_start"], text_len=W["t_len"],
               reverse=W["reverse"])
    monkeypatch.setenv("WFA_HIP_PAIRS_BAND", "250")
    check_dict(wa.align_pairs(pats, txts, i=idx, j=idx, summary=True), o, want, (name, "align_pairs"))
    check_dict(wa.align_windows(pset, tset, summary=True, **wkw), o, want, (name, "align_windows"))
    with wa.sequence_set(pset) as P, wa.sequence_set(tset) as T:
        check_dict(wa.align_windows(P, T, summary=True, **wkw), o, want, (name, "align_windows, handles"))
    monkeypatch.delenv("WFA_HIP_PAIRS_BAND")
    check_dict(wa.align_windows(pset, tset, summary=True, **wkw), o, want, (name, "align_windows, one chunk"))
    check_dict(wa.align_batch(batch, summary=True), o, want, (name, "align_batch"))
    check_dict(wa.wavefront_align_batch(txts, pats, summary=True), o, want, (name, "wavefront_align_batch"))
    few = wa.align_pairs(pats, txts, i=idx[:7], j=idx[:7], summary=True)            # below 1 024 pairs too
    check_dict(few, {k: v[:7] for k, v in o.items()}, want[:7], (name, "seven pairs"))
    empty = wa.align_pairs(pats, txts, i=[], j=[], summary=True)
    assert empty["summary"]["M"].shape == (0,) and empty["summary"]["locations"].shape == (0, 4)
    # summary=False: the op strings, as before
    for out in (wa.align_windows(pset, tset, **wkw), wa.align_windows(pset, tset, summary=False, **wkw), wa.align_batch(batch),
                wa.align_pairs(pats, txts, i=idx, j=idx)):
        assert set(out) == {"score", "status", "cigar_ops", "cigarstrings"}
        assert_same(o, out["score"], out["status"], [np.asarray(out["cigar_ops"][q], np.uint8).tobytes() for q in range(n)], batch, name)


@pytest.mark.gpu
def test_refusals(gpu):
    pats, txts = PAIRS["short"]
    batch = datagen.from_strings(pats[:50], txts[:50], upper=True)
    _, nc = configs_pair(span="end-to-end", scope="score")
    al = _native.Aligner(nc)
    try:
        rb = al.batch(batch)
        rb.run()
        rb.sync()
        with pytest.raises(ValueError, match="needs scope=full"):
            rb.summary()
        rb.close()
        nf = nc.copy()
        nf.scope = 1
        al.set_config(nf)
        rb = al.batch(batch)
        with pytest.raises(ValueError, match="needs a finished run"):
            rb.summary()
        rb.run()
        assert _native.lib().wfa_hip_batch_summary(rb._h, None) == _native.EINVAL
        assert rb.summary().shape == (50, 10)         # (syncs the run itself)
        rb.close()
        e = np.zeros(0, np.int64)
        rb = al.batch(dict(seqs=np.zeros(1, np.uint8), p_off=e, t_off=e, p_len=e.astype(np.int32), t_len=e.astype(np.int32)))
        rb.run()
        assert rb.summary().shape == (0, 10)
        rb.close()
    finally:
        al.close()
