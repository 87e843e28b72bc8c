"""The two reductions of op strings, the part that needs no GPU: the C entries are declared, exported and bound; the host-only
statements wfa_hip_ops_summary / wfa_hip_ops_pileup (what the kernels compute, for one pair) equal plain Python restatements of the
rules on hand-written op strings and on every op string the oracle returns for a mutated corpus; the Python forms refuse a score
scope and bad arrays before they touch a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from common import configs_pair
from oracle import loader
from pywfa_amd import WavefrontAligner, _native, datagen
from reduce_common import core_of, py_pileup, py_summary

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

ENTRIES = {
    "wfa_hip_batch_summary": "int wfa_hip_batch_summary(wfa_hip_batch_t* batch, int32_t* summary);",
    "wfa_hip_ops_summary": "int wfa_hip_ops_summary(const uint8_t* ops, int64_t ops_len, int32_t plen, int32_t tlen, int32_t* out10);",
    "wfa_hip_pileup_create": "wfa_hip_pileup_t* wfa_hip_pileup_create(wfa_hip_aligner_t* aligner, const wfa_hip_seqset_t* texts);",
    "wfa_hip_pileup_add": "int wfa_hip_pileup_add(wfa_hip_pileup_t* pileup, wfa_hip_batch_t* batch, const int32_t* j, const int32_t* t_start , "
                          "const uint8_t* keep );",
    "wfa_hip_pileup_read": "int wfa_hip_pileup_read(wfa_hip_pileup_t* pileup, int32_t seq, int64_t start, int64_t len, int32_t* counts );",
    "wfa_hip_pileup_clear": "int wfa_hip_pileup_clear(wfa_hip_pileup_t* pileup);",
    "wfa_hip_pileup_destroy": "void wfa_hip_pileup_destroy(wfa_hip_pileup_t* pileup);",
    "wfa_hip_ops_pileup": "int wfa_hip_ops_pileup(const uint8_t* ops, int64_t ops_len, const uint8_t* pattern, int32_t plen, int32_t tlen, "
                          "int32_t* rows );",
}


def header_text():
    txt = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_header_declares_the_entries_and_constants():
    txt = header_text()
    for decl in ENTRIES.values():
        assert decl in txt, decl
    assert "#define WFA_HIP_SUMMARY_COLS 10 " in txt and "#define WFA_HIP_PILEUP_COLS 8 " in txt
    assert "typedef struct wfa_hip_pileup wfa_hip_pileup_t;" in txt
    raw = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    assert "32 BYTES PER TEXT BASE" in raw and "NOT CHECKED FOR OVERFLOW" in raw


def test_native_lists_and_binds_the_entries():
    L = _native.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    for name in ENTRIES:
        assert name in _native.SYMBOLS and hasattr(L, name), name
    assert L.wfa_hip_batch_summary.argtypes == [vp, vp]
    assert L.wfa_hip_ops_summary.argtypes == [vp, i64, i32, i32, vp]
    assert L.wfa_hip_pileup_create.argtypes == [vp, vp] and L.wfa_hip_pileup_create.restype is vp
    assert L.wfa_hip_pileup_add.argtypes == [vp] * 5
    assert L.wfa_hip_pileup_read.argtypes == [vp, i32, i64, i64, vp]
    assert L.wfa_hip_pileup_clear.argtypes == [vp]
    assert L.wfa_hip_pileup_destroy.argtypes == [vp] and L.wfa_hip_pileup_destroy.restype is None
    assert L.wfa_hip_ops_pileup.argtypes == [vp, i64, vp, i32, i32, vp]
    assert _native.SUMMARY_COLS == 10 and _native.PILEUP_COLS == 8 and len(_native.PILEUP_COLUMNS) == 8
    assert L.wfa_hip_abi_version() == _native.ABI_VERSION
    for f in (_native.ResidentBatch.summary, _native.Aligner.pileup, _native.Pileup.add, _native.Pileup.read, _native.Pileup.clear,
              _native.ops_summary, _native.ops_pileup, WavefrontAligner.pileup):
        assert callable(f)


def test_null_handles():
    L = _native.lib()
    out = np.zeros(80, np.int32)
    assert L.wfa_hip_batch_summary(None, out.ctypes.data) == _native.EINVAL
    assert not L.wfa_hip_pileup_create(None, None)
    assert L.wfa_hip_global_error().decode() == "null aligner"
    assert L.wfa_hip_pileup_add(None, None, None, None, None) == _native.EINVAL
    assert L.wfa_hip_pileup_read(None, 0, 0, 1, out.ctypes.data) == _native.EINVAL
    assert L.wfa_hip_pileup_clear(None) == _native.EINVAL
    L.wfa_hip_pileup_destroy(None)
    ops = np.frombuffer(b"MMXM", np.uint8)
    assert L.wfa_hip_ops_summary(ops.ctypes.data, 4, 4, 4, None) == _native.EINVAL
    assert L.wfa_hip_ops_summary(None, 4, 4, 4, out.ctypes.data) == _native.EINVAL
    assert L.wfa_hip_ops_summary(ops.ctypes.data, -1, 4, 4, out.ctypes.data) == _native.EINVAL
    assert L.wfa_hip_ops_summary(None, 0, 4, 4, out.ctypes.data) == _native.OK
    assert L.wfa_hip_ops_pileup(ops.ctypes.data, 4, None, 4, 4, out.ctypes.data) == _native.EINVAL
    assert L.wfa_hip_ops_pileup(ops.ctypes.data, 4, ops.ctypes.data, 4, 4, None) == _native.EINVAL
    assert L.wfa_hip_ops_pileup(None, 0, None, 0, 0, None) == _native.OK
    # an op string that outruns its pair adds nothing
    out[:] = 0
    assert L.wfa_hip_ops_pileup(ops.ctypes.data, 4, ops.ctypes.data, 3, 4, out.ctypes.data) == _native.EINVAL
    assert L.wfa_hip_ops_pileup(ops.ctypes.data, 4, ops.ctypes.data, 4, 3, out.ctypes.data) == _native.EINVAL
    assert not out.any()


def consumed(ops):
    ops = bytes(ops)
    return sum(c in b"MXD" for c in ops), sum(c in b"MXI" for c in ops)


HAND = [b"", b"XXIIDD", b"I", b"D", b"X", b"M", b"IIDDMMXMDDII", b"DDIIMXXMIID", b"MIIDDIIDDM", b"MDIDIDIM", b"XMX", b"IMI", b"DMD",
        b"MMMMIIIIDDDDMMMM", b"XDMMIIMDDMXI", b"M" * 64, b"I" * 63 + b"M" + b"D" * 64 + b"M", b"M" + b"I" * 127 + b"D" * 130 + b"M" + b"X" * 70,
        b"D" * 64 + b"I" * 64 + b"M" * 64 + b"D" * 64 + b"I" * 64, (b"MID" * 50) + b"M", b"X" * 200]


@pytest.mark.parametrize("ops", HAND, ids=[f"hand{k}" for k in range(len(HAND))])
def test_hand_written_op_strings(ops):
    pl, tl = consumed(ops)
    for plen, tlen in ((pl, tl), (pl + 3, tl + 5), (0, tl), (pl, 0)):
        want = py_summary(ops, plen, tlen)
        got = _native.ops_summary(ops, plen, tlen)
        assert got.dtype == np.int32 and np.array_equal(got, want), (ops, plen, tlen, got, want)
    pattern = (b"ACGTNacgt-" * (pl // 10 + 1))[:pl]
    rows = np.zeros((tl, 8), np.int32)
    rows[:] = np.arange(8)                          # (added to, not overwritten)
    want = py_pileup(ops, pattern, rows.copy())
    got = _native.ops_pileup(ops, pattern, tl, rows)
    assert got is rows and np.array_equal(got, want), ops
    check_column_sums(ops, got - np.arange(8, dtype=np.int32)[None, :] if tl else got)


def check_column_sums(ops, rows):
    """Every column total follows from the summary of the aligned core."""
    core = core_of(ops)
    if core is None:
        assert not rows.any()
        return
    inner = bytes(ops)[core[0]:core[1] + 1]
    s = _native.ops_summary(inner, *consumed(inner))
    tot = rows.sum(axis=0)
    assert tot[:5].sum() == s[0] + s[1] and tot[5] == s[2] and tot[6] == s[5] and tot[7] == s[1], (ops, tot, s)


def corpus():
    """200 mutated pairs of ~150 bases (6 % substitutions and indels), every fifth pattern holding Ns and other letters."""
    batch = datagen.generate(200, 150, 0.06, 4242, use_native=False)
    seqs = batch["seqs"].copy()
    rng = np.random.default_rng(5)
    for q in range(0, 200, 5):
        at = batch["p_off"][q] + rng.integers(0, batch["p_len"][q], 6)
        seqs[at[:4]] = ord("N")
        seqs[at[4]] = ord("R")
        seqs[at[5]] = ord("a")
    return dict(batch, seqs=seqs)


CORPUS = corpus()
CONFIGS = [
    ("end-to-end", dict(span="end-to-end"), CORPUS),
    ("ends-free pattern ends", dict(span="ends-free", pattern_begin_free=12, pattern_end_free=12), datagen.trim_text(CORPUS, 10)),
    ("ends-free text ends", dict(span="ends-free", text_begin_free=14, text_end_free=9),
     (lambda b: dict(seqs=b["seqs"], p_off=b["t_off"], p_len=b["t_len"], t_off=b["p_off"], t_len=b["p_len"]))(datagen.trim_text(CORPUS, 8))),
    ("end-to-end, step limit", dict(span="end-to-end", max_steps=80), CORPUS),
]


@pytest.mark.parametrize("name,kw,batch", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_oracle_op_strings(name, kw, batch):
    o = loader.run(loader.oracle(), loader.make_config(**kw), batch)
    n = len(o["cigars"])
    assert n == 200
    lead = trail = with_n = 0
    for q in range(n):
        ops = o["cigars"][q]
        plen, tlen = int(batch["p_len"][q]), int(batch["t_len"][q])
        s = _native.ops_summary(ops, plen, tlen)
        assert np.array_equal(s, py_summary(ops, plen, tlen)), (name, q)
        if o["status"][q] != 0:
            continue
        assert s[0] + s[1] + s[3] == plen and s[0] + s[1] + s[2] == tlen, (name, q)
        pattern = batch["seqs"][batch["p_off"][q]:batch["p_off"][q] + plen].tobytes()
        rows = _native.ops_pileup(ops, pattern, tlen)
        assert np.array_equal(rows, py_pileup(ops, pattern, np.zeros((tlen, 8), np.int32))), (name, q)
        check_column_sums(ops, rows)
        lead += ops[:1] in (b"I", b"D")
        trail += ops[-1:] in (b"I", b"D")
        with_n += rows[:, 4].any()
    done = int((np.asarray(o["status"]) == 0).sum())
    if "max_steps" in kw:
        assert 1 <= n - done <= n // 2, done                   # some pairs end at the step limit, most do not
        assert all(len(o["cigars"][q]) == 0 for q in range(n) if o["status"][q] != 0)
    else:
        assert done == n
    if "ends-free" in name:
        assert lead > 20 and trail > 20, (lead, trail)          # clipped ends in front of and behind the core
    if name in ("end-to-end", "ends-free pattern ends"):         # (the 40 patterns holding letters outside ACGT, all completed)
        assert with_n >= 20, with_n                              # patterns holding N feed the `other` column


def scoped(scope):
    """A WavefrontAligner without a native aligner: whatever raises here raised before any device was touched."""
    al = object.__new__(WavefrontAligner)
    al._cfg = configs_pair(scope=scope)[1]
    return al


SEQS = ["ACGTACGTACGTACGT", "ACGTACGAACGTACGTAA", "ACGT", ""]


def test_score_scope_is_refused_before_any_device():
    al = scoped("score")
    with pytest.raises(ValueError, match="pileup needs scope='full'"):
        al.pileup(SEQS, i=[0], j=[1])
    with pytest.raises(ValueError, match="summary=True needs scope='full'"):
        al.align_windows(SEQS, i=[0], j=[1], summary=True)
    with pytest.raises(ValueError, match="summary=True needs scope='full'"):
        al.align_pairs(SEQS, i=[0], j=[1], summary=True)
    with pytest.raises(ValueError, match="summary=True needs scope='full'"):
        al.align_batch(datagen.from_strings(SEQS[:2], SEQS[:2]), summary=True)
    with pytest.raises(ValueError, match="summary=True needs scope='full'"):
        al.wavefront_align_batch(SEQS[:2], SEQS[:2], summary=True)


@pytest.mark.parametrize("kw,match", [
    (dict(i=[0, 1], j=[1.0, 2.0]), "j must hold integers"),
    (dict(i=[0, 1], j=[1]), "differ in length"),
    (dict(i=[0, 1], j=[1, 2], text_len=[1, 2, 3]), "text_len and i differ in length"),
    (dict(i=[0, -1], j=[1, 2]), r"i\[1\] is negative"),
    (dict(i=[0, 1], j=[1, 4]), r"j\[1\] = 4 is out of range"),
    (dict(i=[0, 1], j=[1, 2], text_start=[0, -3]), r"text_start\[1\] = -3 is negative"),
    (dict(i=[0, 1, 0], j=[1, 2, 2], text_start=[0, 2, 3], text_len=[18, 3, 1]), r"text_start\[1\] \+ text_len\[1\] = 2 \+ 3 runs past the end of text sequence 2 \(4 bases\)"),
    (dict(i=[0, 1], j=[1, 2], reverse=[0, 2]), r"reverse\[1\] = 2 is neither 0 nor 1"),
    (dict(i=[0, 1], j=[1, 2], min_score=-1.5), "min_score must be an integer"),
])
def test_bad_arrays_are_refused_before_any_device(kw, match):
    al = scoped("full")
    with pytest.raises(ValueError, match=match):
        al.pileup(SEQS, **kw)
    with pytest.raises(ValueError, match=match):
        al.pileup(SEQS, list(SEQS), **kw)
    if "min_score" not in kw:
        with pytest.raises(ValueError, match=match):
            al.align_windows(SEQS, summary=True, **kw)
