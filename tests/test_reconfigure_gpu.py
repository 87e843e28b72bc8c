"""Aligners reconfigured through their setters equal the oracle of the configuration they were moved to.

pywfa's WavefrontAligner is used by changing settings between calls (``a.scope = "full"``, ``a.distance = ...``); the setters here
re-derive the whole native configuration.  These tests move live aligners — after a first call, so that the mailbox
instance, the pilots and the pool exist — between a catalogue of configurations chosen to enter and leave every branch of the
library's configuration derivation (the score-mapped forms, the one-component LIN form, the run-time penalty shapes, heuristics, free
ends, step limits, BiWFA, the wildcard), and check every entry point against the oracle of the target configuration, and against a
fresh aligner created in it (a failure there tells leaked state from a kernel bug).

Default run: every ordered pair of states on the single pairs and the 16 / 17-pair batches (the general-kernel tiny form), and a
covering walk for the larger batches, resident batches and score matrices.  WFA_TEST_FULL=1: every entry point at every size on
every ordered pair."""
import os

import numpy as np
import pytest

import common
import validate_oracle as vo   # (tools/, on the tests' path)
from oracle import loader
from pywfa_amd import _native, datagen
import pywfa_amd
from pywfa_amd.align import _INT_MAX

pytestmark = pytest.mark.gpu

FULL = os.environ.get("WFA_TEST_FULL") == "1"
INT32_MIN = -2147483648

# ------------------------------------------------------------------------------------------------------------- states
# (no state combines match < 0 with free begins, tests/test_oracle_vs_ref.py; no BiWFA state has free ends)
FREE = dict(pattern_begin_free=5, pattern_end_free=3, text_begin_free=4, text_end_free=5)
STATES = {
    "affine": {},
    "affine-e2e-score": dict(span="end-to-end", scope="score"),
    "match-1": dict(match=-1),                                   # rescaled penalties (a run-time shape), score_mode 1 after the map
    "match-1-score": dict(match=-1, scope="score"),
    "affine2p-e2e": dict(distance="affine2p", span="end-to-end"),
    "lev-score": dict(distance="levenshtein", scope="score"),    # score_mode 2
    "lev-full": dict(distance="levenshtein"),                    # LIN
    "indel-score": dict(distance="indel", scope="score"),
    "indel-full": dict(distance="indel"),                        # LIN, no mismatch candidate
    "linear-full": dict(distance="linear"),                      # LIN
    "linear-match-1": dict(distance="linear", match=-1),         # not mapped
    "ends-free": dict(FREE),
    "adaptive": dict(heuristic="adaptive"),
    "xdrop": dict(heuristic="X-drop", xdrop=30),
    "max-steps": dict(max_steps=40),
    "biwfa": dict(memory_mode="biwfa"),
    "wildcard": dict(wildcard="N"),
    "rtc-shape": dict(mismatch=7, gap_opening=5, gap_extension=3),   # no built-in instantiation (tests/test_fuzz_gpu.py)
}
NAMES = list(STATES)
SCORE_MODE = ("match-1-score", "lev-score", "indel-score")
LIN = ("lev-full", "indel-full", "linear-full")

DEFAULTS = dict(distance="affine", memory_mode="high", match=0, mismatch=4, gap_opening=6, gap_extension=2, gap_opening2=24,
                gap_extension2=1, scope="full", span="ends-free", pattern_begin_free=0, pattern_end_free=0, text_begin_free=0,
                text_end_free=0, heuristic=None, min_wavefront_length=10, max_distance_threshold=50, steps_between_cutoffs=1,
                xdrop=20, wildcard=None, max_steps=0)
# constructor keyword -> property, in the order the walk applies them
PROP = dict(distance="distance", match="match_score", mismatch="mismatch_penalty", gap_opening="gap_opening_penalty",
            gap_extension="gap_extension_penalty", gap_opening2="gap_opening2_penalty", gap_extension2="gap_extension2_penalty",
            scope="scope", span="span", pattern_begin_free="pattern_begin_free", pattern_end_free="pattern_end_free",
            text_begin_free="text_begin_free", text_end_free="text_end_free", heuristic="heuristic",
            min_wavefront_length="min_wavefront_length", max_distance_threshold="max_distance_threshold",
            steps_between_cutoffs="steps_between_cutoffs", xdrop="xdrop", memory_mode="memory_mode", max_steps="max_steps",
            wildcard="wildcard")


def full_kw(kw):
    return dict(DEFAULTS, **kw)


def getter_value(k, v):
    """What the getter of constructor keyword ``k`` reads after ``v`` was set."""
    return (_INT_MAX if v <= 0 else v) if k == "max_steps" else v


def has_free(kw):
    kw = full_kw(kw)
    return kw["span"] == "ends-free" and any(kw[k] for k in FREE)


def move(a, kw):
    """Move the live aligner ``a`` to configuration ``kw`` through the Python setters: in a fixed order apply every setter that the
    library accepts, keep the refused ones (intermediate combinations such as X-drop under an edit distance) and retry them until
    nothing changes.  Returns the setters that were refused on the way."""
    target = full_kw(kw)
    pending = [k for k in PROP if getattr(a, PROP[k]) != getter_value(k, target[k])]
    refused = []
    while pending:
        left = []
        for k in pending:
            try:
                setattr(a, PROP[k], target[k])
            except (ValueError, NotImplementedError):
                left.append(k)
                refused.append(k)
        assert len(left) < len(pending), f"the setters cannot reach {kw}: {left} refused"
        pending = left
    for k in PROP:
        assert getattr(a, PROP[k]) == getter_value(k, target[k]), (k, kw)
    return refused


def assert_native_config(al, kw):
    """The configuration at the C ABI is the oracle's of ``kw`` (field by field)."""
    oc, _ = common.configs_pair(**kw)
    got = al.get_config()
    for name, _ in _native.Config._fields_:
        assert getattr(got, name) == getattr(oc, name), (name, kw)


# ------------------------------------------------------------------------------------------------------------- inputs
_rng = np.random.default_rng(20261016)


def _rnd(n):
    return "".join(_rng.choice(list("ACGT"), size=n))


def _mutate(s, e, alphabet="ACGT"):
    out = []
    for ch in s:
        u = _rng.random()
        if u < e / 3:
            out.append(str(_rng.choice(list(alphabet))))
        elif u < 2 * e / 3:
            out.append(str(_rng.choice(list("ACGT")))); out.append(ch)
        elif u < e:
            pass
        else:
            out.append(ch)
    return "".join(out)


def _gen(n, L, e, seed):
    b = datagen.generate(n, L, e, seed)
    return [datagen.pair_strings(b, i) for i in range(n)]


def _n_pair(L):
    s = _rnd(L)
    t = list(_mutate(s, 0.05))
    for j in _rng.integers(0, len(t), size=max(1, L // 40)):
        t[j] = "N"
    p = list(s)
    p[int(_rng.integers(0, L))] = "N"
    return "".join(p), "".join(t)


def _short_pool():
    """4 097 pairs of 5 - 1 000 bases: 150-bp reads, short and long divergent ones, unrelated pairs, pairs with N."""
    pairs = _gen(2900, 150, 0.03, 7101) + _gen(600, 60, 0.08, 7102) + _gen(300, 400, 0.05, 7103) + _gen(100, 900, 0.04, 7104)
    pairs += [(_rnd(int(_rng.integers(5, 200))), _rnd(int(_rng.integers(5, 200)))) for _ in range(100)]
    pairs += [_n_pair(int(_rng.integers(20, 300))) for _ in range(97)]
    order = _rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    # (the first 16 pairs hold every kind: an N pair, an unrelated pair, a long read)
    nidx = [i for i, (p, t) in enumerate(pairs) if "N" in p]
    pairs[1], pairs[nidx[5]] = pairs[nidx[5]], pairs[1]
    pairs[7], pairs[nidx[6]] = pairs[nidx[6]], pairs[7]
    pairs[4] = (_rnd(120), _rnd(140))
    pairs[11] = _gen(1, 950, 0.06, 7105)[0]
    assert len(pairs) == 4097 and all(5 <= min(len(p), len(t)) and max(len(p), len(t)) <= 1000 for p, t in pairs)
    return pairs


SHORT = _short_pool()
LONG = [_gen(1, L, e, 7200 + i)[0] for i, (L, e) in enumerate([(1200, 0.02), (1500, 0.05), (1300, 0.1), (1450, 0.03),
                                                               (1100, 0.08), (1500, 0.01), (1250, 0.04), (1400, 0.06)])]
UNION = SHORT + LONG
UBATCH = datagen.from_strings([p for p, _ in UNION], [t for _, t in UNION])
NS = len(SHORT)
LONG_IDX = list(range(NS, NS + len(LONG)))
# batches on both sides of every size switch (general-kernel tiny form 16 / 17, tiny plan of the batch run 128 / 129, the small-batch
# form of align_batch 1 024 / 1 025, banded tiny form 4 096 / 4 097); 1 024 / 1 025 / 4 097 carry the long reads
SIZES = (16, 17, 128, 129, 1024, 1025, 4096, 4097)
IDX = {n: (list(range(n)) if n in (16, 17, 128, 129, 4096) else list(range(n - len(LONG))) + LONG_IDX) for n in SIZES}
BATCH = {n: datagen.subset(UBATCH, IDX[n]) for n in SIZES}
STRS = {n: ([UNION[i][0] for i in IDX[n]], [UNION[i][1] for i in IDX[n]]) for n in SIZES}

# single pairs (every read >= the largest free end); the register stages hand the long / divergent ones on
SINGLES = [SHORT[0], SHORT[1], SHORT[4], LONG[1], LONG[2], _gen(1, 600, 0.12, 7300)[0], (_rnd(300), _rnd(280)),
           _n_pair(200), ("ACGTACGTAC", "ACGTACGTAC"), _gen(1, 1000, 0.05, 7301)[0]]
SBATCH = datagen.from_strings([p for p, _ in SINGLES], [t for _, t in SINGLES])
# edge cases (empty, length 1, ...), only in states without free ends
_special = vo.corpus_special(seed=11)
SPECIAL = [datagen.pair_strings(_special, i) for i in range(min(200, len(_special["p_len"])))]
SPECIAL = [(p.upper(), t.upper()) for p, t in SPECIAL]
SPBATCH = datagen.from_strings([p for p, _ in SPECIAL], [t for _, t in SPECIAL])


def _reads():
    """24 reads of 40 - 300 bases for score_matrix / nearest: families, an unrelated read, reads with N."""
    out = []
    for _ in range(5):
        f = _rnd(int(_rng.integers(40, 300)))
        out += [f] + [_mutate(f, 0.04) for _ in range(3)]
    out += [_rnd(150), _n_pair(120)[0], _n_pair(90)[1], _rnd(40)]
    assert len(out) == 24 and min(map(len, out)) >= 5
    return out


READS = _reads()
MBATCH = datagen.from_strings([READS[i] for i in range(24) for _ in range(24)], [READS[j] for _ in range(24) for j in range(24)])


# ------------------------------------------------------------------------------------------------------------- the oracle
_ORACLE = {}


def oracle(kw, which):
    """The oracle's results for configuration ``kw`` on an input set, cached: "singles", "union", "special", "matrix" (scope score)."""
    key = (tuple(sorted(full_kw(kw).items(), key=lambda x: x[0])), which)
    if key not in _ORACLE:
        ckw = dict(kw, scope="score") if which == "matrix" else kw
        oc, _ = common.configs_pair(**ckw)
        batch = {"singles": SBATCH, "union": UBATCH, "special": SPBATCH, "matrix": MBATCH}[which]
        _ORACLE[key] = loader.run(loader.oracle(), oc, batch)
    return _ORACLE[key]


def expected(kw, entry, size):
    full = full_kw(kw)["scope"] == "full"
    if entry in ("score_matrix", "nearest"):
        o = oracle(kw, "matrix")
        score, status = o["score"].reshape(24, 24), o["status"].reshape(24, 24)
        if entry == "score_matrix":
            return {"score": score, "status": status}
        rj, rs = ref_topk(score, status, 3)
        return {"j": rj, "score": rs}
    if entry == "wavefront_align":
        o = oracle(kw, "singles")
        return {"score": o["score"], "status": o["status"], "cigars": o["cigars"] if full else None}
    if size == "special":
        o = oracle(kw, "special")
        return {"score": o["score"], "status": o["status"], "cigars": o["cigars"] if full else None}
    o = oracle(kw, "union")
    idx = IDX[size]
    return {"score": o["score"][idx], "status": o["status"][idx], "cigars": [o["cigars"][i] for i in idx] if full else None}


def ref_topk(score, status, k):
    """All-vs-all top-k of a score matrix (as tests/test_cross_topk_gpu.py): status-0 cells, j != i, by (-score, j), padded."""
    m = score.shape[0]
    rj = np.full((m, k), -1, np.int32)
    rs = np.full((m, k), INT32_MIN, np.int32)
    for i in range(m):
        ok = status[i] == 0
        ok[i] = False
        cols = np.nonzero(ok)[0]
        sel = cols[np.lexsort((cols, -score[i, cols].astype(np.int64)))][:k]
        rj[i, :len(sel)] = sel
        rs[i, :len(sel)] = score[i, sel]
    return rj, rs


# ------------------------------------------------------------------------------------------------------------- entry points
_CODE_CHARS = np.frombuffer(b"MIDNSHP=XB", np.uint8)


def _rle_ops(off, code, rlen, n):
    return [np.repeat(_CODE_CHARS[code[off[i]:off[i + 1]]], rlen[off[i]:off[i + 1]]).tobytes() for i in range(n)]


def run_entry(a, entry, size):
    """Call one entry point of the Python aligner ``a``; returns its results in the form of ``expected``."""
    full = a.scope == "full"
    if entry == "wavefront_align":
        score, status, cig = [], [], []
        for p, t in SINGLES:
            score.append(a.wavefront_align(t, p))
            status.append(a.status)
            cig.append(a.cigarstring)
        return {"score": np.array(score, np.int32), "status": np.array(status, np.int32), "cigars": cig if full else None}
    if entry == "score_matrix":
        score, status = a.score_matrix(READS)
        return {"score": score, "status": status}
    if entry == "nearest":
        r = a.nearest(READS, k=3)
        return {"j": r["j"], "score": r["score"]}
    if entry == "wavefront_align_batch":
        pats, txts = (list(x) for x in zip(*SPECIAL)) if size == "special" else STRS[size]
        out = a.wavefront_align_batch(txts, pats)
        return {"score": out["score"], "status": out["status"],
                "cigars": [bytes(o) for o in out["cigar_ops"]] if full else None}
    batch = BATCH[size]
    n = len(batch["p_len"])
    if entry == "align_batch":
        out = a.align_batch(batch)
        return {"score": out["score"], "status": out["status"],
                "cigars": [bytes(o) for o in out["cigar_ops"]] if full else None}
    if entry == "align_batch_results":
        res = a.align_batch_results(batch)
        return {"score": res.score, "status": res.status, "cigars": _rle_ops(res.run_off, res.run_code, res.run_len, n),
                "locs": np.asarray(res.locations)}
    if entry == "resident_batch":
        rb = a.resident_batch(batch)
        try:
            rb.run()
            rb.sync()
            score, status, cig = rb.results(full)
        finally:
            rb.close()
        cigars = None
        if full:
            ops, cbeg, clen = cig
            cigars = [ops[cbeg[i]:cbeg[i] + clen[i]].tobytes() for i in range(n)]
        return {"score": score, "status": status, "cigars": cigars}
    raise AssertionError(entry)


def _cigar_form(entry, cigars):
    # (wavefront_align reports the CIGAR string; the oracle's op bytes are compared in that form)
    return [common.rle(c) for c in cigars] if entry == "wavefront_align" else list(cigars)


def _diff(exp, got, entry, oracle_side=True):
    """The first difference between two result dicts (``exp`` the oracle's unless ``oracle_side`` is False), or None."""
    for k in exp:
        if k == "cigars":
            if exp[k] is None or got.get(k) is None:
                if (exp[k] is None) != (got.get(k) is None):
                    return "cigars present on one side only"
                continue
            e, g = _cigar_form(entry, exp[k]) if oracle_side else list(exp[k]), list(got[k])
            bad = [i for i in range(len(e)) if e[i] != g[i]]
            if len(e) != len(g) or bad:
                i = bad[0] if bad else -1
                return f"CIGAR of item {i}: expected {e[i][:80] if bad else len(e)} got {g[i][:80] if bad else len(g)}"
            continue
        ea, ga = np.asarray(exp[k]), np.asarray(got[k])
        if ea.shape != ga.shape or not np.array_equal(ea, ga):
            if ea.shape != ga.shape:
                return f"{k}: shape {ea.shape} vs {ga.shape}"
            i = np.flatnonzero((ea != ga).ravel())
            return f"{k}: {i.size} items differ, first {int(i[0])}: expected {ea.ravel()[i[0]]} got {ga.ravel()[i[0]]}"
    return None


_FRESH = {}


def fresh(state, entry, size):
    """The results of a fresh aligner created in ``state`` (cached)."""
    key = (state, entry, size)
    if key not in _FRESH:
        a = pywfa_amd.WavefrontAligner(**STATES[state])
        try:
            _FRESH[key] = run_entry(a, entry, size)
        finally:
            a.close()
    return _FRESH[key]


def check(a, state, entry, size, ctx):
    """``a`` (moved to ``state``) on one entry point equals the oracle of ``state``, and a fresh aligner created in ``state``."""
    kw = STATES[state] if isinstance(state, str) else state
    got = run_entry(a, entry, size)
    d = _diff(expected(kw, entry, size), got, entry)
    if d is not None:
        note = ""
        if isinstance(state, str):
            fd = _diff(expected(kw, entry, size), fresh(state, entry, size), entry)
            note = " (a fresh aligner in this state agrees with the oracle: state leaked from the previous configuration)" \
                if fd is None else f" (a fresh aligner in this state is wrong too: {fd})"
        raise AssertionError(f"{ctx}: {entry} size={size}: {d}{note}")
    if isinstance(state, str):
        f = fresh(state, entry, size)
        assert _diff(f, got, entry, oracle_side=False) is None and (("locs" not in f) or np.array_equal(f["locs"], got["locs"])), \
            f"{ctx}: {entry} size={size}: differs from a fresh aligner in {state}"


def entry_points(kw, sizes_of):
    """(entry, size) of every entry point for configuration ``kw``; ``sizes_of(entry)`` picks the batch sizes."""
    full = full_kw(kw)["scope"] == "full"
    out = [("wavefront_align", None)]
    for entry in ("wavefront_align_batch", "align_batch", "align_batch_results", "resident_batch"):
        if entry == "align_batch_results" and not full:
            continue
        out += [(entry, n) for n in sizes_of(entry)]
    if not has_free(kw):
        out.append(("wavefront_align_batch", "special"))
    out += [("score_matrix", None), ("nearest", None)]
    return out


# ------------------------------------------------------------------------------------------------------------- transitions
def _first_call(a):
    a.wavefront_align(SINGLES[0][1], SINGLES[0][0])


@pytest.mark.parametrize("src", NAMES)
def test_every_transition_single_pairs_and_tiny_batches(gpu, src):
    """Every ordered pair (src, dst): singles and the 16 / 17-pair batches (with WFA_TEST_FULL=1: every entry point at every size)."""
    for dst in NAMES:
        if dst == src:
            continue
        a = pywfa_amd.WavefrontAligner(**STATES[src])
        try:
            _first_call(a)
            move(a, STATES[dst])
            ctx = f"{src} -> {dst}"
            if FULL:
                todo = entry_points(STATES[dst], lambda e: SIZES)
            else:
                todo = [("wavefront_align", None), ("wavefront_align_batch", 16), ("wavefront_align_batch", 17)]
            for entry, size in todo:
                check(a, dst, entry, size, ctx)
            assert_native_config(a._native, STATES[dst])
        finally:
            a.close()


def _covering_walk():
    """A walk through the states in which every state is entered from at least three predecessors, among them a state with a mapped
    score (score_mode 1 / 2) and a LIN state."""
    walk = [NAMES[0]]
    for i, dst in enumerate(NAMES):
        sm = [s for s in SCORE_MODE if s != dst][i % 2]
        lin = [s for s in LIN if s != dst][i % 2]
        other = [s for s in NAMES if s not in (dst, sm, lin)][(5 * i + 3) % (len(NAMES) - 3)]
        for pred in (sm, lin, other):
            if walk[-1] != pred:
                walk.append(pred)
            walk.append(dst)
    return walk


def test_covering_walk_every_entry_point(gpu):
    """One aligner along a covering walk: every entry point, batches on both sides of every size switch, resident batches, score
    matrices and top-k against the oracle of each state it is moved to."""
    walk = _covering_walk()
    seen = {}
    for s, d in zip(walk, walk[1:]):
        seen.setdefault(d, set()).add(s)
    assert all(len(seen[d]) >= 3 for d in NAMES)
    sizes = {"wavefront_align_batch": SIZES, "align_batch": (16, 1024, 1025), "align_batch_results": (128, 129, 4097),
             "resident_batch": (128, 129, 4096)}
    a = pywfa_amd.WavefrontAligner(**STATES[walk[0]])
    try:
        _first_call(a)
        for prev, dst in zip(walk, walk[1:]):
            move(a, STATES[dst])
            for entry, size in entry_points(STATES[dst], (lambda e: SIZES) if FULL else sizes.get):
                check(a, dst, entry, size, f"walk {prev} -> {dst}")
            assert_native_config(a._native, STATES[dst])
    finally:
        a.close()


@pytest.mark.parametrize("src", NAMES)
def test_c_abi_set_config_every_transition(gpu, src):
    """_native.Aligner.set_config on every ordered pair: get_config reads the target back, single pairs and a 17-pair batch equal its
    oracle."""
    _, nsrc = common.configs_pair(**STATES[src])
    for dst in NAMES:
        if dst == src:
            continue
        oc, nc = common.configs_pair(**STATES[dst])
        full = oc.scope == 1
        al = _native.Aligner(nsrc)
        try:
            p, t = SINGLES[0]
            al.align_pair(p.encode(), t.encode(), nsrc.scope == 1)
            al.set_config(nc)
            assert_native_config(al, STATES[dst])
            o = oracle(STATES[dst], "singles")
            for i, (p, t) in enumerate(SINGLES):
                score, status, ops = al.align_pair(p.encode(), t.encode(), full)
                assert (score, status) == (o["score"][i], o["status"][i]), (src, dst, i)
                if full:
                    assert ops == o["cigars"][i], (src, dst, i, common.rle(ops), common.rle(o["cigars"][i]))
            score, status, cig = al.align_batch(BATCH[17], full)
            cigars = [cig[0][cig[1][i]:cig[1][i] + cig[2][i]].tobytes() for i in range(17)] if full else None
            common.assert_same(expected(STATES[dst], "align_batch", 17), score, status, cigars, BATCH[17], f"C ABI {src} -> {dst}")
        finally:
            al.close()


def _multi_walk():
    walk = [NAMES[0]]
    for i, dst in enumerate(NAMES):
        pred = (SCORE_MODE + LIN)[i % 6]
        if pred == dst:
            pred = "affine"
        if walk[-1] != pred:
            walk.append(pred)
        walk.append(dst)
    return walk


def _multi_check(out, kw, size, ctx, full):
    cigars = [bytes(o) for o in out[2]] if full else None
    common.assert_same(expected(kw, "align_batch", size), out[0], out[1], cigars, BATCH[size], ctx)


def test_multi_aligner_walks(gpu):
    """The multi-device entry (two aligners on device 0 on a one-GPU box, as test_multi_device_entry_shards_and_merges), moved along a
    covering walk: through _native.MultiAligner.set_config, and through the setters of WavefrontAligner(devices=...)."""
    walk = _multi_walk()
    _, nc0 = common.configs_pair(**STATES[walk[0]])
    m = _native.MultiAligner(nc0, [0, 0])
    try:
        m.align_batch(BATCH[17], nc0.scope == 1)
        for prev, dst in zip(walk, walk[1:]):
            oc, nc = common.configs_pair(**STATES[dst])
            m.set_config(nc)
            for size in (17, 1025):
                score, status, cig = m.align_batch(BATCH[size], oc.scope == 1)
                ops = [cig[0][cig[1][i]:cig[1][i] + cig[2][i]] for i in range(len(score))] if cig is not None else None
                _multi_check((score, status, ops), STATES[dst], size, f"MultiAligner {prev} -> {dst}", oc.scope == 1)
    finally:
        m.close()
    a = pywfa_amd.WavefrontAligner(devices=[0, 0], **STATES[walk[0]])
    try:
        _first_call(a)
        a.wavefront_align_batch(*reversed(STRS[17]))
        for prev, dst in zip(walk, walk[1:]):
            move(a, STATES[dst])
            for size in (17, 1025):
                check(a, dst, "wavefront_align_batch", size, f"devices=[0, 0] {prev} -> {dst}")
            check(a, dst, "wavefront_align", None, f"devices=[0, 0] {prev} -> {dst}")
    finally:
        a.close()


def test_single_pairs_without_the_mailbox(gpu, monkeypatch):
    """WFA_HIP_MAILBOX=0 (read when the aligner is created): the launch-per-call tiny path, on a walk through the LIN and score-mapped
    states."""
    monkeypatch.setenv("WFA_HIP_MAILBOX", "0")
    walk = ["affine", "lev-score", "lev-full", "match-1", "lev-full", "indel-full", "match-1-score", "linear-full", "lev-score",
            "indel-score", "linear-match-1", "indel-full", "affine-e2e-score", "lev-full", "affine"]
    a = pywfa_amd.WavefrontAligner(**STATES[walk[0]])
    try:
        _first_call(a)
        for prev, dst in zip(walk, walk[1:]):
            move(a, STATES[dst])
            check(a, dst, "wavefront_align", None, f"no mailbox {prev} -> {dst}")
            check(a, dst, "wavefront_align_batch", 16, f"no mailbox {prev} -> {dst}")
    finally:
        a.close()


# ------------------------------------------------------------------------------------------------------------- refused setters
def refusals(kw):
    """(property, value, exception) that the library must refuse in configuration ``kw``."""
    k = full_kw(kw)
    out = [("scope", "half", ValueError), ("distance", "hamming", NotImplementedError)]
    if k["distance"] in ("linear", "affine", "affine2p"):
        out.append(("mismatch_penalty", 0, ValueError))
    if k["distance"] in ("levenshtein", "indel"):
        out.append(("heuristic", "X-drop", ValueError))
    elif k["heuristic"] == "X-drop":
        out.append(("distance", "levenshtein", ValueError))
    free_begins = k["span"] == "ends-free" and (k["pattern_begin_free"] or k["text_begin_free"])
    if k["distance"] != "indel" and k["distance"] != "levenshtein" and k["scope"] == "full":
        if free_begins and k["match"] == 0:
            out.append(("match_score", -1, NotImplementedError))
        if k["match"] < 0 and not free_begins:
            out.append(("pattern_begin_free", 5, NotImplementedError))
    if has_free(kw):
        out.append(("memory_mode", "biwfa", NotImplementedError))
    if k["memory_mode"] == "biwfa":
        out.append(("text_end_free", 5, NotImplementedError))
    return out


@pytest.mark.parametrize("state", NAMES)
def test_refused_setters_leave_the_configuration(gpu, state):
    """Settings the library refuses raise, the getter keeps the old value, and the next calls — single pairs on the aligner, batches
    through the multi-device entry — still equal the oracle of the unchanged state.  max_steps is pushed and taken back."""
    kw = STATES[state]
    a = pywfa_amd.WavefrontAligner(devices=[0, 0], **kw)
    try:
        _first_call(a)
        for prop, value, exc in refusals(kw):
            old = getattr(a, prop)
            with pytest.raises(exc):
                setattr(a, prop, value)
            assert getattr(a, prop) == old, (state, prop)
        assert_native_config(a._native, kw)
        for entry, size in (("wavefront_align", None), ("wavefront_align_batch", 17), ("wavefront_align_batch", 1025)):
            check(a, state, entry, size, f"{state} after refused setters")
        # the step limit: set, then taken back to none
        if full_kw(kw)["max_steps"] == 0:
            a.max_steps = 25
            assert a.max_steps == 25
            for entry, size in (("wavefront_align", None), ("wavefront_align_batch", 17)):
                check(a, dict(kw, max_steps=25), entry, size, f"{state} + max_steps=25")
            a.max_steps = 0
            assert a.max_steps == _INT_MAX
            check(a, state, "wavefront_align_batch", 17, f"{state} after max_steps=0")
    finally:
        a.close()


# ------------------------------------------------------------------------------------------------------------- the wildcard
WILD_ENTRIES = [("align_batch", 129), ("align_batch", 1025), ("align_batch_results", 129), ("resident_batch", 129),
                ("score_matrix", None), ("nearest", None), ("wavefront_align", None), ("wavefront_align_batch", 17)]


@pytest.mark.parametrize("entry,size", WILD_ENTRIES)
def test_wildcard_setter_reaches_every_entry_point(gpu, entry, size):
    """The wildcard set and cleared through its setter is what the next call uses, whichever entry point comes first — also when a
    refused setter came in between."""
    pairs = SINGLES if entry == "wavefront_align" else [(r, r) for r in READS] if size is None else list(zip(*STRS[size]))
    assert any("N" in p + t for p, t in pairs)
    a = pywfa_amd.WavefrontAligner()
    try:
        _first_call(a)
        a.wildcard = "N"
        assert a.wildcard == "N"
        check(a, "wildcard", entry, size, "wildcard set")
        a.wildcard = None
        check(a, "affine", entry, size, "wildcard cleared")
        a.wildcard = "n"
        with pytest.raises(ValueError):
            a.mismatch_penalty = 0
        check(a, "wildcard", entry, size, "wildcard set, then a refused setter")
    finally:
        a.close()


# ------------------------------------------------------------------------------------------------------------- run-time path failure
def test_run_time_path_failure_across_reconfiguration(gpu, monkeypatch):
    """WFA_HIP_RTC_FAIL=1 (every run-time compile fails): a walk from a run-time penalty shape to a built-in one, back, and on to LIN
    and score-mapped states.  (The shape 5/4/3 is used by no other test, so that its compile is attempted in this process.)"""
    monkeypatch.setenv("WFA_HIP_RTC_FAIL", "1")
    rtc = dict(mismatch=5, gap_opening=4, gap_extension=3)
    walk = [rtc, {}, rtc, STATES["lev-full"], dict(rtc, scope="score"), STATES["match-1"], rtc]
    a = pywfa_amd.WavefrontAligner(**walk[0])
    try:
        _first_call(a)
        for i, kw in enumerate(walk):
            if i:
                move(a, kw)
            for entry, size in (("wavefront_align", None), ("wavefront_align_batch", 17), ("wavefront_align_batch", 129),
                                ("wavefront_align_batch", 1025), ("resident_batch", 4097)):
                check(a, kw, entry, size, f"rtc failure, step {i} {kw}")
    finally:
        a.close()
