"""Registry of the configurations the GPU tests hand the oracle (test infrastructure).

Almost every GPU test asserts "HIP == oracle", so the oracle has to be compared with the real library on every configuration those
tests use.  This module collects them from the module-level lists of the GPU test modules (by importing them: none needs a GPU to
import), applies what the test itself adds to a row (a scope, `memory_mode="biwfa"`, ...), attaches the batch shapes of that test
reduced to their smallest form (the read lengths of the test, at most a few hundred pairs; 2-6 pairs for the long reads) and merges
rows that `loader.make_config` maps to the same fields.  tests/test_oracle_grid_vs_ref.py runs oracle against reference over it.

SOURCES names every list that is collected; WAIVED names the configuration lists of those modules that never reach the oracle, with
the reason.  A configuration list in one of MODULES that is in neither makes the coverage test fail.  Configurations written inside
test functions are read from the modules' source (literal_configs): one that agrees with no collected row gets an entry of its own.
"""
import ast
import functools
import hashlib
import importlib
import inspect

import numpy as np

import common
import corpus_common
from oracle import loader
from pywfa_amd import datagen

PARAMS = tuple(inspect.signature(loader.make_config).parameters)
FIELDS = tuple(n for n, _ in loader.Config._fields_)

MODULES = ("test_parity_gpu", "test_slim_gpu", "test_wide_gpu", "test_biwfa_gpu", "test_cross_gpu", "test_cross_topk_gpu",
           "test_windows_gpu", "test_summary_gpu", "test_reconfigure_gpu", "test_lane_entry_gpu", "test_lane_window_entry_gpu",
           "test_lane_winfin_gpu", "test_int16_range_gpu", "test_optimality_gpu", "test_pipeline_gpu")
# further GPU modules that hand the oracle configurations written inside their functions: no list of theirs is collected, but the
# literals in their source are checked against the registry (literal_configs below)
SCANNED_ONLY = ("test_lane_widths_gpu", "test_lane_probe_gpu", "test_lane_narrow_gpu", "test_baseline_configs_gpu", "test_mailbox_gpu",
                "test_poison_gpu", "test_full_size_gpu")


def key_of(kw):
    """The normalised `loader.make_config` fields of a configuration: what the checkers see."""
    c = loader.make_config(**kw)
    return tuple(getattr(c, n) for n in FIELDS)


def key_name(key):
    """A key as text: the fields that differ from the defaults (ids of the parametrised test, keys of the golden file)."""
    base = key_of({})
    return ",".join(f"{n}={v}" for n, v, d in zip(FIELDS, key, base) if v != d) or "default"


def _null_step_beyond_the_free_begins(kw):
    """match < 0 with equal free begins f: whether some score s = j * (-match) with j > f is a null step, i.e. no wavefront of an
    earlier score can feed it.  From the penalties alone (as the library rescales them under match < 0, R/wavefront_penalties.c):
    scores 0, m, ..., f m are seeded by the free begins; M exists at s if it is seeded or fed by s - x or by a gap component at s;
    a gap component exists at s if M exists at s - o - e or the component at s - e."""
    m, f = -kw["match"], kw.get("pattern_begin_free", 0)
    d = kw.get("distance", "affine")
    x = 2 * kw.get("mismatch", 4) + 2 * m
    if d == "linear":
        gaps = [(0, 2 * kw.get("gap_extension", 2) + m)]
    else:
        gaps = [(2 * kw.get("gap_opening", 6), 2 * kw.get("gap_extension", 2) + m)]
        if d == "affine2p":
            gaps.append((2 * kw.get("gap_opening2", 24), 2 * kw.get("gap_extension2", 1) + m))
    top = f * m + 2 * max([x] + [o + e for o, e in gaps]) + m
    has_m, has_g = [False] * (top + 1), [[False] * (top + 1) for _ in gaps]
    for s in range(top + 1):
        for g, (o, e) in enumerate(gaps):
            has_g[g][s] = (s >= o + e and has_m[s - o - e]) or (o and s >= e and has_g[g][s - e])
        fed = (s >= x and has_m[s - x]) or any(h[s] for h in has_g)
        seeded = s % m == 0 and s // m <= f
        if s % m == 0 and s // m > f and not fed:
            return True
        has_m[s] = seeded or fed
    return False


def reference_undefined(kw):
    """The rows the reference has no defined answer for, both under match < 0 with free begins in an ends-free span:
    unequal free begins — a re-seeded null step whose begin-free cell exists on one side only leaves the cells between diagonal 0
    and that cell unwritten, and later steps read them; equal free begins so short that a null step lies beyond them — that step
    gets lo = hi = 0 and an offsets[0] that is never written (R/wavefront_compute.c:229-251)."""
    pb, tb = kw.get("pattern_begin_free", 0), kw.get("text_begin_free", 0)
    if kw.get("match", 0) >= 0:
        return False
    if pb != tb:
        return True
    return (pb > 0 and kw.get("span", "ends-free") == "ends-free" and kw.get("distance", "affine") not in ("indel", "levenshtein")
            and _null_step_beyond_the_free_begins(kw))


# ---------------------------------------------------------------------------------------------------------------- shapes
# A shape is a tuple: its first item names the builder, the tuple itself is the cache key and the label.
PARITY_SHAPES = tuple(("parity", name) for name in ("150bp_2pct", "150bp_15pct", "1kb_8pct"))


def _pairs(pats, txts):
    return datagen.from_strings(list(pats), list(txts), upper=True)


def _with_n(batch):
    """Every third pair gets an N: in the pattern, in the text, a run in both."""
    pats, txts = [], []
    for i in range(len(batch["p_len"])):
        p, t = datagen.pair_strings(batch, i)
        if i % 3 == 0 and len(p) > 20 and len(t) > 20:
            k = (7 * i) % (min(len(p), len(t)) - 4)
            if i % 9 == 0: p = p[:k] + "N" + p[k + 1:]
            elif i % 9 == 3: t = t[:k] + "N" + t[k + 1:]
            else: p = p[:k] + "NN" + p[k + 2:]; t = t[:k + 1] + "N" + t[k + 2:]
        pats.append(p); txts.append(t)
    return _pairs(pats, txts)


@functools.lru_cache(maxsize=None)
def build_shape(shape):
    kind = shape[0]
    if kind == "parity":       # the corpora of tests/test_parity_gpu.py, same sizes and seeds
        import test_parity_gpu as tp
        n, L, e = tp.SHAPES[shape[1]]
        return datagen.generate(n, L, e, 7000 + L + int(e * 1000))
    if kind == "gen":
        return datagen.generate(*shape[1:])
    if kind == "gen_n":
        return _with_n(datagen.generate(*shape[1:]))
    if kind == "ragged":       # corpus_common.ragged_batch (tests/test_wide_gpu.py)
        return corpus_common.ragged_batch(*shape[1:])
    if kind == "slim_ragged":  # tests/test_slim_gpu.py ragged(seed, n, lmin, lmax, err, indel_bias)
        import test_slim_gpu as ts
        return ts.ragged(*shape[1:])
    if kind == "hands_on":     # short unrelated pairs, prefixes, overhangs (tests/test_wide_gpu.py)
        rng = np.random.default_rng(4242)
        alpha = np.frombuffer(b"ACGT", np.uint8)
        pats, txts = [], []
        for i in range(shape[1]):
            pl = int(rng.integers(65, 260))
            p = alpha[rng.integers(0, 4, pl)]
            t = (alpha[rng.integers(0, 4, int(rng.integers(65, 260)))], p[:int(rng.integers(40, pl + 1))],
                 np.concatenate([alpha[rng.integers(0, 4, int(rng.integers(0, 40)))], p]), p[::-1])[i % 4]
            pats.append(p.tobytes().decode()); txts.append(t.tobytes().decode())
        return _pairs(pats, txts)
    if kind == "cross":        # pairs of the read families of tests/test_cross*_gpu.py (reads of 0-300 bases, two empty)
        import test_cross_topk_gpu as tk
        reads = tk.READS_NE if shape[1] else tk.READS
        a, b = reads[:14], reads[14:28]
        return _pairs([p for p in a for _ in b], [t for _ in a for t in b])
    if kind == "cross_oracle": # tests/test_cross_gpu.py test_against_oracle: all-vs-all over reads of 0-200 bases
        import test_cross_gpu as tc
        reads = tc.families(21, 8, 6, 0, 200)[:shape[1]]
        return _pairs([p for p in reads for _ in reads], [t for _ in reads for t in reads])
    if kind == "short_divergent":   # tests/test_biwfa_gpu.py: unrelated reads of 40-100 bases, a repeat, an empty pattern
        rng = np.random.default_rng(5)
        pats = ["".join(rng.choice(list("ACGT"), size=int(rng.integers(40, 101)))) for _ in range(shape[1])]
        txts = ["".join(rng.choice(list("ACGT"), size=int(rng.integers(40, 101)))) for _ in range(shape[1])]
        return _pairs(pats + ["ACGT" * 20, ""], txts + ["ACGT" * 20, "ACGTACGT"])
    if kind == "windows":      # reads of tests/test_windows_gpu.py against the windows they were cut from, either strand
        import test_windows_gpu as tw
        pats, txts = [], []
        for read, (r, pos, n, rev) in list(zip(tw.READS, tw.ORIGIN))[:shape[1]]:
            pats.append(tw.revcomp(read) if rev else read)
            txts.append(tw.REFS[r][max(0, pos - 5):pos + n + 5])
        return _pairs(pats, txts)
    if kind == "summary":      # tests/test_summary_gpu.py: ACGT-only pairs and the pairs that hold an N
        import test_summary_gpu as tsu
        pats, txts = tsu.PAIRS[shape[1]]
        pick = list(range(len(pats))) if shape[1] == "long" else list(range(120)) + list(range(tsu.N_PURE["short"], len(pats)))
        return _pairs([pats[i] for i in pick], [txts[i] for i in pick])
    if kind == "reconfigure":  # the edge-case pairs of tests/test_reconfigure_gpu.py (free ends of up to 5: pairs that long only)
        import test_reconfigure_gpu as tr
        sel = [(p, t) for p, t in tr.SPECIAL if not shape[1] or (len(p) >= 5 and len(t) >= 5)]
        return _pairs([p for p, _ in sel], [t for _, t in sel])
    if kind == "lane_edges":   # the constructed pairs of tests/test_lane_entry_gpu.py
        import test_lane_entry_gpu as tle
        return tle.edge_pairs()
    if kind == "int16_len":    # tests/int16_common.py: four pairs of exactly L bases with the work at their end
        import int16_common
        return int16_common.length_batch(shape[1], 3100 + shape[1] % 100)
    if kind == "pipeline":     # tests/pipeline_common.py: 300 listed windows, the rescue windows, the long reads' chain windows
        import pipeline_common as pc
        from test_windows_gpu import materialise
        if shape[1] == 2:
            reads, W = pc.long_reads()[0], pc.as_rig_list(pc.expected_long()["w"], [len(r) for r in pc.long_reads()[0]])
        else:
            reads, e = pc.corpus()[0], pc.expected_placement()
            lens = [len(r) for r in reads]
            W = pc.as_rig_list({k: v[:300] for k, v in e["w"].items()}, lens) if shape[1] == 0 else pc.as_rig_list(dict(e["rescue"], text_start=e["rescue"]["text_start"], text_len=e["rescue"]["text_len"]), lens)
        return _pairs(*materialise(reads, pc.genome()[0], W))
    if kind == "biwfa_levels": # tests/test_biwfa_gpu.py, the level-queue test: 3 kb, 700 and 90 bases
        return _pairs(*zip(*[datagen.pair_strings(b, i) for b in (datagen.generate(3, 3000, 0.10, 99), datagen.generate(20, 700, 0.15, 98),
                                                                   datagen.generate(20, 90, 0.1, 97)) for i in range(len(b["p_len"]))]))
    raise KeyError(shape)


def build_optimality(name, kw):
    """Corpora of tests/test_optimality_gpu.py depend on the configuration (pairs shorter than the free ends are dropped)."""
    import test_optimality_gpu as to
    return to.corpus(name, kw)


# --------------------------------------------------------------------------------------------------------------- sources
def _same(i, item): return [item]
def _scoped(**extra): return lambda i, item: [dict(item, scope=s, **extra) for s in ("full", "score")]
def _with(**extra): return lambda i, item: [dict(item, **extra)]
def _under(**base): return lambda i, item: [dict(base, **item)]
def _named(i, item): return [item[1]]
def _named_score(i, item): return [dict(item[1], scope="score")]


def _summary(i, item):
    import test_summary_gpu as tsu
    return [tsu.config_for(item[0], item[1], kind) for kind in ("short", "long")]


def _summary_shapes(i, item, kw):
    import test_summary_gpu as tsu
    return [("summary", kind) for kind in ("short", "long") if tsu.config_for(item[0], item[1], kind) == kw]


def _value(i, item): return [item[1]]            # rows of a dict are its (name, value) items


def _lane_shapes_kw(module):
    def expand(i, item):
        return [importlib.import_module(module).config_kw(item[0])]
    return expand


def _pen(pen, **kw):
    return dict(kw, mismatch=pen[0], gap_opening=pen[1], gap_extension=pen[2])


def _banded(i, item):
    import test_parity_gpu as tp
    if isinstance(item, dict):
        return [_pen(pen, **item) for pen in tp.BANDED_PENS]
    return [_pen(item, **kw) for kw in tp.BANDED_KWS]


def _biwfa_steps(i, item):
    import test_biwfa_gpu as tb
    return [dict(item, scope=s, memory_mode="biwfa", max_steps=ms) for ms in tb.STEP_LIMITS for s in ("full", "score")]


BANDED_SHAPES = [("gen", 30, 1500, 0.05, 9500), ("gen", 6, 3000, 0.08, 9501), ("gen", 200, 200, 0.10, 9502)]


def _free(kw):
    return any(kw.get(k, 0) for k in ("pattern_begin_free", "pattern_end_free", "text_begin_free", "text_end_free"))


SHORT = (("gen", 300, 150, 0.04, 6150), ("gen", 200, 150, 0.15, 6151))
# (module, attribute, rows -> configurations, shapes(i, row, kw))
SOURCES = [
    ("test_parity_gpu", "GRID", _same, lambda i, r, kw: PARITY_SHAPES),
    ("test_parity_gpu", "LANE_GENERAL", _with(scope="score"), lambda i, r, kw: PARITY_SHAPES[:2]),
    ("test_parity_gpu", "SEG_XDROP", _with(scope="score"), lambda i, r, kw: PARITY_SHAPES[:2]),
    ("test_parity_gpu", "TENKB", _same, lambda i, r, kw: [("gen", 4, 10000, 0.08, 1003)]),
    ("test_parity_gpu", "PIGGYBACK", lambda i, item: [dict(item, scope="full"), dict(item, scope="full", memory_mode="high")],
     lambda i, r, kw: [("gen", 30, 1500, 0.06, 8800), ("gen", 6, 4000, 0.08, 8801), ("gen", 3, 10000, 0.08, 8802), ("gen", 20, 2500, 0.01, 8803)]),
    ("test_parity_gpu", "PIGGYBACK_2P", _with(distance="affine2p", scope="full"),
     lambda i, r, kw: [("gen", 30, 1500, 0.06, 8900), ("gen", 4, 3000, 0.08, 8901)] +
                      ([("gen", 3, 10000, 0.08, 8902), ("gen", 20, 2500, 0.01, 8903)] if "heuristic" in r else [])),
    ("test_parity_gpu", "SINGLE_CALLS", _same, lambda i, r, kw: [("gen", 64, 150, 0.04, 4711), ("gen_n", 64, 150, 0.04, 4711)]),
    ("test_parity_gpu", "ALIGN_PAIR", _same, lambda i, r, kw: [("gen_n", 40, 150, 0.04, 4712)]),
    ("test_parity_gpu", "WILD", _under(scope="full", wildcard="N"), lambda i, r, kw: [("gen_n", 300, 150, 0.03, 71 + i), ("gen_n", 40, 900, 0.06, 72 + i)]),
    ("test_parity_gpu", "LIN", _with(scope="full"), lambda i, r, kw: [("gen", 300, 150, 0.04, 8800 + i), ("gen", 200, 150, 0.15, 8900 + i)]),
    ("test_parity_gpu", "SEG_PENS", lambda i, item: [_pen(item, span="end-to-end", scope="score")],
     lambda i, r, kw: [("gen", 300, 150, 0.02, 7000), ("gen", 200, 150, 0.2, 7002), ("gen", 100, 480, 0.03, 7003), ("gen", 200, 40, 0.1, 7004)]),
    ("test_parity_gpu", "BANDED_PENS", _banded, lambda i, r, kw: BANDED_SHAPES),
    ("test_parity_gpu", "BANDED_KWS", _banded, lambda i, r, kw: BANDED_SHAPES),
    ("test_slim_gpu", "CONFIGS", _scoped(),
     lambda i, r, kw: [("slim_ragged", 31 + i, 8, 1100, 4000, 0.08, 6), ("gen", 3, 10000, 0.08, 4100 + i), ("slim_ragged", 77 + i, 6, 1200, 9000, 0.03),
                       ("gen", 40, 1500, 0.15, 4200 + i)]),
    ("test_slim_gpu", "EXACT", _scoped(),
     lambda i, r, kw: [("slim_ragged", 500 + i, 60, 520, 1150, 0.06, 3), ("slim_ragged", 600 + i, 60, 200, 700, 0.12), ("gen", 40, 1000, 0.03, 4300 + i)]),
    ("test_slim_gpu", "WINDOWED", _scoped(), lambda i, r, kw: [("gen", 2, 30000, 0.08, 900), ("gen", 2, 45000, 0.02, 901)]),
    ("test_slim_gpu", "OVERFLOW", _value, lambda i, r, kw: [("gen", 3, 6000, 0.12, 515)]),
    ("test_wide_gpu", "CASES", _same, lambda i, r, kw: [("ragged", 12, 2500, 0.10, 9100 + i), ("ragged", 40, 1200, 0.10, 9500 + i), ("gen", 6, 2500, 0.10, 9100 + i)]),   # (ragged: short and empty pairs clamp the free ends, as in the GPU test; gen: room for them)
    ("test_wide_gpu", "ADAPT_CASES", _same, lambda i, r, kw: [("ragged", 30, 2500, 0.10, 9300 + i), ("gen", 12, 2500, 0.10, 9300 + i)]),
    ("test_wide_gpu", "HANDS_ON", _same, lambda i, r, kw: [("hands_on", 200)]),
    ("test_wide_gpu", "BEYOND_16KB", _same, lambda i, r, kw: [("gen", 2, 17000, 0.06, 8801)]),
    ("test_wide_gpu", "MIDLENGTH", lambda i, item: [dict(span="end-to-end", scope=s, distance=item[2]) for s in ("score", "full")],
     lambda i, r, kw: [("gen", 200, r[0], r[1], 131)]),
    ("test_biwfa_gpu", "SHORT_DIVERGENT", _with(scope="full", memory_mode="biwfa"), lambda i, r, kw: [("short_divergent", 120)]),
    ("test_biwfa_gpu", "STEP_KW0", _biwfa_steps,
     lambda i, r, kw: [("gen", 200, 150, 0.05, 21), ("gen", 100, 150, 0.2, 22), ("gen", 20, 1500, 0.08, 24), ("gen", 3, 10000, 0.08, 25)]),
    ("test_biwfa_gpu", "CONFIGS", _with(scope="full", memory_mode="biwfa"),
     lambda i, r, kw: [("gen", 200, 150, 0.2, 3901 + 7 * i), ("gen", 40, 1500, 0.08, 3903 + 7 * i), ("gen", 5, 10000, 0.08, 3905 + 7 * i)]),
    ("test_biwfa_gpu", "LEVEL_KWS", _with(scope="full", memory_mode="biwfa"), lambda i, r, kw: [("biwfa_levels",)]),
    ("test_biwfa_gpu", "BIWFA_HEUR", _scoped(memory_mode="biwfa", span="end-to-end"),
     lambda i, r, kw: [("gen", 150, 150, 0.2, 3901 + 7 * i), ("gen", 30, 1500, 0.08, 3903 + 7 * i), ("gen", 4, 10000, 0.08, 3905 + 7 * i)]),
    ("test_cross_gpu", "ORACLE_KWS", _same, lambda i, r, kw: [("cross_oracle", 16)]),
    ("test_cross_gpu", "GRID", _named_score, lambda i, r, kw: [("cross", _free(kw))]),
    ("test_cross_topk_gpu", "GRID", _named_score, lambda i, r, kw: [("cross", _free(kw))]),
    ("test_windows_gpu", "SCOPED", _named, lambda i, r, kw: [("windows", 160)]),
    ("test_summary_gpu", "CONFIGS", _summary, _summary_shapes),
    ("test_reconfigure_gpu", "STATES", _value, lambda i, r, kw: [("reconfigure", _free(kw))] + list(SHORT[:1])),
    ("test_lane_entry_gpu", "SHAPES", _lane_shapes_kw("test_lane_entry_gpu"), lambda i, r, kw: [("lane_edges",)] + list(SHORT[:1])),
    ("test_lane_window_entry_gpu", "SHAPES", _lane_shapes_kw("test_lane_window_entry_gpu"), lambda i, r, kw: [("lane_edges",)] + list(SHORT[:1])),
    ("test_lane_winfin_gpu", "SHAPES", _lane_shapes_kw("test_lane_winfin_gpu"), lambda i, r, kw: [("lane_edges",)] + list(SHORT[:1])),
    ("test_int16_range_gpu", "KWS", lambda i, item: [dict(item[1], scope=s) for s in ("score", "full")] if "scope" not in item[1] else [item[1]],
     lambda i, r, kw: [("int16_len", 32000)] + ([("int16_len", 16000)] if kw.get("distance") == "affine2p" else [])),
    ("test_optimality_gpu", "HEUR", lambda i, item: [dict(item[1], scope="full")], lambda i, r, kw: [("optimality", r[0])]),
    ("test_pipeline_gpu", "ORACLE_KWS", _same, lambda i, r, kw: [("pipeline", i)]),
]

# configuration lists of MODULES that never reach the oracle
WAIVED = {
    ("test_optimality_gpu", "EXACT"): "exact families: checked against the dynamic-programming recurrence (tests/dp_reference.py), not the oracle",
    ("test_optimality_gpu", "LONG"): "exact families: checked against the dynamic-programming recurrence, not the oracle",
    ("test_optimality_gpu", "ENTRY_KW"): "exact families: checked against the dynamic-programming recurrence, not the oracle",
}


def rows_of(module, attr):
    """The rows of a collected list; a dict gives its (name, value) items."""
    obj = getattr(importlib.import_module(module), attr)
    return list(obj.items()) if isinstance(obj, dict) else list(obj)


def _is_config(d):
    return isinstance(d, dict) and set(d) <= set(PARAMS)


def config_lists(module):
    """Names of the module-level lists / dicts of `module` whose rows are configurations (or (name, configuration) pairs)."""
    out = []
    mod = importlib.import_module(module)
    for name, obj in vars(mod).items():
        if name.startswith("_") or not isinstance(obj, (list, tuple, dict)) or not obj or _is_config(obj):
            continue
        rows = list(obj.values()) if isinstance(obj, dict) else list(obj)
        cfgs = [r[1] if isinstance(r, tuple) and len(r) == 2 and isinstance(r[0], str) else r for r in rows]
        if all(c is None or _is_config(c) for c in cfgs) and any(isinstance(c, dict) for c in cfgs):
            out.append((name, obj))
    return out


def is_declared(obj):
    """Whether a configuration list is collected (SOURCES) or waived with a reason (WAIVED), under whichever module it is defined in."""
    return any(getattr(importlib.import_module(m), a) is obj for m, a in [s[:2] for s in SOURCES] + list(WAIVED))


@functools.lru_cache(maxsize=None)
def already_pinned():
    """Keys of the BiWFA configurations tests/test_oracle_vs_ref.py compares with the library (in its ultralow mode)."""
    import test_oracle_vs_ref as tov
    keys = set()
    for kw in tov.BIWFA:
        keys.add(key_of(dict(kw, scope="score", memory_mode="biwfa")))
    for kw in tov.BIWFA_FULL:
        keys.add(key_of(dict(kw, scope="full", memory_mode="biwfa")))
    for kw in tov.BIWFA_HEUR:
        for scope in ("full", "score"):
            keys.add(key_of(dict(kw, scope=scope, memory_mode="biwfa", span="end-to-end")))
    return frozenset(keys)


@functools.lru_cache(maxsize=None)
def registry():
    """name -> entry(kw, key, shapes, sources, biwfa, pinned_elsewhere, undefined), one per distinct configuration."""
    entries = {}
    for module, attr, expand, shapes in SOURCES:
        for i, row in enumerate(rows_of(module, attr)):
            for kw in expand(i, row):
                key = key_of(kw)
                e = entries.setdefault(key, dict(kw=dict(kw), key=key, name=key_name(key), shapes=[], sources=[]))
                e["sources"].append(f"{module}.{attr}[{i}]")
                for s in shapes(i, row, kw):
                    if s not in e["shapes"]:
                        e["shapes"].append(s)
    # configurations written inside test functions that agree with no collected row: entries of their own (both scopes where the
    # literal leaves the scope open), on generic short and 1.5 kb batches
    for module in MODULES + SCANNED_ONLY:
        for _, partial in literal_configs(module):
            if matches(partial, entries.values()):
                continue
            for kw in ([partial] if "scope" in partial else [dict(partial, scope=sc) for sc in ("score", "full")]):
                key = key_of(kw)
                e = entries.setdefault(key, dict(kw=dict(kw), key=key, name=key_name(key), shapes=list(SHORT) + [("gen", 20, 1500, 0.08, 6152)], sources=[]))
                e["sources"].append(f"{module}: literal {sorted(partial.items())}")
    for e in entries.values():
        e["biwfa"] = e["kw"].get("memory_mode") == "biwfa"
        e["pinned_elsewhere"] = e["key"] in already_pinned()
        e["undefined"] = reference_undefined(e["kw"])
    return {e["name"]: e for e in entries.values()}


def batch_of(shape, kw):
    return build_optimality(shape[1], kw) if shape[0] == "optimality" else build_shape(shape)


# ------------------------------------------------------------------------------------- configurations written inside functions
CONFIG_CALLS = ("dict", "configs_pair", "make_config")


def literal_configs(module):
    """(line, partial configuration) of every `dict(...)`, `configs_pair(...)` and `make_config(...)` call in the source of `module`
    whose named keywords are all `make_config` parameters: the keywords with literal values (a `scope=scope` is left out)."""
    mod = importlib.import_module(module)
    out = []
    for node in ast.walk(ast.parse(inspect.getsource(mod))):
        if not isinstance(node, ast.Call):
            continue
        name = node.func.id if isinstance(node.func, ast.Name) else node.func.attr if isinstance(node.func, ast.Attribute) else None
        named = [k for k in node.keywords if k.arg is not None]
        if name not in CONFIG_CALLS or not named or not all(k.arg in PARAMS for k in named):
            continue
        kw = {}
        for k in named:
            try:
                kw[k.arg] = ast.literal_eval(k.value)
            except ValueError:
                pass
        try:
            loader.make_config(**kw)
        except (KeyError, TypeError, AttributeError):
            continue   # (values no configuration can hold: a table that merely shares the parameter names)
        if kw:
            out.append((node.lineno, kw))
    return out


def matches(partial, entries):
    """Whether one of `entries` has, field for field, the values `partial` names (the fields it leaves open may be anything)."""
    c = loader.make_config(**partial)
    want = [(FIELDS.index(p), getattr(c, p)) for p in partial]
    return any(all(e["key"][i] == v for i, v in want) for e in entries)


def matches_an_entry(partial):
    return matches(partial, registry().values())


def reference_refuses(kw):
    """Configurations the library answers with exit(): BiWFA with free ends, X-drop under indel / levenshtein."""
    free = any(kw.get(k, 0) for k in ("pattern_begin_free", "pattern_end_free", "text_begin_free", "text_end_free"))
    return (kw.get("memory_mode") == "biwfa" and free) or (kw.get("heuristic") == "X-drop" and kw.get("distance") in ("indel", "levenshtein"))


# literals of those modules that never reach the oracle: (module, sorted items) -> reason
WAIVED_LITERALS = {}


# ----------------------------------------------------------------------------------------------------- recorded results
@functools.lru_cache(maxsize=None)
def special():
    """(corpus_special(seed=99), its 64-pair extract)"""
    import validate_oracle as vo
    sp = vo.corpus_special(seed=99)
    return sp, corpus_common.special_mini(sp)


def digest(r):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(r["status"], np.int32).tobytes())
    h.update(np.ascontiguousarray(r["score"], np.int32).tobytes())
    if r["cigars"] is not None:
        h.update(b"\n".join(r["cigars"]))
    return h.hexdigest()


def mini_config(e):
    mini = special()[1]
    return loader.make_config(**common.clamp_free(e["kw"], mini)), mini
