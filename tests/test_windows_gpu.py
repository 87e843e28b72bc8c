"""Windowed batches on the GPU (wfa_hip_batch_create_windows, WavefrontAligner.align_windows): windows of resident sequences, the
pattern on either strand, give pair for pair the oracle's score, status and op string for the materialised strings (Python slicing and
a reverse complement on the host) — through the C ABI binding and through align_windows, across configurations, scopes, residues of
the starts and lengths, letters, lengths, set lifetimes and refusals.  Every pair of every list is compared, exact equality."""
import numpy as np
import pytest

from common import assert_same, configs_pair, rle
from oracle import loader
from pywfa_amd import WavefrontAligner, _native, datagen
from pywfa_amd.align import _OP_CHARS, _flank_scan, _ops_to_tuples
from test_cross_topk_gpu import GRID

LETTERS = np.array(list("ACGT"))
COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp(s):
    return s.translate(COMP)[::-1]


def mutate(rng, f, div):
    """A copy of the base array `f` (values 0-3) with substitutions, deletions and insertions at `div` in all."""
    n = len(f)
    r = rng.random(n)
    sub = rng.integers(0, 4, n)
    out = np.where(r < div / 3, sub, f)
    counts = np.where((r >= div / 3) & (r < 2 * div / 3), 0, np.where((r >= 2 * div / 3) & (r < div), 2, 1))
    rep = np.repeat(np.arange(n), counts)
    res = out[rep]
    dup = np.r_[False, rep[1:] == rep[:-1]]
    res[dup] = sub[rep[dup]]
    return res


def corpus(seed=77, nreads=320):
    """Four references of 20-60 kb, the last with several N runs; reads of 100-200 bases cut from random positions of them (from the
    bases under the Ns too), mutated at 3 %, every second one stored reverse-complemented.  Returns the references, the N runs of the
    last one, the reads and per read (reference, position, length of the locus, stored reversed)."""
    rng = np.random.default_rng(seed)
    bases = [rng.integers(0, 4, n) for n in (20000, 35000, 60000, 30011)]
    refs = ["".join(LETTERS[b]) for b in bases]
    runs = [(0, 7), (1500, 1501), (4000, 4016), (9000, 9100), (15003, 15350), (22222, 22230), (30000, 30011)]
    last = list(refs[3])
    for a, b in runs:
        last[a:b] = "N" * (b - a)
    refs[3] = "".join(last)
    reads, origin = [], []
    for k in range(nreads):
        r = int(rng.integers(0, 4))
        n = int(rng.integers(100, 201))
        pos = int(rng.integers(0, len(bases[r]) - n + 1))
        s = "".join(LETTERS[mutate(rng, bases[r][pos:pos + n], 0.03)])
        rev = k % 2 == 1
        reads.append(revcomp(s) if rev else s)
        origin.append((r, pos, n, rev))
    return refs, runs, reads, origin


REFS, NRUNS, READS, ORIGIN = corpus()


def materialise(P, T, W):
    """The explicit pairs of a window list: Python slicing and the reverse complement, on the upper-cased strings."""
    T = P if T is None else T
    n = len(W["i"])
    pats, txts = [], []
    for q in range(n):
        p, t = P[W["i"][q]].upper(), T[W["j"][q]].upper()
        ps = int(W["p_start"][q]) if W.get("p_start") is not None else 0
        ts = int(W["t_start"][q]) if W.get("t_start") is not None else 0
        pl = int(W["p_len"][q]) if W.get("p_len") is not None else len(p) - ps
        tl = int(W["t_len"][q]) if W.get("t_len") is not None else len(t) - ts
        assert 0 <= ps and 0 <= pl and ps + pl <= len(p) and 0 <= ts and 0 <= tl and ts + tl <= len(t), q
        pw = p[ps:ps + pl]
        if W.get("reverse") is not None and W["reverse"][q]:
            pw = revcomp(pw)
        pats.append(pw)
        txts.append(t[ts:ts + tl])
    return pats, txts


def oracle_windows(kw, P, T, W):
    pats, txts = materialise(P, T, W)
    batch = datagen.from_strings(pats, txts, upper=True)
    o = loader.run(loader.oracle(), loader.make_config(**kw), batch)
    clean = sum(1 for p, t in zip(pats, txts) if not (set(p) | set(t)) - set("ACGT"))
    return o, batch, clean


def native_set(al, seqs):
    b = datagen.from_strings(b"", list(seqs), upper=True)
    return al.seqset(b["seqs"], b["t_off"], b["t_len"])


def cigars_of(cig, n):
    ops, cbeg, clen = cig
    return [ops[cbeg[q]:cbeg[q] + clen[q]].tobytes() for q in range(n)]


def native_windows(al, ps, ts, W):
    return al.batch_windows(ps, ts, W["i"], W["j"], W.get("p_start"), W.get("p_len"), W.get("t_start"), W.get("t_len"), W.get("reverse"))


def oracle_locations(o, batch):
    """What the reference's class derives from the oracle's op strings: (pattern_start, pattern_end, text_start, text_end)."""
    out = np.zeros((len(o["cigars"]), 4), np.int32)
    for q, c in enumerate(o["cigars"]):
        ct = _ops_to_tuples(np.frombuffer(c, np.uint8))
        pl, tl = int(batch["p_len"][q]), int(batch["t_len"][q])
        if ct and pl and tl:
            out[q] = _flank_scan(ct, 1, 1, tl, pl)[2:]
    return out


def check_abi(kw, P, T, W, o, batch, clean, ctx):
    """Through the C ABI binding: sets, wfa_hip_batch_create_windows, run, results, rle; the 2-bit routing."""
    _, nc = configs_pair(**kw)
    full = nc.scope == 1
    n = len(W["i"])
    al = _native.Aligner(nc)
    try:
        ps = native_set(al, P)
        ts = native_set(al, T) if T is not None else None
        rb = native_windows(al, ps, ts, W)
        rb.run()
        rb.sync()
        score, status, cig = rb.results(full)
        routed = rb.last_kernel()[1]
        got = rb.rle() if full else None
        rb.close()
        ps.close()
        if ts is not None:
            ts.close()
    finally:
        al.close()
    assert_same(o, score, status, cigars_of(cig, n) if full else None, batch, (ctx, "C ABI"))
    if nc.wildcard not in tuple(b"ACGTacgt"):
        # a pair takes the 2-bit kernels exactly when its two WINDOWS hold only ACGT, whatever else its sequences hold
        assert routed == clean, (ctx, "2-bit pairs", routed, clean)
    if full:
        off, code, rlen, locs = got
        assert np.array_equal(locs, oracle_locations(o, batch)), (ctx, "locations")
        for q in range(n):
            assert "".join(f"{rlen[k]}{_OP_CHARS[code[k]]}" for k in range(off[q], off[q + 1])) == rle(o["cigars"][q]), (ctx, q)


def check_python(kw, P, T, W, o, batch, ctx, aligner=None):
    """Through WavefrontAligner.align_windows (lists of str, or handles when `aligner` is given)."""
    al = aligner or WavefrontAligner(**kw)
    n = len(W["i"])
    out = al.align_windows(P, T, i=W["i"], j=W["j"], pattern_start=W.get("p_start"), pattern_len=W.get("p_len"),
                           text_start=W.get("t_start"), text_len=W.get("t_len"), reverse=W.get("reverse"))
    full = kw.get("scope", "full") == "full"
    assert out["score"].dtype == np.int32 and out["status"].dtype == np.int32 and len(out["score"]) == n, ctx
    cigars = None
    if full:
        assert len(out["cigar_ops"]) == n and len(out["cigarstrings"]) == n, ctx
        cigars = [np.asarray(out["cigar_ops"][q], np.uint8).tobytes() for q in range(n)]
    else:
        assert "cigar_ops" not in out and "cigarstrings" not in out, ctx
    assert_same(o, out["score"], out["status"], cigars, batch, (ctx, "align_windows"))
    if full:
        for q in range(n):
            assert out["cigarstrings"][q] == rle(o["cigars"][q]), (ctx, q)
    return out


def check_both(kw, P, T, W, ctx):
    o, batch, clean = oracle_windows(kw, P, T, W)
    check_abi(kw, P, T, W, o, batch, clean, ctx)
    check_python(kw, P, T, W, o, batch, ctx)
    return o, clean


def as_list(rows):
    """rows of (i, j, p_start, p_len, t_start, t_len, reverse) -> the arrays of a window list"""
    a = np.array(rows, dtype=np.int64).reshape(-1, 7)
    return dict(i=a[:, 0].copy(), j=a[:, 1].astype(np.int32), p_start=a[:, 2].astype(np.int32), p_len=a[:, 3].copy(),
                t_start=a[:, 4].copy(), t_len=a[:, 5].astype(np.int32), reverse=a[:, 6].astype(np.uint8))


def seed_rows(seed, n, pad_lo, pad_hi, clip=0.25, fixed_pad=None):
    """Seeds: read k against a window of its reference around its locus, padded on both sides (clipped to the reference);
    `clip` of the pairs take a pattern window (a clipped read), on the read's strand.  Every window is at least 8 bases long."""
    rng = np.random.default_rng(seed)
    rows = []
    while len(rows) < n:
        k = int(rng.integers(0, len(READS)))
        r, pos, ln, rev = ORIGIN[k]
        if fixed_pad is None:
            left, right = int(rng.integers(pad_lo, pad_hi + 1)), int(rng.integers(pad_lo, pad_hi + 1))
        else:
            left = right = fixed_pad
            if pos < left or pos + ln + right > len(REFS[r]):
                continue
        t0, t1 = max(0, pos - left), min(len(REFS[r]), pos + ln + right)
        ps, pl = 0, len(READS[k])
        if rng.random() < clip:
            ps = int(rng.integers(1, 40))
            pl = int(rng.integers(40, len(READS[k]) - ps + 1))
        rows.append((k, r, ps, pl, t0, t1 - t0, int(rev)))
    return rows


def grid_rows():
    rows = seed_rows(1, 1900, 0, 30)
    rng = np.random.default_rng(2)
    for r, ref in enumerate(REFS):   # windows touching position 0 and the sequence end, on both strands of some read
        for k in rng.integers(0, len(READS), 6):
            k = int(k)
            rows.append((k, r, 0, len(READS[k]), 0, int(rng.integers(100, 260)), int(ORIGIN[k][3])))
            tl = int(rng.integers(100, 260))
            rows.append((k, r, 0, len(READS[k]), len(ref) - tl, tl, 1 - int(ORIGIN[k][3])))
    rows += [rows[int(q)] for q in rng.integers(0, len(rows), 150)]          # duplicates
    for q in rng.integers(0, 1900, 100):                                      # overlapping windows: the same pair shifted a little
        k, r, ps, pl, t0, tl, rev = rows[int(q)]
        t0b = min(max(0, t0 + int(rng.integers(-9, 10))), len(REFS[r]) - tl)
        rows.append((k, r, ps, pl, t0b, tl, rev))
    order = rng.permutation(len(rows))
    return [rows[int(q)] for q in order]


GRID_LIST = as_list(grid_rows())
SCOPED = [(f"{name}-{scope}", dict(kw, scope=scope)) for name, kw in GRID for scope in ("score", "full")]


def test_grid_list_covers_what_it_should():
    W = GRID_LIST
    assert 2000 <= len(W["i"]) <= 5000
    assert set(W["t_start"] % 16) == set(range(16)) and set(W["t_len"] % 16) == set(range(16))
    assert (W["t_start"] == 0).any() and any(W["t_start"][q] + W["t_len"][q] == len(REFS[W["j"][q]]) for q in range(len(W["i"])))
    assert (W["p_start"] > 0).sum() > 200 and 0.3 < W["reverse"].mean() < 0.7
    assert ((W["p_start"] > 0) & (W["reverse"] == 1)).any() and ((W["p_start"] > 0) & (W["reverse"] == 0)).any()
    assert min(W["t_len"].min(), W["p_len"].min()) >= 8          # (the grid's free ends go up to 8)
    pats, txts = materialise(READS, REFS, W)
    on_n_ref = W["j"] == 3
    dirty = np.array(["N" in t for t in txts])
    assert (on_n_ref & ~dirty).sum() > 100 and dirty.sum() > 3, "windows of the N-holding reference that avoid the Ns, and some that do not"


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", SCOPED, ids=[g[0] for g in SCOPED])
def test_grid(gpu, name, kw):
    check_both(kw, READS, REFS, GRID_LIST, name)


@pytest.mark.gpu
@pytest.mark.parametrize("scope", ["score", "full"])
def test_padded_seeds(gpu, scope):
    """Text windows of read length plus padding: ends-free with free text ends equal to the padding, and end-to-end."""
    pad = 24
    W = as_list(seed_rows(3, 2500, 0, 0, clip=0.0, fixed_pad=pad))
    assert (W["t_len"] == np.array([ORIGIN[k][2] for k in W["i"]]) + 2 * pad).all()     # the read's locus and the padding
    for kw in (dict(span="ends-free", text_begin_free=pad, text_end_free=pad, scope=scope), dict(span="end-to-end", scope=scope)):
        o, _ = check_both(kw, READS, REFS, W, ("padded", kw))
        assert (np.asarray(o["status"]) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("scope", ["score", "full"])
def test_edges_and_one_set(gpu, scope):
    """Empty and one-base windows, duplicates, overlapping windows, i == j; texts=None: windows of one set against windows of the same set."""
    rng = np.random.default_rng(4)
    rows = []
    for _ in range(1200):   # a window of a reference against an overlapping or nearby window of the same or another reference
        i = int(rng.integers(0, len(REFS)))
        j = i if rng.random() < 0.7 else int(rng.integers(0, len(REFS)))
        pl, tl = int(rng.integers(0, 260)), int(rng.integers(0, 260))
        ps = int(rng.integers(0, len(REFS[i]) - pl + 1))
        ts = min(max(0, ps + int(rng.integers(-20, 21))), len(REFS[j]) - tl) if j == i else int(rng.integers(0, len(REFS[j]) - tl + 1))
        rows.append((i, j, ps, pl, ts, tl, int(rng.random() < 0.5)))
    for i in range(len(REFS)):
        n = len(REFS[i])
        for rev in (0, 1):
            rows += [(i, i, 0, 0, 0, 0, rev), (i, i, n, 0, n, 0, rev), (i, i, 5, 0, 5, 40, rev), (i, i, 5, 40, 5, 0, rev),
                     (i, i, 0, 1, 0, 1, rev), (i, i, n - 1, 1, n - 1, 1, rev), (i, i, 77, 1, 60, 35, rev), (i, i, 60, 35, 77, 1, rev),
                     (i, i, 100, 200, 100, 200, rev), (i, i, n - 200, 200, n - 200, 200, rev)]
    rows += [rows[int(q)] for q in rng.integers(0, len(rows), 100)]
    W = as_list(rows)
    assert (W["p_len"] == 0).any() and (W["t_len"] == 0).any() and (W["p_len"] == 1).any() and (W["t_len"] == 1).any()
    for kw in (dict(span="end-to-end", scope=scope), dict(scope=scope), dict(scope=scope, wildcard="N")):
        check_both(kw, REFS, None, W, ("one set", kw))
    # the reads' set against itself: read windows on both strands
    rows = []
    for _ in range(800):
        i, j = int(rng.integers(0, len(READS))), int(rng.integers(0, len(READS)))
        pl, tl = int(rng.integers(0, len(READS[i]) + 1)), int(rng.integers(0, len(READS[j]) + 1))
        rows.append((i, j, int(rng.integers(0, len(READS[i]) - pl + 1)), pl, int(rng.integers(0, len(READS[j]) - tl + 1)), tl, int(rng.random() < 0.5)))
    check_both(dict(span="end-to-end", scope=scope, max_steps=80), READS, None, as_list(rows), "reads against reads")


@pytest.mark.gpu
@pytest.mark.parametrize("scope", ["score", "full"])
def test_long_windows(gpu, scope):
    """Windows longer than 512 bases: 2 kb exact, 10 kb under the adaptive heuristic, a handful under gap-affine-2p."""
    rng = np.random.default_rng(5)
    longs = []
    origin = []
    for n in [2000] * 10 + [10000] * 4 + [700, 1300]:
        r = int(rng.integers(0, 3))
        pos = int(rng.integers(0, len(REFS[r]) - n + 1))
        b = np.array([("ACGT".index(c)) for c in REFS[r][pos:pos + n]])
        s = "".join(LETTERS[mutate(rng, b, 0.02)])
        rev = len(longs) % 2 == 1
        longs.append(revcomp(s) if rev else s)
        origin.append((r, pos, n, rev))

    def rows_for(ks, shift, first=0):
        rows = []
        for k in ks:
            r, pos, n, rev = origin[k]
            t0 = max(0, pos - shift)
            t1 = min(len(REFS[r]), pos + n + shift)
            rows.append((first + k, r, 0, len(longs[k]), t0, t1 - t0, int(rev)))
            ps = 1 + k
            rows.append((first + k, r, ps, len(longs[k]) - ps - 3, pos + ps, n - ps - 3, int(rev)))     # a pattern window of the long read
        return rows

    two_kb, ten_kb, mid = list(range(10)), list(range(10, 14)), [14, 15]
    check_both(dict(span="end-to-end", scope=scope), longs, REFS, as_list(rows_for(two_kb + mid, 7)), "2 kb exact")
    check_both(dict(span="end-to-end", scope=scope, heuristic="adaptive"), longs, REFS, as_list(rows_for(ten_kb + two_kb[:3], 11)), "10 kb adaptive")
    check_both(dict(span="end-to-end", scope=scope, distance="affine2p"), longs, REFS, as_list(rows_for(two_kb[:4] + mid, 5)), "affine2p")
    # long and short windows in one list
    W = as_list(rows_for(two_kb[:5], 3, first=len(READS)) + seed_rows(6, 300, 0, 20))
    check_both(dict(span="end-to-end", scope=scope), READS + longs, REFS, W, "long and short")


def letter_rows():
    """Windows of the N-holding reference that cross an N run, end just before one and start just after one, as texts (reads as
    patterns) and as patterns (on both strands: the N stays N under the complement)."""
    rng = np.random.default_rng(7)
    rows = []
    n3 = len(REFS[3])
    for a, b in NRUNS:
        for tl in (40, 150, 233):
            for t0 in (a - tl, a - tl + 1, a - tl // 2, a - 1, a, b - 1, b, b + 1, b - tl // 2):
                if t0 < 0 or t0 + tl > n3:
                    continue
                k = int(rng.integers(0, len(READS)))
                rows.append((k, 3, 0, len(READS[k]), t0, tl, int(ORIGIN[k][3])))
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("scope", ["score", "full"])
def test_letters(gpu, scope):
    rows = letter_rows() + seed_rows(8, 600, 0, 25)
    W = as_list(rows)
    pats, txts = materialise(READS, REFS, W)
    just_before = sum(1 for q, t in enumerate(txts) if "N" not in t and any(W["t_start"][q] + W["t_len"][q] == a for a, _ in NRUNS) and W["j"][q] == 3)
    just_after = sum(1 for q, t in enumerate(txts) if "N" not in t and any(W["t_start"][q] == b for _, b in NRUNS) and W["j"][q] == 3)
    assert just_before >= 5 and just_after >= 5 and sum("N" in t for t in txts) >= 30
    for kw in (dict(wildcard="N", scope=scope), dict(wildcard="N", scope=scope, span="end-to-end", max_steps=150),
               dict(scope=scope, span="end-to-end", max_steps=150),            # letters outside ACGT without a wildcard: byte pairs too
               dict(wildcard="A", scope=scope, span="end-to-end", max_steps=150)):   # a wildcard among ACGT: every pair on its bytes
        _, clean = check_both(kw, READS, REFS, W, ("letters", kw))
        assert 0 < clean < len(rows)
    # the N-holding reference as the pattern set too, both strands (texts=None)
    rng = np.random.default_rng(9)
    rows = []
    for a, b in NRUNS:
        for pl in (30, 120):
            for p0 in (a - pl, a - pl + 3, a - 2, b - 1, b, b - pl // 2):
                if p0 < 0 or p0 + pl > len(REFS[3]):
                    continue
                for rev in (0, 1):
                    rows.append((3, int(rng.integers(0, 4)), p0, pl, int(rng.integers(0, 19000)), int(rng.integers(20, 160)), rev))
                    rows.append((3, 3, p0, pl, max(0, p0 - 3), pl, rev))
    for kw in (dict(wildcard="N", scope=scope, span="end-to-end", max_steps=120), dict(scope=scope, span="end-to-end", max_steps=120),
               dict(wildcard="C", scope=scope, max_steps=120)):
        check_both(kw, REFS, None, as_list(rows), ("letters as patterns", kw))
    # lower-case input: upper-cased on the way in, as wavefront_align_batch does
    kw = dict(scope=scope, span="end-to-end")
    W = as_list(seed_rows(10, 300, 0, 20))
    o, batch, _ = oracle_windows(kw, READS, REFS, W)
    check_python(kw, [s.lower() for s in READS], [s.lower() for s in REFS], W, o, batch, "lower case")


@pytest.mark.gpu
@pytest.mark.parametrize("scope", ["score", "full"])
def test_lifetime_and_reuse(gpu, scope):
    kw = dict(span="end-to-end", scope=scope)
    full = scope == "full"
    W = as_list(letter_rows()[:120] + seed_rows(11, 700, 0, 20))
    n = len(W["i"])
    o, batch, clean = oracle_windows(kw, READS, REFS, W)
    _, nc = configs_pair(**kw)
    al = _native.Aligner(nc)
    try:
        ps, ts = native_set(al, READS), native_set(al, REFS)
        rb = native_windows(al, ps, ts, W)
        ps.close()
        ts.close()                                   # the batch outlives both sets
        other = native_set(al, REFS[::-1])            # (something else takes the released blocks)
        for _ in range(2):
            rb.run()
            rb.sync()
            s, t, cig = rb.results(full)
            assert_same(o, s, t, cigars_of(cig, n) if full else None, batch, "after the sets are gone")
            assert rb.last_kernel()[1] == clean
        ex = al.batch(batch)                         # the explicit batch of the same materialised pairs
        ex.run()
        ex.sync()
        assert rb.last_kernel()[1] == ex.last_kernel()[1] and rb.algorithmic_bytes() == ex.algorithmic_bytes()
        if full:
            for g, r, what in zip(rb.rle(), ex.rle(), ("run offsets", "run codes", "run lengths", "locations")):
                assert g.dtype == r.dtype and np.array_equal(g, r), what
        ex.close()
        rb.close()
        other.close()
        # one set serves a windowed batch, an indexed batch and a cross run in turn; every optional array NULL = the indexed batch
        rs = native_set(al, READS[:60])
        i = np.arange(60, dtype=np.int32)
        j = i[::-1].copy()
        outs = []
        for make in (lambda: al.batch_windows(rs, None, i, j), lambda: al.batch_indexed(rs, None, i, j), None,
                     lambda: al.batch_windows(rs, rs, i, j)):
            if make is None:
                x = al.cross(rs)
                dense = x.dense()
                x.close()
                continue
            b = make()
            b.run()
            b.sync()
            outs.append(b.results(full))
            b.close()
        rs.close()
        oi, bi, _ = oracle_windows(kw, READS[:60], None, dict(i=i, j=j))
        for s, t, cig in outs:
            assert_same(oi, s, t, cigars_of(cig, 60) if full else None, bi, "every optional array NULL")
        assert np.array_equal(dense[0][i, j], outs[0][0])
    finally:
        al.close()
    # open handles through align_windows, the set reused by nearest() and align_pairs() in between
    wa = WavefrontAligner(**kw)
    with wa.sequence_set(READS) as R, wa.sequence_set(REFS) as G:
        check_python(kw, R, G, W, o, batch, "handles", aligner=wa)
        near = wa.nearest(R, k=1)
        assert near["j"].shape == (len(READS), 1)
        pairs = wa.align_pairs(R, i=[0, 1], j=[1, 0])
        assert len(pairs["score"]) == 2
        check_python(kw, R, G, W, o, batch, "handles again", aligner=wa)
    with pytest.raises(ValueError, match="closed"):
        wa.align_windows(R, G, i=[0], j=[0])


def multipart_list():
    """A list long enough for two host parts of the list planner (it splits a list over host threads once every part gets 65536
    pairs, and the parts meet on a multiple of 256, the generator's chunk): 2 * 65536 + 300 windows of 20-40 bases, the 300 leaving
    a partial last chunk.  Texts are three references of a few thousand bases, the last with five single Ns; patterns are copies
    of them with 3 % substitutions (same coordinates) and the reverse complements of those copies, so that a reversed pair is as
    related as a forward one.  About 1 % of the pairs are reversed, about 1 % are byte pairs (their text window covers an N), and a
    pair that is both sits at the part boundary, on either side of it and at the end of the list.
    Returns the pattern set, the text set, the list and the boundary position."""
    n = 2 * 65536 + 300
    edge = (n // 2) & ~255
    rng = np.random.default_rng(21)
    bases = [rng.integers(0, 4, m) for m in (3000, 4100, 5003)]
    lens = np.array([len(b) for b in bases])
    n_at = (700, 1733, 2500, 3301, 4250)
    texts = [LETTERS[b] for b in bases]
    texts[2][list(n_at)] = "N"
    texts = ["".join(t) for t in texts]
    copies = ["".join(LETTERS[np.where(rng.random(len(b)) < 0.03, rng.integers(0, 4, len(b)), b)]) for b in bases]
    pats = copies + [revcomp(s) for s in copies]
    r = rng.integers(0, 3, n)
    pl, tl = rng.integers(20, 41, n), rng.integers(20, 41, n)
    ts = 3 + (rng.random(n) * (lens[r] - 46)).astype(np.int64)
    ps = ts + rng.integers(-3, 4, n)
    rev = rng.random(n) < 0.01
    for k, q in enumerate((edge - 1, edge, edge + 1, n - 1)):
        r[q], ts[q], tl[q], ps[q], pl[q], rev[q] = 2, n_at[k] - 10 - k, 30 + k, n_at[k] - 9, 27 + k, True
    W = dict(i=np.where(rev, 3 + r, r).astype(np.int64), j=r.astype(np.int32),
             p_start=np.where(rev, lens[r] - (ps + pl), ps).astype(np.int32), p_len=pl.astype(np.int64),
             t_start=ts.astype(np.int64), t_len=tl.astype(np.int32), reverse=rev.astype(np.uint8))
    return pats, texts, W, edge


@pytest.mark.gpu
@pytest.mark.parametrize("scope", ["score", "full"])
def test_multipart_list(gpu, scope):
    """Two host parts: what each part writes from its own base (the op-region prefix, the two work lists, the chunk bases of the
    word and byte slots) against the oracle, pair for pair."""
    pats, texts, W, edge = multipart_list()
    n = len(W["i"])
    assert n == 2 * 65536 + 300 and n // 65536 >= 2 and edge % 256 == 0 and n % 256 != 0
    kw = dict(span="end-to-end", scope=scope)
    o, batch, clean = oracle_windows(kw, pats, texts, W)
    dirty = np.array(["N" in texts[W["j"][q]][W["t_start"][q]:W["t_start"][q] + W["t_len"][q]] for q in range(n)])
    assert n - clean == dirty.sum() and 0.005 * n < dirty.sum() < 0.02 * n and 0.005 * n < W["reverse"].sum() < 0.02 * n
    assert ((W["j"] == 2) & ~dirty).sum() > 10000, "windows of the N-holding reference that avoid the Ns"
    spots = (edge - 1, edge, edge + 1, n - 1)
    assert all(dirty[q] and W["reverse"][q] for q in spots)
    assert dirty[:edge].any() and not dirty[:edge].all() and (W["reverse"][:edge] == 1).any() and (W["reverse"][edge:] == 1).any()
    # through the C ABI binding: first the two pairs that go wrong when a part's base is off, by name, then every pair
    full = scope == "full"
    _, nc = configs_pair(**kw)
    al = _native.Aligner(nc)
    try:
        ps, ts = native_set(al, pats), native_set(al, texts)
        rb = native_windows(al, ps, ts, W)
        rb.run()
        rb.sync()
        score, status, cig = rb.results(full)
        routed = rb.last_kernel()[1]
        rb.close()
        ps.close()
        ts.close()
    finally:
        al.close()
    for q, what in ((edge - 1, "last pair of the first part"), (edge, "first pair of the second part"), (n - 1, "last pair of the list")):
        assert (score[q], status[q]) == (o["score"][q], o["status"][q]), (what, q)
        if full:
            ops, cbeg, clen = cig
            assert rle(ops[cbeg[q]:cbeg[q] + clen[q]].tobytes()) == rle(o["cigars"][q]), (what, q)
    assert_same(o, score, status, cigars_of(cig, n) if full else None, batch, ("two parts", scope, "C ABI"))
    assert routed == clean, ("two parts", "2-bit pairs", routed, clean)
    check_python(kw, pats, texts, W, o, batch, ("two parts", scope))


@pytest.mark.gpu
def test_refusals(gpu):
    kw = dict(span="end-to-end", scope="full")
    _, nc = configs_pair(**kw)
    W = as_list(seed_rows(12, 40, 0, 10))
    o, batch, _ = oracle_windows(kw, READS, REFS, W)

    def usable(al, ps, ts):
        rb = native_windows(al, ps, ts, W)
        rb.run()
        rb.sync()
        s, t, cig = rb.results(True)
        rb.close()
        assert_same(o, s, t, cigars_of(cig, 40), batch, "usable afterwards")

    al, al2 = _native.Aligner(nc), _native.Aligner(nc)
    try:
        ps, ts, foreign = native_set(al, READS), native_set(al, REFS), native_set(al2, REFS)
        # the first out-of-range window is named, with its values
        bad = dict(W, t_start=W["t_start"].copy(), p_len=W["p_len"].copy())
        bad["t_start"][17] = len(REFS[bad["j"][17]]) - bad["t_len"][17] + 1
        bad["p_len"][30] = 100000
        with pytest.raises(_native.NativeError, match=rf"window out of range at position 17 .*\[{bad['t_start'][17]}, {bad['t_start'][17]} \+ {bad['t_len'][17]}\)"):
            native_windows(al, ps, ts, bad)
        assert "position 17 " in al.error()
        usable(al, ps, ts)
        bad = dict(W, p_start=W["p_start"].copy())
        bad["p_start"][5] = -2
        with pytest.raises(_native.NativeError, match="negative start or length at position 5 "):
            native_windows(al, ps, ts, bad)
        bad = dict(W, i=W["i"].copy())
        bad["i"][9] = len(READS)
        with pytest.raises(_native.NativeError, match="index out of range at position 9 "):
            native_windows(al, ps, ts, bad)
        usable(al, ps, ts)
        with pytest.raises(_native.NativeError, match="another aligner"):
            native_windows(al, ps, foreign, W)
        # a wildcard changed after packing
        nw = nc.copy()
        nw.wildcard = ord("N")
        al.set_config(nw)
        with pytest.raises(_native.NativeError, match="another wildcard"):
            native_windows(al, ps, ts, W)
        al.set_config(nc)
        usable(al, ps, ts)
        # free ends larger than a listed WINDOW (the sequences are long enough)
        nf = nc.copy()
        nf.span, nf.text_begin_free, nf.text_end_free = 1, 30, 30
        al.set_config(nf)
        short = dict(W, t_len=W["t_len"].copy())
        short["t_len"][3] = 29
        with pytest.raises(_native.NativeError, match="Ends-free parameters must be not larger than the sequences"):
            native_windows(al, ps, ts, short)
        rb = native_windows(al, ps, ts, W)     # every listed window is longer than the free ends: fine
        rb.close()
        al.set_config(nc)
        usable(al, ps, ts)
        # an empty list is a valid empty batch
        e = np.zeros(0, np.int32)
        rb = al.batch_windows(ps, ts, e, e, e, e, e, e, np.zeros(0, np.uint8))
        rb.run()
        rb.sync()
        s, t, _ = rb.results(True)
        assert len(s) == 0 and len(t) == 0 and rb.last_kernel()[1] == 0
        rb.close()
        usable(al, ps, ts)
        for x in (ps, ts, foreign):
            x.close()
    finally:
        al.close()
        al2.close()
    for scope in ("score", "full"):
        out = WavefrontAligner(scope=scope).align_windows(READS[:3], REFS[:1], i=[], j=[])
        assert out["score"].shape == (0,) and out["status"].shape == (0,)
    wa = WavefrontAligner(text_begin_free=30, text_end_free=30)
    with pytest.raises(_native.NativeError, match="Ends-free parameters"):
        wa.align_windows(READS, REFS, i=[0], j=[0], text_start=[5], text_len=[29])


@pytest.mark.gpu
def test_chunked_lists(gpu, monkeypatch):
    """Lists longer than the pair budget run in consecutive chunks and come back joined."""
    W = as_list(seed_rows(13, 2500, 0, 20))
    monkeypatch.setenv("WFA_HIP_PAIRS_BAND", "700")
    for kw in (dict(span="end-to-end"), dict(span="end-to-end", scope="score")):
        o, batch, _ = oracle_windows(kw, READS, REFS, W)
        check_python(kw, READS, REFS, W, o, batch, ("chunks of 700", kw))
