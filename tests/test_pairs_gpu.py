"""Indexed batches on the GPU (wfa_hip_batch_create_indexed, WavefrontAligner.align_pairs / sequence_set): a list of (i, j) index
pairs over resident sequence sets gives, pair for pair, the oracle's score, status and op string for the explicit pairs — through the
C ABI binding and through align_pairs, across configurations, scopes, lengths, letters, sizes, set lifetimes and refusals.  Every pair
of every list is compared, exact equality."""
import numpy as np
import pytest

from common import assert_same, configs_pair, rle
from oracle import loader
from pywfa_amd import WavefrontAligner, _native, datagen
from test_cross_topk_gpu import GRID

INT32_MIN = np.iinfo(np.int32).min
FREE = ("pattern_begin_free", "pattern_end_free", "text_begin_free", "text_end_free")


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


def family_reads(seed, founders, copies, lo, hi, div=0.03, empty=0, alphabet="ACGT", n_rate=0.0):
    """Reads in families (founder f's copies are reads f * copies .. + copies), then `empty` empty reads; the family of every read."""
    rng = np.random.default_rng(seed)
    letters = np.array(list(alphabet))
    reads, fam = [], []
    for f in range(founders):
        base = rng.integers(0, 4, int(rng.integers(lo, hi + 1)))
        for _ in range(copies):
            s = letters[mutate(rng, base, div) % len(letters)] if len(base) else letters[:0]
            if n_rate and len(s) and rng.random() < 0.5:
                s = np.where(rng.random(len(s)) < n_rate, "N", s)
            reads.append("".join(s))
            fam.append(f)
    reads += [""] * empty
    fam += [-1] * empty
    return reads, np.array(fam)


def pair_list(seed, fam_p, fam_t, n, related=0.85, same=False):
    """A seeded list: `related` of the pairs inside a family, the rest anywhere; then duplicates of earlier pairs, pairs with an
    empty read and (one set) i == j."""
    rng = np.random.default_rng(seed)
    m, k = len(fam_p), len(fam_t)
    i = rng.integers(0, m, n)
    j = rng.integers(0, k, n)
    for q in np.flatnonzero(rng.random(n) < related):
        c = np.flatnonzero(fam_t == fam_p[i[q]])
        if len(c) and fam_p[i[q]] >= 0:
            j[q] = c[rng.integers(0, len(c))]
    dup = rng.integers(0, n, n // 10)
    i = np.concatenate([i, i[dup]])
    j = np.concatenate([j, j[dup]])
    ep, et = np.flatnonzero(fam_p < 0), np.flatnonzero(fam_t < 0)
    if len(ep) and len(et):
        i = np.concatenate([i, [ep[0], ep[-1], 0]])
        j = np.concatenate([j, [et[0], 1, et[-1]]])
    if same:
        d = rng.integers(0, m, 25)
        i = np.concatenate([i, d])
        j = np.concatenate([j, d])
    order = rng.permutation(len(i))
    return i[order].astype(np.int64), j[order].astype(np.int32)


def oracle_pairs(kw, P, T, i, j):
    T = P if T is None else T
    batch = datagen.from_strings([P[a] for a in i], [T[b] for b in j], upper=True)
    return loader.run(loader.oracle(), loader.make_config(**kw), batch), batch


def native_set(al, seqs):
    b = datagen.from_strings(b"", list(seqs), upper=True)
    return al.seqset(b["seqs"], b["t_off"], b["t_len"])


def cigars_of(cig, n):
    ops, cbeg, clen = cig
    return [ops[cbeg[q]:cbeg[q] + clen[q]].tobytes() for q in range(n)]


def check_abi(kw, P, T, i, j, o, batch, ctx):
    """Through the C ABI binding: sets, wfa_hip_batch_create_indexed, run, results."""
    _, nc = configs_pair(**kw)
    full = nc.scope == 1
    al = _native.Aligner(nc)
    try:
        ps = native_set(al, P)
        ts = native_set(al, T) if T is not None else None
        rb = al.batch_indexed(ps, ts, i, j)
        rb.run()
        rb.sync()
        score, status, cig = rb.results(full)
        if nc.wildcard not in tuple(b"ACGT") and not any((set(P[a]) | set((P if T is None else T)[b])) - set("ACGT") for a, b in zip(i, j)):
            assert rb.last_kernel()[1] == len(i), ctx     # (a list with byte pairs reports its 2-bit pairs, as an explicit batch does)
        rb.close()
        ps.close()
        if ts is not None:
            ts.close()
    finally:
        al.close()
    assert_same(o, score, status, cigars_of(cig, len(i)) if full else None, batch, (ctx, "C ABI"))


def check_python(kw, P, T, i, j, o, batch, ctx, aligner=None):
    """Through WavefrontAligner.align_pairs (lists of str, or handles when `aligner` is given)."""
    al = aligner or WavefrontAligner(**kw)
    out = al.align_pairs(P, T, i=i, j=j)
    full = kw.get("scope", "full") == "full"
    assert out["score"].dtype == np.int32 and out["status"].dtype == np.int32 and len(out["score"]) == len(i), ctx
    cigars = None
    if full:
        assert len(out["cigar_ops"]) == len(i) and len(out["cigarstrings"]) == len(i), ctx
        cigars = [np.asarray(out["cigar_ops"][q], np.uint8).tobytes() for q in range(len(i))]
    else:
        assert "cigar_ops" not in out and "cigarstrings" not in out, ctx
    assert_same(o, out["score"], out["status"], cigars, batch, (ctx, "align_pairs"))
    if full:
        for q in range(len(i)):
            assert out["cigarstrings"][q] == rle(o["cigars"][q]), (ctx, q)
    return out


def check_both(kw, P, T, i, j, ctx):
    o, batch = oracle_pairs(kw, P, T, i, j)
    check_abi(kw, P, T, i, j, o, batch, ctx)
    check_python(kw, P, T, i, j, o, batch, ctx)
    return o


READS, FAM = family_reads(11, 24, 5, 0, 300, empty=2)               # 122 reads of 0-300 bases, two empty
NE = [k for k, s in enumerate(READS) if len(s) >= 8]                # (free ends of up to 8 need reads at least that long)
READS_NE, FAM_NE = [READS[k] for k in NE], FAM[NE]

SCOPED = [(f"{name}-{scope}", dict(kw, scope=scope)) for name, kw in GRID for scope in ("score", "full")]
SCOPED += [(f"memory_{mm}-full", dict(memory_mode=mm, scope="full", span="end-to-end")) for mm in ("medium", "low")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", SCOPED, ids=[g[0] for g in SCOPED])
def test_grid(gpu, name, kw):
    reads, fam = (READS_NE, FAM_NE) if any(kw.get(k, 0) for k in FREE) else (READS, FAM)
    i, j = pair_list(5, fam, fam, 1500, same=True)
    check_both(kw, reads, None, i, j, (name, "one set"))
    cut = 50
    i, j = pair_list(6, fam[:cut], fam[cut:], 1200)
    check_both(kw, reads[:cut], reads[cut:], i, j, (name, "two sets"))


@pytest.mark.gpu
@pytest.mark.parametrize("scope", ["score", "full"])
def test_lengths(gpu, scope):
    """Slot pairs and pairs that point into the sets' words in one list, a 10 kb pair, and a longest sequence nobody lists."""
    short, fs = family_reads(21, 6, 4, 100, 500, div=0.02)
    mid, fm = family_reads(22, 3, 3, 520, 1200, div=0.02)
    big, _ = family_reads(23, 1, 2, 10000, 10000, div=0.01)
    unlisted, _ = family_reads(24, 1, 1, 20000, 20000)
    reads = short + mid + big + unlisted
    fam = np.concatenate([fs, fm + 100, [200, 200], [300]])
    listed = len(reads) - 1
    i, j = pair_list(7, fam[:listed], fam[:listed], 400, related=1.0, same=True)
    a, b, c = len(short) + len(mid), len(short) + len(mid) + 1, len(short)
    i = np.concatenate([i, [a, 0, c, c + 1]])   # the 10 kb pair, short x longer, longer x short, two unrelated longer reads
    j = np.concatenate([j, [b, c, 1, c + 4]]).astype(np.int32)
    assert max(i.max(), j.max()) < listed and (np.array([len(reads[k]) for k in i]) > 512).any()
    for kw in (dict(span="end-to-end", scope=scope), dict(scope=scope, max_steps=300, span="end-to-end")):
        check_both(kw, reads, None, i, j, ("lengths", kw))
    # two sets: the long reads as texts only
    keep = np.flatnonzero(i < len(short))
    check_both(dict(span="end-to-end", scope=scope), short, reads, i[keep], j[keep], ("lengths", "two sets"))


@pytest.mark.gpu
@pytest.mark.parametrize("scope", ["score", "full"])
def test_letters(gpu, scope):
    wild, fw = family_reads(31, 8, 4, 20, 200, n_rate=0.03, empty=1)
    clean, fc = family_reads(32, 4, 3, 20, 200)
    reads, fam = wild + clean, np.concatenate([fw, fc + 50])
    assert any("N" in s for s in reads) and any(s and "N" not in s for s in reads)
    i, j = pair_list(8, fam, fam, 900, same=True)
    for kw in (dict(wildcard="N", scope=scope), dict(wildcard="N", scope=scope, span="end-to-end"),
               dict(scope=scope, span="end-to-end"),                      # letters outside ACGT without a wildcard: byte pairs too
               dict(wildcard="A", scope=scope, span="end-to-end")):       # a wildcard among ACGT: every pair on its bytes
        check_both(kw, reads, None, i, j, ("letters", kw))
    cut = len(wild)
    i, j = pair_list(9, fam[:cut], fam[cut:], 500, related=0.0)
    check_both(dict(wildcard="N", scope=scope), reads[:cut], reads[cut:], i, j, ("letters", "two sets"))
    # lower-case input: upper-cased on the way in, as wavefront_align_batch does
    kw = dict(scope=scope, span="end-to-end")
    i, j = pair_list(10, fc, fc, 300, same=True)
    o, batch = oracle_pairs(kw, clean, None, i, j)
    check_python(kw, [s.lower() for s in clean], None, i, j, o, batch, "lower case")


def _big_workload():
    """16 384 reads of ~150 bp in 1 024 families of 16 at 2 %; every read against every read of its family: 262 144 pairs."""
    rng = np.random.default_rng(2025)
    letters = np.array(list("ACGT"))
    reads = []
    for _ in range(1024):
        base = rng.integers(0, 4, 150)
        reads += ["".join(letters[mutate(rng, base, 0.02)]) for _ in range(16)]
    r = np.arange(16384)
    i = np.repeat(r, 16)
    j = (np.repeat(r // 16 * 16, 16) + np.tile(np.arange(16), 16384)).astype(np.int32)
    order = rng.permutation(len(i))
    return reads, i[order], j[order]


@pytest.mark.gpu
def test_size(gpu):
    reads, i, j = _big_workload()
    assert len(i) >= 262144 and len(reads) == 16384
    kw = dict(span="end-to-end", scope="score")
    o, batch = oracle_pairs(kw, reads, None, i, j)
    check_abi(kw, reads, None, i, j, o, batch, "size score")
    al = WavefrontAligner(**kw)
    with al.sequence_set(reads) as S:
        assert len(S) == 16384
        check_python(kw, S, None, i, j, o, batch, "size score", aligner=al)
    # a 65 536-pair slice with scope full: op strings against the oracle, run-length encoding against the explicit resident batch
    n = 65536
    kw = dict(span="end-to-end", scope="full")
    i, j = i[:n], j[:n]
    o, batch = oracle_pairs(kw, reads, None, i, j)
    check_python(kw, reads, None, i, j, o, batch, "size full")
    _, nc = configs_pair(**kw)
    al = _native.Aligner(nc)
    try:
        ps = native_set(al, reads)
        rb = al.batch_indexed(ps, None, i, j)
        rb.run()
        rb.sync()
        score, status, cig = rb.results(True)
        assert_same(o, score, status, cigars_of(cig, n), batch, "size full C ABI")
        got = rb.rle()
        ex = al.batch(batch)
        ex.run()
        ex.sync()
        ref = ex.rle()
        assert rb.algorithmic_bytes() == ex.algorithmic_bytes()
        for g, r, what in zip(got, ref, ("run offsets", "run codes", "run lengths", "locations")):
            assert g.dtype == r.dtype and np.array_equal(g, r), what
        ex.close()
        rb.close()
        ps.close()
    finally:
        al.close()


def multipart_list():
    """A list long enough for two host parts of the list planner (it splits a list over host threads once every part gets 65536
    pairs, and the parts meet on a multiple of 256, the generator's chunk): 2 * 65536 + 300 pairs, the 300 leaving a partial last
    chunk, over 300 reads of 32-64 bases in families of five.  Two reads of 600-700 bases are too long for a word slot: listed in
    both parts, they put the sets' words in front of the slots.  Two reads hold an N: about 1 % of the pairs are byte pairs, and
    one sits at the part boundary, on either side of it and at the end of the list.  Returns the reads, the list and the boundary."""
    n = 2 * 65536 + 300
    edge = (n // 2) & ~255
    short, _ = family_reads(61, 60, 5, 32, 64)
    longs, _ = family_reads(62, 1, 2, 600, 700, div=0.02)
    wild = [short[0][:20] + "N" + short[0][20:], short[1][:9] + "N" + short[1][10:]]
    reads = short + longs + wild
    m, lg, wd = len(short), len(short), len(short) + 2
    rng = np.random.default_rng(63)
    i = rng.integers(0, m, n)
    j = np.where(rng.random(n) < 0.85, i // 5 * 5 + rng.integers(0, 5, n), rng.integers(0, m, n))
    for q in np.flatnonzero(rng.random(n) < 0.01):          # a byte pair: an N-holding read on either side, or on both
        kind = q % 3
        i[q], j[q] = (wd + q % 2, j[q]) if kind == 0 else (i[q], wd + q % 2) if kind == 1 else (wd, wd + 1)
    for base in (0, edge):                                   # the long reads, in each part
        for k, (a, b) in enumerate(((lg, lg + 1), (lg + 1, lg), (lg, 3), (4, lg + 1), (lg + 1, lg + 1))):
            i[base + 40 + 9001 * k], j[base + 40 + 9001 * k] = a, b
    for q, (a, b) in zip((edge - 1, edge, edge + 1, n - 1), ((wd, wd + 1), (wd + 1, wd), (0, wd), (wd + 1, 6))):
        i[q], j[q] = a, b
    return reads, i.astype(np.int64), j.astype(np.int32), edge


@pytest.mark.gpu
@pytest.mark.parametrize("scope", ["score", "full"])
def test_multipart_list(gpu, scope):
    """Two host parts: what each part writes from its own base (the op-region prefix, the two work lists, the chunk bases behind
    the sets' words) against the oracle, pair for pair."""
    reads, i, j, edge = multipart_list()
    n = len(i)
    assert n == 2 * 65536 + 300 and n // 65536 >= 2 and edge % 256 == 0 and n % 256 != 0
    length = np.array([len(s) for s in reads])
    dirty = np.array(["N" in s for s in reads])
    too_long = (length[i] > 512) | (length[j] > 512)         # (512: the longest sequence that still gets a word slot)
    byte_pair = dirty[i] | dirty[j]
    assert (length > 512).sum() == 2 and 600 <= length[length > 512].min() and length.max() <= 700
    assert 3 <= too_long[:edge].sum() <= 10 and 3 <= too_long[edge:].sum() <= 10
    assert 0.005 * n < byte_pair.sum() < 0.02 * n and byte_pair[:edge].any() and byte_pair[edge:].any()
    assert all(byte_pair[q] for q in (edge - 1, edge, edge + 1, n - 1))
    kw = dict(span="end-to-end", scope=scope)
    o, batch = oracle_pairs(kw, reads, None, i, j)
    # through the C ABI binding: first the two pairs that go wrong when a part's base is off, by name, then every pair
    full = scope == "full"
    _, nc = configs_pair(**kw)
    al = _native.Aligner(nc)
    try:
        ps = native_set(al, reads)
        rb = al.batch_indexed(ps, None, i, j)
        rb.run()
        rb.sync()
        score, status, cig = rb.results(full)
        routed = rb.last_kernel()[1]
        rb.close()
        ps.close()
    finally:
        al.close()
    for q, what in ((edge - 1, "last pair of the first part"), (edge, "first pair of the second part"), (n - 1, "last pair of the list")):
        assert (score[q], status[q]) == (o["score"][q], o["status"][q]), (what, q)
        if full:
            ops, cbeg, clen = cig
            assert rle(ops[cbeg[q]:cbeg[q] + clen[q]].tobytes()) == rle(o["cigars"][q]), (what, q)
    assert_same(o, score, status, cigars_of(cig, n) if full else None, batch, ("two parts", scope, "C ABI"))
    assert routed == n - byte_pair.sum(), ("two parts", "2-bit pairs", routed)
    check_both(kw, reads, None, i, j, ("two parts", scope))


@pytest.mark.gpu
@pytest.mark.parametrize("scope", ["score", "full"])
def test_lifetime_and_reuse(gpu, scope):
    kw = dict(span="end-to-end", scope=scope)
    long_reads, fl = family_reads(41, 2, 3, 600, 900, div=0.02)
    wild, fw = family_reads(42, 3, 3, 50, 150, n_rate=0.03)
    reads, fam = READS + long_reads + wild, np.concatenate([FAM, fl + 100, fw + 200])   # slots, set words and set bytes all in use
    cut = 60
    i, j = pair_list(12, fam[:cut], fam[cut:], 800)
    o, batch = oracle_pairs(kw, reads[:cut], reads[cut:], i, j)
    _, nc = configs_pair(**kw)
    full = scope == "full"
    al = _native.Aligner(nc)
    try:
        ps, ts = native_set(al, reads[:cut]), native_set(al, reads[cut:])
        rb = al.batch_indexed(ps, ts, i, j)
        ps.close()
        ts.close()                                   # the batch outlives both sets
        other = native_set(al, reads[::-1])           # (something else takes the released blocks)
        rb.run()
        rb.sync()
        first = rb.results(full)
        assert_same(o, first[0], first[1], cigars_of(first[2], len(i)) if full else None, batch, "after the sets are gone")
        ex = al.batch(batch)                         # (this list holds byte pairs: the count is the explicit batch's, its 2-bit pairs)
        ex.run()
        ex.sync()
        assert rb.last_kernel()[1] == ex.last_kernel()[1]
        ex.close()
        rb.run()                                     # a second run of the same batch
        rb.sync()
        again = rb.results(full)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        if full:
            assert cigars_of(first[2], len(i)) == cigars_of(again[2], len(i))
        rb.close()
        clean = np.flatnonzero((i < len(READS)) & (j + cut < len(READS)))   # pairs of ACGT reads only: last_kernel() reports npairs
        ps, ts = native_set(al, reads[:cut]), native_set(al, reads[cut:])
        rb = al.batch_indexed(ps, ts, i[clean], j[clean])
        ps.close()
        ts.close()
        for _ in range(2):
            rb.run()
            rb.sync()
            assert rb.last_kernel()[1] == len(clean) > 0
        assert np.array_equal(rb.results(full)[0], first[0][clean])
        rb.close()
        other.close()
    finally:
        al.close()
    # one set feeding two indexed batches with a nearest run in between
    wa = WavefrontAligner(**kw)
    S = wa.sequence_set(reads)
    try:
        i1, j1 = pair_list(13, fam, fam, 500, same=True)
        i2, j2 = pair_list(14, fam, fam, 700, same=True)
        o1, b1 = oracle_pairs(kw, reads, None, i1, j1)
        o2, b2 = oracle_pairs(kw, reads, None, i2, j2)
        check_python(kw, S, None, i1, j1, o1, b1, "first batch of the set", aligner=wa)
        near = wa.nearest(S, k=2)
        assert near["j"].shape == (len(reads), 2)
        check_python(kw, S, None, i2, j2, o2, b2, "second batch of the set", aligner=wa)
        check_python(kw, S, S, i1, j1, o1, b1, "the set as both arguments", aligner=wa)
        assert len(S) == len(reads)
    finally:
        S.close()
    with pytest.raises(ValueError, match="closed"):
        wa.align_pairs(S, i=[0], j=[0])


@pytest.mark.gpu
def test_refusals(gpu):
    L = _native.lib()
    kw = dict(span="end-to-end", scope="full")
    _, nc = configs_pair(**kw)
    reads = [s for s in READS if s][:40]
    good_i, good_j = np.arange(40, dtype=np.int32), np.arange(40, dtype=np.int32)[::-1].copy()
    o, batch = oracle_pairs(kw, reads, None, good_i, good_j)

    def usable(al, ps):
        rb = al.batch_indexed(ps, None, good_i, good_j)
        rb.run()
        rb.sync()
        s, t, cig = rb.results(True)
        rb.close()
        assert_same(o, s, t, cigars_of(cig, 40), batch, "usable afterwards")

    al, al2 = _native.Aligner(nc), _native.Aligner(nc)
    try:
        ps, foreign = native_set(al, reads), native_set(al2, reads)
        # an index outside its set: EINVAL, the message names the first bad position
        for bad_q, bad in ((17, 40), (3, -1)):
            i = good_i.copy()
            i[bad_q] = bad
            i[30] = 99
            assert not L.wfa_hip_batch_create_indexed(al._h, ps._h, None, 40, i.ctypes.data, good_j.ctypes.data)
            assert f"position {bad_q} " in al.error()
            with pytest.raises(ValueError, match=f"position {bad_q} "):
                al.batch_indexed(ps, None, i, good_j)
            usable(al, ps)
        j = good_j.copy()
        j[39] = 40
        with pytest.raises(ValueError, match="position 39 "):
            al.batch_indexed(ps, None, good_i, j)
        with pytest.raises(ValueError, match="differ in length"):
            al.batch_indexed(ps, None, good_i, good_j[:5])
        # a set of another aligner, as patterns and as texts
        with pytest.raises(ValueError, match="another aligner"):
            al.batch_indexed(foreign, None, good_i, good_j)
        with pytest.raises(ValueError, match="another aligner"):
            al.batch_indexed(ps, foreign, good_i, good_j)
        usable(al, ps)
        # a set packed under another wildcard
        nw = nc.copy()
        nw.wildcard = ord("N")
        al.set_config(nw)
        with pytest.raises(ValueError, match="another wildcard"):
            al.batch_indexed(ps, None, good_i, good_j)
        al.set_config(nc)
        usable(al, ps)
        # an empty list is a valid empty batch
        e = np.zeros(0, np.int32)
        rb = al.batch_indexed(ps, None, e, e)
        rb.run()
        rb.sync()
        s, t, cig = rb.results(True)
        assert len(s) == 0 and len(t) == 0 and rb.last_kernel()[1] == 0
        rb.close()
        usable(al, ps)
        ps.close()
        foreign.close()
    finally:
        al.close()
        al2.close()
    # free ends longer than a LISTED sequence; fine when only an unlisted sequence is too short
    kw = dict(pattern_begin_free=10, text_end_free=6, scope="full")
    seqs = ["ACGTACGTACGTACGT", "ACGTACGAACGTACGTAA", "ACGT", "ACGTTCGTACGTACGA"]
    wa = WavefrontAligner(**kw)
    for i, j in (([0, 2], [1, 1]), ([0, 1], [1, 2])):   # the short read as a pattern, then as a text
        with pytest.raises(ValueError, match="Ends-free parameters must be not larger than the sequences"):
            wa.align_pairs(seqs, i=i, j=j)
    i, j = [0, 1, 3, 3], [1, 3, 0, 3]
    o, batch = oracle_pairs(kw, seqs, None, i, j)
    check_python(kw, seqs, None, i, j, o, batch, "unlisted short read", aligner=wa)
    check_abi(kw, seqs, None, np.array(i), np.array(j), o, batch, "unlisted short read")
    # align_pairs: empty lists, handles of another aligner, checks before any upload
    for scope in ("score", "full"):
        wb = WavefrontAligner(scope=scope)
        out = wb.align_pairs(seqs, i=[], j=[])
        assert out["score"].shape == (0,) and out["status"].shape == (0,) and out["score"].dtype == np.int32
        if scope == "full":
            assert len(out["cigarstrings"]) == 0 and len(out["cigar_ops"]) == 0
        out = wb.align_pairs([], i=np.zeros(0, np.int64), j=np.zeros(0, np.int64))
        assert out["score"].shape == (0,)
    with wa.sequence_set(seqs) as S:
        with pytest.raises(ValueError, match="another aligner"):
            WavefrontAligner().align_pairs(S, i=[0], j=[0])
        with pytest.raises(ValueError, match="another aligner"):
            WavefrontAligner().nearest(S, k=1)
        with pytest.raises(ValueError, match="out of range"):
            wa.align_pairs(S, i=[4], j=[0])
        with pytest.raises(ValueError, match="negative"):
            wa.align_pairs(S, i=[0], j=[-1])
        check_python(kw, S, None, i, j, o, batch, "usable afterwards", aligner=wa)


@pytest.mark.gpu
def test_chunked_lists(gpu, monkeypatch):
    """Lists longer than the pair budget run in consecutive chunks and come back joined."""
    kw = dict(span="end-to-end")
    i, j = pair_list(15, FAM, FAM, 2500, same=True)
    o, batch = oracle_pairs(kw, READS, None, i, j)
    monkeypatch.setenv("WFA_HIP_PAIRS_BAND", "700")
    check_python(kw, READS, None, i, j, o, batch, "chunks of 700")
    o, batch = oracle_pairs(dict(kw, scope="score"), READS, None, i, j)
    check_python(dict(kw, scope="score"), READS, None, i, j, o, batch, "chunks of 700, score")


@pytest.mark.gpu
def test_workflow_nearest_then_align(gpu):
    """Find the hits, then align them: nearest() on open handles, its padding filtered, align_pairs with scope full."""
    reads, _ = family_reads(51, 30, 8, 120, 200, div=0.02)
    loners, _ = family_reads(52, 3, 1, 120, 200)
    queries = [reads[f * 8 + c] for f in range(30) for c in range(2)] + loners      # the loners have no hit: rows of padding
    cands = [reads[f * 8 + c] for f in range(30) for c in range(2, 8)] + [""]
    kw = dict(span="end-to-end", scope="full", max_steps=60)
    a = WavefrontAligner(**kw)
    with a.sequence_set(queries) as Q, a.sequence_set(cands) as C:
        near = a.nearest(Q, C, k=4)
        keep = near["j"] >= 0
        assert keep.any() and not keep.all()
        i = np.nonzero(keep)[0]
        j = near["j"][keep]
        with pytest.raises(ValueError, match="negative"):
            a.align_pairs(Q, C, i=np.repeat(np.arange(len(queries)), 4), j=near["j"].reshape(-1))
        o, batch = oracle_pairs(kw, queries, cands, i, j)
        out = check_python(kw, Q, C, i, j, o, batch, "workflow", aligner=a)
    assert np.array_equal(out["score"], near["score"][keep])
    assert (out["status"] == 0).all()
