"""Shared by the tests of left alignment: the rule restated in plain Python, straight from the text of include/wfa_hip.h ("left
alignment"), the repeat corpus, and the window list of the GPU tests.  Expected strings are the rule applied to the ORACLE's op strings,
never to the device's output."""
import functools
import re

import numpy as np

from oracle import loader
from pywfa_amd import datagen
from reduce_common import core_of
from test_windows_gpu import LETTERS, as_list, materialise, revcomp

M, I, D = ord("M"), ord("I"), ord("D")


def expand(cigar):
    """"41M1D49M" -> one letter per op"""
    return b"".join(c.encode() * int(n) for n, c in re.findall(r"(\d+)([MXID])", cigar))


def py_left_align(ops, pattern, text):
    """The rule for one pair: (the rewritten ops, runs moved, merges)."""
    ops, P, T = bytearray(ops), bytes(pattern), bytes(text)
    core = core_of(ops)
    moved_runs = merges = 0
    if core is None:
        return bytes(ops), 0, 0
    first, last = core
    v = h = i = 0
    while i < last:
        c = ops[i]
        if i <= first or c not in (I, D):
            v += c in b"MXD"
            h += c in b"MXI"
            i += 1
            continue
        a, L = i, 0
        while ops[a + L] == c:
            L += 1
        end = a + L
        S, x = (T, h) if c == I else (P, v)
        moved = False
        while True:
            while a - 1 > first and ops[a - 1] == M and S[x - 1] == S[x + L - 1]:       # SHIFT
                ops[a - 1], ops[a + L - 1] = c, M
                a, x, moved = a - 1, x - 1, True
            if moved and a - 1 > first and ops[a - 1] == c:                              # MERGE
                n = 0
                while ops[a - 1 - n] == c:
                    n += 1
                a, x, L, merges = a - n, x - n, L + n, merges + 1
                continue
            break                                                                        # STOP
        moved_runs += moved
        if c == I:
            h += end - i
        else:
            v += end - i
        i = end
    return bytes(ops), moved_runs, merges


# ---- the repeat corpus --------------------------------------------------------------------------------------------------------------

def _random(rng, n):
    return "".join(LETTERS[rng.integers(0, 4, n)])


def _mutated(rng, s, rate=0.06):
    """A third each: substitution, deletion of 1-3, insertion of 1-3."""
    out, k = [], 0
    while k < len(s):
        r = rng.random()
        if r < rate / 3:
            out.append(LETTERS[(list("ACGT").index(s[k]) + int(rng.integers(1, 4))) % 4])
            k += 1
        elif r < 2 * rate / 3:
            k += int(rng.integers(1, 4))
        elif r < rate:
            out.append(_random(rng, int(rng.integers(1, 4))))
        else:
            out.append(s[k])
            k += 1
    return "".join(out)


@functools.lru_cache(maxsize=None)
def repeat_corpus(n=500, seed=20261):
    """Pairs (read, text): text = 30 random bases, a repeat, 20 random, a repeat, 30 random, the repeats of period 1-3 and 3-40
    copies; the read is the text mutated at 6 %."""
    rng = np.random.default_rng(seed)
    pats, txts = [], []
    for _ in range(n):
        rep = [_random(rng, int(rng.integers(1, 4))) * int(rng.integers(3, 41)) for _ in range(2)]
        t = _random(rng, 30) + rep[0] + _random(rng, 20) + rep[1] + _random(rng, 30)
        pats.append(_mutated(rng, t))
        txts.append(t)
    return tuple(pats), tuple(txts)


METRICS = {"affine": dict(distance="affine"), "levenshtein": dict(distance="levenshtein"), "indel": dict(distance="indel")}


@functools.lru_cache(maxsize=None)
def corpus_oracle(metric):
    """The oracle's results of the repeat corpus end to end under `metric`, and the rule applied to each of its strings."""
    pats, txts = repeat_corpus()
    kw = dict(span="end-to-end", **METRICS[metric])
    batch = datagen.from_strings(list(pats), list(txts), upper=True)
    o = loader.run(loader.oracle(), loader.make_config(**kw), batch)
    want = [py_left_align(ops, p.encode(), t.encode()) if st == 0 else (ops, 0, 0) for ops, p, t, st in zip(o["cigars"], pats, txts, o["status"])]
    return kw, batch, o, want


# ---- the window list of the GPU tests -------------------------------------------------------------------------------------------------

KW = dict(span="end-to-end")


def _unlike(rng, n, avoid):
    """n random bases, none of the letters in `avoid` at either end"""
    while True:
        s = _random(rng, n)
        if s[0] not in avoid and s[-1] not in avoid:
            return s


@functools.lru_cache(maxsize=None)
def gpu_list(seed=5):
    """Reads against windows of two references, each pair built around one repeat (or two) with a planted event, so that the oracle's
    gap sits at the right end of the repeat and the rule moves it.  Returns refs, reads, the window list W and `names`: name -> pair."""
    rng = np.random.default_rng(seed)
    ref_parts, reads, rows, names = [[], []], [], [], {}
    ref_len = [0, 0]

    def add(name, text, read, r=0, rev=False, pad=(0, 0)):
        """`text` goes into reference r between two random pads; the window is the text alone"""
        lead, tail = _random(rng, 7 + pad[0]), _random(rng, 5 + pad[1])
        t0 = ref_len[r] + len(lead)
        ref_parts[r] += [lead, text, tail]
        ref_len[r] += len(lead) + len(text) + len(tail)
        names[name] = len(reads)
        rows.append((len(reads), r, 0, len(read), t0, len(text), int(rev)))
        reads.append(revcomp(read) if rev else read)

    def flank(n, avoid):
        return _unlike(rng, n, avoid)

    # the round boundary: a one-base gap run that the oracle leaves at op 63 / 64 (and their neighbours) of a homopolymer
    for start in (62, 63, 64, 65, 127, 128):
        for kind in "ID":
            left, right = flank(start - 8, "A"), flank(30, "A")
            more, less = left + "A" * 9 + right, left + "A" * 8 + right
            text, read = (more, less) if kind == "I" else (less, more)
            add(f"round_{start}_{kind}", text, read, r=start % 2)
    # a shift of 65 - 130 ops: homopolymers of that length
    for n in (65, 66, 100, 127, 128, 129, 130):
        a, b = flank(20, "C"), flank(25, "C")
        add(f"shift_{n}_D", a + "C" * n + b, a + "C" * (n + 1) + b)
        add(f"shift_{n}_I", a + "C" * (n + 1) + b, a + "C" * n + b, rev=True)
    # a run longer than 64: a 70-base deletion inside a 200-base period-2 repeat, and the insertion
    a, b = flank(33, "GT"), flank(31, "GT")
    add("long_I", a + "GT" * 100 + b, a + "GT" * 65 + b)
    add("long_D", a + "GT" * 65 + b, a + "GT" * 100 + b, r=1)
    # periods 1, 2 and 3
    for unit in ("T", "CA", "GAT"):
        for copies in (5, 23):
            a, b = flank(40, unit), flank(41, unit)
            add(f"period_{unit}_{copies}_D", a + unit * copies + b, a + unit * (copies + 1) + b, rev=copies == 23)
            add(f"period_{unit}_{copies}_I", a + unit * (copies + 1) + b, a + unit * copies + b, r=1)
    # two runs of one pair: two deletions in one homopolymer that a substitution in the read separates; the second run shifts over
    # the Ms the first left behind when the repeats touch (one homopolymer, two one-base runs under the one-component metrics)
    a, b = flank(30, "A"), flank(30, "A")
    add("two_runs", a + "A" * 30 + b, a + "A" * 12 + "G" + "A" * 14 + b)
    add("two_repeats", a + "A" * 12 + "CA" * 9 + b, a + "A" * 11 + "CA" * 8 + b)
    add("two_kinds", a + "A" * 12 + b[:5] + "CA" * 9 + b, a + "A" * 13 + b[:5] + "CA" * 8 + b)
    # a substitution inside the repeat stops the run; a read that ends inside the repeat
    add("stopped", a + "A" * 20 + b, a + "A" * 8 + "T" + "A" * 10 + b)
    add("ends_inside", a + "A" * 20, a + "A" * 19)
    # the byte path: an N in the read outside the repeat, beside 2-bit pairs
    a2 = a[:10] + "N" + a[11:]
    add("bytes_D", a + "C" * 12 + b, a2 + "C" * 13 + b)
    add("bytes_I", a + "GA" * 12 + b, a2 + "GA" * 11 + b, rev=True)
    # random repeat pairs (as the corpus: more than one event per read, both kinds), either strand
    pats, txts = repeat_corpus(160, seed + 1)
    for k, (p, t) in enumerate(zip(pats, txts)):
        add(f"random_{k}", t, p, r=k % 2, rev=k % 3 == 0)
    refs = ["".join(parts) for parts in ref_parts]
    return refs, reads, as_list(rows), names


@functools.lru_cache(maxsize=None)
def gpu_expectation(metric="affine", max_steps=0):
    """The oracle's results of the materialised list under `metric` and, per pair, the rule applied to its string (a pair whose status
    is not 0 keeps its bytes)."""
    refs, reads, W, names = gpu_list()
    pats, txts = materialise(reads, refs, W)
    kw = dict(KW, **METRICS[metric])
    if max_steps:
        kw["max_steps"] = max_steps
    o = loader.run(loader.oracle(), loader.make_config(**kw), datagen.from_strings(pats, txts, upper=True))
    want = [py_left_align(ops, p.encode(), t.encode()) if st == 0 else (ops, 0, 0) for ops, p, t, st in zip(o["cigars"], pats, txts, o["status"])]
    return dict(kw=kw, refs=refs, reads=reads, W=W, names=names, pats=pats, txts=txts, o=o, want=want)
