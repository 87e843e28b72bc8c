"""Shared by the tests of the SAM fields (test_sam_abi.py, test_sam_gpu.py): the rule restated in plain Python, straight from the text of
include/wfa_hip.h ("SAM fields"); an independent check that rebuilds the reference span from the read, the CIGAR and the MD string
alone; the oracle's strings of the repeat corpus; and the window list of the GPU tests.  Expected fields are the rule applied to the
ORACLE's op strings, never to the device's output."""
import functools
import re

import numpy as np

from leftalign_common import METRICS, _random, py_left_align, repeat_corpus
from oracle import loader
from pywfa_amd import datagen
from test_windows_gpu import as_list, materialise, revcomp

EQX, CORE = 1, 2
FLAGS = (0, EQX, CORE, EQX | CORE)
UNMAPPED = ((-1, 0, 0, 0, 0, 0, 0, 0), b"", b"")
MD_FORM = re.compile(rb"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*")
ENDS_FREE = dict(span="ends-free", pattern_begin_free=12, pattern_end_free=12, text_begin_free=12, text_end_free=12)


def py_sam(ops, text, flags=0, status=0):
    """The rule for one pair: (the row of 8, the CIGAR, the MD string)."""
    ops, T = bytes(ops), bytes(text)
    anchors = b"M" if flags & CORE else b"MX"
    at = [k for k, c in enumerate(ops) if c in anchors]
    if status != 0 or not at:
        return UNMAPPED
    f, l = at[0], at[-1]
    before, span, after = ops[:f], ops[f:l + 1], ops[l + 1:]
    count = lambda s, letters: sum(c in letters for c in s)   # noqa: E731
    pos, clip_left, clip_right = count(before, b"XI"), count(before, b"XD"), count(after, b"XD")
    letter = {"M": "=" if flags & EQX else "M", "X": "X" if flags & EQX else "M", "D": "I", "I": "D"}
    mapped = "".join(letter[chr(c)] for c in span)
    cigar = f"{clip_left}S" if clip_left else ""
    cigar += "".join(f"{len(m.group(0))}{m.group(1)}" for m in re.finditer(r"(.)\1*", mapped))
    cigar += f"{clip_right}S" if clip_right else ""
    md, run, h = "", 0, pos
    for k, c in enumerate(span):
        c = chr(c)
        if c == "M":
            run += 1
        elif c == "X":
            md, run = md + f"{run}{chr(T[h])}", 0
        elif c == "I":
            if span[k - 1:k] != b"I":
                md, run = md + f"{run}^", 0
            md += chr(T[h])
        h += c in "MXI"
    md += str(run)
    row = (pos, count(span, b"MXI"), clip_left, clip_right, count(span, b"XID"), len(cigar), len(md), count(span, b"MXD"))
    return row, cigar.encode(), md.encode()


def ref_from(read, cigar, md):
    """The reference bases a read covers, rebuilt as a SAM reader would: the CIGAR lays the read's aligned bases over the reference with
    gaps for the deleted ones, the MD string then names every reference base that is not the read's.  None if the two disagree."""
    cig = [(int(n), c) for n, c in re.findall(r"(\d+)([MIDS=X])", cigar)]
    if "".join(f"{n}{c}" for n, c in cig) != cigar:
        return None
    cols, r = [], 0    # one entry per reference base of the span: the read's base, or None under a deletion
    for n, c in cig:
        if c in "M=X":
            cols += list(read[r:r + n])
        if c == "D":
            cols += [None] * n
        if c in "M=XIS":
            r += n
    if r != len(read):
        return None
    out, k = [], 0
    for num, dele, sub in re.findall(r"(\d+)|\^([A-Z]+)|([A-Z])", md):
        if num:
            n = int(num)
            if any(b is None for b in cols[k:k + n]) or k + n > len(cols):
                return None
            out += cols[k:k + n]
            k += n
        elif dele:
            if cols[k:k + len(dele)] != [None] * len(dele):
                return None
            out += list(dele)
            k += len(dele)
        else:
            if k >= len(cols) or cols[k] is None:
                return None
            out.append(sub)
            k += 1
    return "".join(out) if k == len(cols) else None


def span_counts(ops, flags):
    """(X, I, D) of the span of an op string with an anchor"""
    anchors = b"M" if flags & CORE else b"MX"
    at = [k for k, c in enumerate(ops) if c in anchors]
    span = ops[at[0]:at[-1] + 1]
    return span.count(b"X"), span.count(b"I"), span.count(b"D")


@functools.lru_cache(maxsize=None)
def corpus_strings(metric, ends_free=False):
    """The oracle's op strings and statuses of the repeat corpus under `metric`, end to end or with every end free."""
    pats, txts = repeat_corpus()
    kw = dict(ENDS_FREE if ends_free else dict(span="end-to-end"), **METRICS[metric])
    o = loader.run(loader.oracle(), loader.make_config(**kw), datagen.from_strings(list(pats), list(txts), upper=True))
    return pats, txts, o["cigars"], o["status"]


# ---- the window list of the GPU tests -------------------------------------------------------------------------------------------------

KW = dict(span="end-to-end")
MAX_STEPS = 6


def _other(c):
    return "ACGT"[("ACGT".index(c) + 1) % 4]


def _sub(s, k):
    return s[:k] + _other(s[k]) + s[k + 1:]


@functools.lru_cache(maxsize=None)
def gpu_list(seed=11):
    """Reads against windows of two references, built like the list of leftalign_common: every pair is one planted shape.  Returns refs,
    reads, the window list W, `names` (name -> pair) and `free` (the pairs of the ends-free sub-list, which is run on its own)."""
    rng = np.random.default_rng(seed)
    ref_parts, reads, rows, names = [[], []], [], [], {}
    ref_len = [0, 0]

    def add(name, text, read, r=0, rev=False):
        lead, tail = _random(rng, 7), _random(rng, 5)
        t0 = ref_len[r] + len(lead)
        ref_parts[r] += [lead, text, tail]
        ref_len[r] += len(lead) + len(text) + len(tail)
        names[name] = len(reads)
        rows.append((len(reads), r, 0, len(read), t0, len(text), int(rev)))
        reads.append(revcomp(read) if rev else read)

    def distinct(n):
        """n random bases without two equal neighbours: a gap in it has one place"""
        s = [_random(rng, 1)] if n else []
        while len(s) < n:
            c = _random(rng, 1)
            if c != s[-1]:
                s.append(c)
        return "".join(s)

    # op strings of length 0 .. 129: exact pairs; an empty pattern window, an empty text window
    for n in (0, 1, 63, 64, 65, 127, 128, 129):
        s = distinct(n)
        add(f"len_{n}", s, s, r=n % 2)
    add("empty_pattern", distinct(9), "")
    add("empty_text", "", distinct(9), r=1)
    # match runs of exactly 9 .. 1000 between two substitutions, and one exact pair of 1 100 bases
    for n in (9, 10, 99, 100, 999, 1000):
        s = distinct(n + 42)
        add(f"match_{n}", s, _sub(_sub(s, 20), 21 + n), r=n % 2, rev=n in (99, 999))
    s = distinct(1100)
    add("exact_1100", s, s)
    # runs that end at op 63 or 64, that straddle 63 / 64, and that cross three rounds: a gap of g bases whose last op is `end`
    for kind in "ID":
        for end, g in ((63, 5), (64, 5), (66, 7), (199, 140)):
            a, b = distinct(end + 1 - g), distinct(30)
            gap = distinct(g + 2)[1:-1]
            while gap[0] == b[0] or gap[-1] == a[-1] or gap[0] == a[-1] or gap[-1] == b[0]:
                gap = distinct(g + 2)[1:-1]
            more, less = a + gap + b, a + b
            text, read = (more, less) if kind == "I" else (less, more)
            add(f"gap_{kind}_{end}_{g}", text, read, r=end % 2, rev=end == 66)
    # an M run that ends at op 63 / 64 (an X behind it: the X at op 64 / 65), an X at op 63, X X adjacent, spans that start / end with X
    for k in (63, 64, 65):
        s = distinct(100)
        add(f"x_at_{k}", s, _sub(s, k), r=k % 2)
    s = distinct(80)
    add("xx", s, _sub(_sub(s, 30), 31))
    add("x_first", s, _sub(s, 0), r=1)
    add("x_last", s, _sub(s, 79))
    add("x_both", s, _sub(_sub(s, 0), 79), rev=True)
    add("all_x", "ACGT", "CATG")                       # no M at all
    # X directly before and directly after an I run; I run, D, I run
    a, b, g = distinct(40), distinct(40), "ACA"
    for name, read in (("x_before_i", _sub(a, 39) + b), ("x_after_i", a + _sub(b, 0))):
        add(name, a + g + b, read, r=1)
    # the byte path: an N in the read, an N in the text under an X, an N in the text inside a deleted run
    for k in range(4):
        a, b = distinct(40 + k), distinct(45)
        add(f"n_read_{k}", a + b, a[:10] + "N" + a[11:] + b, rev=k == 1)
        add(f"n_text_x_{k}", a[:10] + "N" + a[11:] + b, a + b, r=1)
        add(f"n_text_del_{k}", a + "GNT" + b, a + b, rev=k == 2)
    # random repeat pairs (several events per read, both kinds), either strand
    pats, txts = repeat_corpus(160, seed + 1)
    for k, (p, t) in enumerate(zip(pats, txts)):
        add(f"random_{k}", t, p, r=k % 2, rev=k % 3 == 0)
    # the ends-free sub-list: the read's ends hang over the window (leading / trailing D), or the window's over the read's (I)
    free = []
    for k in range(12):
        s = distinct(90 + k)
        hang_l, hang_r = distinct(3 + k % 4), distinct(2 + k % 5)
        name = f"free_{k}"
        if k % 2 == 0:
            add(name, s, hang_l + _sub(s, 40) + hang_r, r=k % 2, rev=k % 4 == 0)      # soft clips on both sides
        else:
            add(name, hang_l + s + hang_r, s[:50] + s[52:], r=k % 2, rev=k % 3 == 0)  # pos > 0
        free.append(names[name])
    refs = ["".join(parts) for parts in ref_parts]
    return refs, reads, as_list(rows), names, tuple(free)


def _select(W, idx):
    return {k: v[idx] for k, v in W.items()}


@functools.lru_cache(maxsize=None)
def gpu_expectation(metric="affine", part="main", max_steps=0, left_align=False):
    """The oracle's results of one part of the materialised list — "main" (end to end, everything but the ends-free sub-list) or "free"
    (that sub-list, every end free) — under `metric`, and per pair and flag combination the rule applied to its string."""
    refs, reads, W, names, free = gpu_list()
    idx = np.array(sorted(free) if part == "free" else [q for q in range(len(reads)) if q not in free])
    W = _select(W, idx)
    pats, txts = materialise(reads, refs, W)
    kw = dict(ENDS_FREE if part == "free" else KW, **METRICS[metric])
    if max_steps:
        kw["max_steps"] = max_steps
    o = loader.run(loader.oracle(), loader.make_config(**kw), datagen.from_strings(pats, txts, upper=True))
    strings = list(o["cigars"])
    if left_align:
        strings = [py_left_align(ops, p.encode(), t.encode())[0] if st == 0 else ops for ops, p, t, st in zip(strings, pats, txts, o["status"])]
    want = {fl: [py_sam(ops, t.encode(), fl, st) for ops, t, st in zip(strings, txts, o["status"])] for fl in FLAGS}
    return dict(kw=kw, refs=refs, reads=reads, W=W, names={k: int(np.flatnonzero(idx == v)[0]) for k, v in names.items() if v in idx},
                pats=pats, txts=txts, o=o, strings=strings, want=want)
