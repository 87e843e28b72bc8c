"""Host-side mirror of pywfa's interface for the wavefront-alignment hot path.

``WavefrontAligner`` keeps the constructor kwargs, methods, properties, exceptions and result
objects of pywfa's Cython class (/root/reference/pywfa/align.pyx:306-883) and adds batch forms
(``wavefront_align_batch`` / ``align_batch``).  Every alignment — single pair or batch — runs on the
GPU through the C ABI of ``libwfa_hip.so`` (include/wfa_hip.h); there is no CPU path in this package
and constructing an aligner fails loudly when the library or a HIP device is missing.

Deliberate deviations from the reference (DESIGN.md §"Deviations"):
  * invalid penalties / ends-free sizes raise ``ValueError`` where WFA2-lib calls ``exit(1)``
    (wavefront_penalties.c:101-112, wavefront_align.c:95-101);
  * ``memory_mode="biwfa"``: ``scope="score"`` runs the ordinary score-only kernels (the reference returns the same
    scores there as in its other memory modes), ``scope="full"`` runs the breakpoint recursion on the device
    (csrc/wfa_biwfa.hpp); with a heuristic both directions of every breakpoint search cut their
    wavefronts off as the reference's do (wavefront_bialigner.c:53,161-166; both scopes); BiWFA with free ends raises ``NotImplementedError`` (the reference itself
    ``exit(1)``s, wavefront_align.c:60-75);
  * property setters re-derive the whole native configuration (the reference pokes single C fields
    and leaves derived state stale).
"""
import os
import sys

import numpy as np

from . import _native
from . import datagen

_NO_OPS = np.zeros(0, np.uint8)   # (the op string of a call without a backtrace: one read-only array for every such call)
_NO_OPS.flags.writeable = False

__all__ = ["WavefrontAligner", "AlignmentResult", "BatchResults", "Pileup", "clip_cigartuples", "cigartuples_to_str",
           "elide_mismatches_from_cigar"]

# CIGAR tuple codes (align.pyx:11-14, README.rst:61-86): M I D N S H P = X B
_OP_CODE = {ord("M"): 0, ord("I"): 1, ord("D"): 2, ord("N"): 3, ord("S"): 4, ord("H"): 5,
            ord("P"): 6, ord("="): 7, ord("X"): 8, ord("B"): 9}
_OP_CHARS = "MIDNSHP=XB"
_INT_MAX = 2147483647


class AlignmentResult:
    """Result object of ``WavefrontAligner.__call__`` (align.pyx:17-180)."""

    def __init__(self, pl, tl, ps, pe, ts, te, ct, s, p, t, status):
        self.pattern_length = pl
        self.text_length = tl
        self.pattern_start = ps
        self.pattern_end = pe
        self.text_start = ts
        self.text_end = te
        self.cigartuples = ct
        self.score = s
        self.pattern = p
        self.text = t
        self.status = status

    def __repr__(self):
        keys = ("score", "pattern_start", "pattern_end", "text_start", "text_end", "cigartuples",
                "pattern", "text")
        return "".join(f"    {k}: {self.__dict__[k]}\n" for k in keys)

    def __str__(self):
        score = "Score: %d" % self.score
        if self.pattern and self.cigartuples:
            t = self.aligned_text
            p = self.aligned_pattern
            if len(t) > 30:
                t = t[:30] + "..."
                p = p[:30] + "..."
            c = self.cigarstring[:30]
            return "\n".join([p, t, c, score, "Length: %d" % len(t)])
        return score

    def __eq__(self, other):
        return isinstance(other, AlignmentResult) and self.__dict__ == other.__dict__

    @staticmethod
    def _aligned(sequence, tuples, begin, end, gap_type):
        """``aligned_pattern`` / ``aligned_text``.  The reference reads every
        ``(code, run)`` tuple as ``(width, kind)`` and inserts a gap only where ``kind`` equals the gap letter; a run
        length is never a letter, so for tuples the aligner produced no gap is inserted, the pieces tile the window
        ``sequence[begin:end]`` and the result is that window.  Hand-made tuples whose second field IS the gap letter
        still get their dashes."""
        window = sequence[begin:end]
        if all(kind != gap_type for _, kind in tuples):
            return window
        pieces, at = [], 0
        for width, kind in tuples:
            if kind == gap_type:
                pieces.append("-" * width)
                continue
            pieces.append(window[at:at + width])
            at += width
        return "".join(pieces) + window[at:end - begin]

    @property
    def aligned_pattern(self):
        if self.pattern:
            return self._aligned(self.pattern, self.cigartuples, self.pattern_start, self.pattern_end, "D")
        return None

    @property
    def aligned_text(self):
        if self.text:
            return self._aligned(self.text, self.cigartuples, self.text_start, self.text_end, "I")
        return None

    @property
    def cigarstring(self):
        return cigartuples_to_str(self.cigartuples)

    # rows of the three-line view per cigartuple code: (takes pattern bases, takes text bases, glyph of the middle row);
    # M / = are joined by '|', X by '*', gaps and clips by blanks, anything else is refused
    _PRETTY_ROWS = {0: (True, True, "|"), 7: (True, True, "|"), 8: (True, True, "*"),
                    1: (False, True, " "), 4: (False, True, " "), 5: (False, True, " "),
                    2: (True, False, " ")}

    @property
    def pretty(self):
        """The CIGAR, the CIGAR without its match runs, and the PATTERN / marks / TEXT rows."""
        rows = {"p": "      PATTERN    ", "g": "                 ", "t": "      TEXT       "}
        used_p = used_t = 0
        for code, run in self.cigartuples:
            if code not in self._PRETTY_ROWS:
                raise ValueError(f"Cigar operation not available for pretty print - {code}")
            on_p, on_t, glyph = self._PRETTY_ROWS[code]
            rows["p"] += self.pattern[used_p:used_p + run] if on_p else "-" * run
            rows["t"] += self.text[used_t:used_t + run] if on_t else "-" * run
            rows["g"] += glyph * run
            used_p += run if on_p else 0
            used_t += run if on_t else 0
        # (the compact form drops the match runs only: the reference's second filter compares an int with a list)
        compact = cigartuples_to_str([ct for ct in self.cigartuples if ct[0] != 0])
        head = f"{self.cigarstring}      ALIGNMENT\n{compact}      ALIGNMENT.COMPACT\n"
        return head + rows["p"] + "\n" + rows["g"] + "\n" + rows["t"] + "\n"


def _flank_scan(ct, threshold_left, threshold_right, text_len, pattern_len):
    """Shared scan of clip_cigartuples / locations: skip ops at both flanks until an M run of at
    least the threshold (align.pyx:199-234, :797-831).  Returns (i, j, ps, pe, ts, te)."""
    ts = ps = 0
    i = 0
    for i in range(len(ct)):
        op, n = ct[i]
        if op == 0:
            if n >= threshold_left:
                break
            ts += n; ps += n
        elif op == 2:
            ps += n
        elif op == 8:
            ts += n; ps += n
        elif op == 1:
            ts += n
    te, pe = text_len, pattern_len
    j = len(ct) - 1
    for j in range(len(ct) - 1, -1, -1):
        op, n = ct[j]
        if op == 0:
            if n >= threshold_right:
                break
            te -= n; pe -= n
        elif op == 2:
            pe -= n
        elif op == 8:
            pe -= n; te -= n
        elif op == 1:
            te -= n
    return i, j, ps, pe, ts, te


def clip_cigartuples(align_result, min_aligned_bases_left=5, min_aligned_bases_right=5):
    """Trim flanking blocks with fewer aligned bases than the thresholds into soft-clips
    (align.pyx:183-250).  Mutates and returns ``align_result``; the score is not adjusted."""
    ct = align_result.cigartuples
    if not ct:
        return align_result
    i, j, ps, pe, ts, te = _flank_scan(ct, int(min_aligned_bases_left), int(min_aligned_bases_right),
                                       align_result.text_length, align_result.pattern_length)
    modified = []
    if align_result.text_start + ts > 0:
        modified.append((4, ts))
    modified += ct[i:j + 1]
    if align_result.text_length - te > 0:
        modified.append((4, align_result.text_length - te))
    align_result.cigartuples = modified
    align_result.text_start, align_result.text_end = ts, te
    align_result.pattern_start, align_result.pattern_end = ps, pe
    return align_result


def elide_mismatches_from_cigar(cigartuples):
    """Merge adjacent M (0) and X (8) runs into single M runs (align.pyx:253-277)."""
    if not cigartuples:
        return []
    out = []
    block = 0
    for op, n in cigartuples:
        if op == 0 or op == 8:
            block += n
        else:
            if block:
                out.append((0, block))
                block = 0
            out.append((op, n))
    if block:
        out.append((0, block))
    return out


def cigartuples_to_str(cigartuples):
    """``[(op, n), ...]`` -> ``"{n}{op}..."`` (align.pyx:280-295)."""
    if not cigartuples:
        return ""
    return "".join(f"{int(n)}{_OP_CHARS[op]}" for op, n in cigartuples)


def left_align_ops(ops, pattern, text):
    """Left-align one pair's op string on the host (no GPU): ``ops`` holds one letter per op (M X I D; a ``str``, ``bytes`` or a
    uint8 array: what ``cigar_ops`` gives), ``pattern`` and ``text`` are the pair's own letters (of a window: the window's, a
    reversed pattern reverse-complemented).  Inside the aligned core, first M to last M, every I or D run moves left over M ops
    while the letter that enters it equals the letter that leaves it, and joins a run of its own kind that it meets; a mismatch, a
    gap of the other kind and the core's first M stop it — the rule ``left_align=True`` applies on the GPU (include/wfa_hip.h,
    "left alignment").  Returns the rewritten ops in the type they came in.  ValueError when the ops do not consume exactly the
    pattern and the text."""
    as_bytes = [x.encode() if isinstance(x, str) else x for x in (ops, pattern, text)]
    out, _moved, _merges = _native.ops_left_align(*as_bytes)
    if isinstance(ops, str):
        return out.tobytes().decode()
    return out if isinstance(ops, np.ndarray) else out.tobytes()


def _rle(ops):
    """Run-length encode a uint8 array of op chars -> (chars, lengths)."""
    if ops.size == 0:
        return ops, np.zeros(0, np.int64)
    change = np.flatnonzero(ops[1:] != ops[:-1]) + 1
    starts = np.concatenate(([0], change))
    lengths = np.diff(np.concatenate((starts, [ops.size])))
    return ops[starts], lengths


def _ops_to_tuples(ops):
    ch, ln = _rle(ops)
    return [(_OP_CODE[int(c)], int(n)) for c, n in zip(ch, ln)]


def _ops_to_string(ops):
    ch, ln = _rle(ops)
    return "".join(f"{int(n)}{chr(int(c))}" for c, n in zip(ch, ln))


class _RunSequence:
    """Read-only sequence over the per-pair CIGAR runs of a batch (run-length encoded on the GPU: ``run_off`` int64[n+1],
    ``run_code`` uint8 = pywfa's cigartuple codes, ``run_len`` int32).  Items are built on access — a Python str per pair
    costs ~1 us, the alignment itself ~0.001 us — ``kind``: "str" = CIGAR string, "ops" = uint8 array of op characters."""

    _CHARS = np.frombuffer(_OP_CHARS.encode(), dtype=np.uint8)   # cigartuple code -> op character

    def __init__(self, run_off, run_code, run_len, kind):
        self._off, self._code, self._len, self._kind = run_off, run_code, run_len, kind

    def __len__(self):
        return len(self._off) - 1

    def _item(self, i):
        a, b = int(self._off[i]), int(self._off[i + 1])
        if self._kind == "str":
            return "".join(f"{n}{_OP_CHARS[c]}" for c, n in zip(self._code[a:b].tolist(), self._len[a:b].tolist()))
        return np.repeat(self._CHARS[self._code[a:b]], self._len[a:b])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._item(j) for j in range(*i.indices(len(self)))]
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(i)
        return self._item(i)

    def __iter__(self):
        return (self._item(i) for i in range(len(self)))


class _OpsSequence:
    """Read-only sequence over the per-pair op strings of a small batch (``ops`` uint8, ``begin`` / ``length`` per pair);
    ``kind``: "str" = CIGAR string (run-length encoded when read), "ops" = uint8 array of op characters."""

    def __init__(self, ops, begin, length, kind):
        self._ops, self._beg, self._len, self._kind = ops, begin, length, kind

    def __len__(self):
        return len(self._beg)

    def _item(self, i):
        o = self._ops[self._beg[i]:self._beg[i] + self._len[i]]
        return _ops_to_string(o) if self._kind == "str" else o

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._item(j) for j in range(*i.indices(len(self)))]
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(i)
        return self._item(i)

    def __iter__(self):
        return (self._item(i) for i in range(len(self)))


class _TextSequence:
    """Read-only sequence of ``str`` over a blob of strings laid end to end (``blob`` uint8, ``off`` int64[n + 1]): the CIGAR or MD
    strings of ``sam=True``, built on access like the items of ``_OpsSequence``."""

    def __init__(self, blob, off):
        self._blob, self._off = blob, off

    def __len__(self):
        return len(self._off) - 1

    def _item(self, i):
        return self._blob[int(self._off[i]):int(self._off[i + 1])].tobytes().decode("latin-1")

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._item(j) for j in range(*i.indices(len(self)))]
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(i)
        return self._item(i)

    def __iter__(self):
        return (self._item(i) for i in range(len(self)))


class BatchResults:
    """Results of a whole batch with the Python-side surface pre-computed on the device: ``score``,
    ``status``, run-length encoded CIGARs (``run_off``, ``run_code``, ``run_len``) and ``locations``
    (n x 4: pattern_start, pattern_end, text_start, text_end).  ``res[i]`` builds the AlignmentResult
    that ``WavefrontAligner.__call__`` would return for pair i."""

    def __init__(self, batch, score, status, run_off, run_code, run_len, locations):
        self._batch = batch
        self.score, self.status = score, status
        self.run_off, self.run_code, self.run_len = run_off, run_code, run_len
        self.locations = locations

    def __len__(self):
        return len(self.score)

    def cigartuples(self, i):
        a, b = int(self.run_off[i]), int(self.run_off[i + 1])
        return [(int(c), int(n)) for c, n in zip(self.run_code[a:b], self.run_len[a:b])]

    def cigarstring(self, i):
        return cigartuples_to_str(self.cigartuples(i))

    def __getitem__(self, i):
        p, t = datagen.pair_strings(self._batch, i)
        ps, pe, ts, te = (int(x) for x in self.locations[i])
        return AlignmentResult(len(p), len(t), ps, pe, ts, te, self.cigartuples(i), int(self.score[i]), p, t,
                               int(self.status[i]))


def _columns(rows, names):
    """The columns of an (n, len(names)) array as a dict of contiguous arrays."""
    return {name: np.ascontiguousarray(rows[:, c]) for c, name in enumerate(names)}


def _dup_columns(rows):
    """The four int32 arrays that ``duplicates=True`` adds to ``reads`` / ``pairs``, from rows in the columns DUP_COLUMNS."""
    rep, size, dup, overflow = (np.ascontiguousarray(rows[:, c]) for c in range(_native.DUP_COLS))
    return dict(dup=dup, dup_rep=rep, dup_size=size, dup_overflow=overflow)


def _summary_dict(rows):
    """The (n, 10) rows of ``ResidentBatch.summary()`` as the dict the ``summary=True`` forms return."""
    out = {name: np.ascontiguousarray(rows[:, k]) for k, name in enumerate(("M", "X", "I", "D", "I_runs", "D_runs"))}
    out["locations"] = np.ascontiguousarray(rows[:, 6:10])
    return out


def _need_full_for_summary(cfg, what="summary=True"):
    if cfg.scope != 1:
        raise ValueError(f"{what} needs scope='full'")


def _sam_flags(cfg, sam, eqx, clip_mismatches):
    """The flags of ``sam=True`` (None without it) after the checks of the three keywords."""
    if not sam:
        if eqx or clip_mismatches:
            raise ValueError(f"{'eqx' if eqx else 'clip_mismatches'}=True needs sam=True")
        return None
    _need_full_for_summary(cfg, "sam=True")
    return (_native.SAM_EQX if eqx else 0) | (_native.SAM_CORE if clip_mismatches else 0)


def _sam_dict(rows, cigar, md):
    """The rows and the two blobs of ``ResidentBatch.sam()`` (chunks joined end to end) as the dict ``sam=True`` returns."""
    out = {name: np.ascontiguousarray(rows[:, _native.SAM_COLUMNS.index(name)])
           for name in ("pos", "ref_len", "clip_left", "clip_right", "nm", "query_len")}
    for name, col, blob in (("cigar", 5, cigar), ("md", 6, md)):
        off = np.zeros(len(rows) + 1, np.int64)
        np.cumsum(rows[:, col], out=off[1:])
        out[name] = _TextSequence(blob, off)
    return out


_CALL_LETTERS = np.frombuffer(b"ACGTN-N", np.uint8)   # (CALL_CODES as letters; deleted bases are dropped before the lookup)


class _Closing:
    """``close()`` and the context manager of an object that owns one native handle, kept under the attribute ``_OWNS`` names."""

    _OWNS = None

    def close(self):
        handle = getattr(self, self._OWNS)
        if handle is not None:
            handle.close()
            setattr(self, self._OWNS, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class Pileup(_Closing):
    """Per-base counts over the text sequences, kept on the GPU (``WavefrontAligner.pileup``).  ``score`` / ``status``: the listed
    pairs' results, in list order.  ``counts(j)``: int32 rows of the columns ``COLUMNS`` for text ``j`` — reads whose aligned base is
    A, C, G, T or another letter, reads that delete the base, reads that insert in front of it, reads that mismatch (these are also
    under their letter).  ``depth(j)``: the reads whose aligned core covers each base.  Counters are int32 and not checked for
    overflow; the table takes 32 bytes per text base until ``close()`` (or the end of the ``with`` block).  ``calls`` / ``consensus`` /
    ``sites`` reduce the table on the GPU against the reference letters: a byte per base or a row per variant site comes back.  A
    pileup made with ``insertions=True`` also keeps what the reads insert (about 24 bytes per insertion and 1 byte per inserted base
    on the GPU): ``insertions`` gives one allele per insertion site, ``consensus(insertions=True)`` splices them in.  A pileup made
    with ``deletions=True`` also keeps every deletion as one event (16 bytes per deletion and 4 bytes per text base on the GPU):
    ``deletions`` gives one deletion length per site where deletions start, ``deletion_starts(j)`` how many start at each base.  A pileup made
    with ``strands=True`` also counts the forward reads on their own (32 more bytes per text base): ``counts`` / ``depth`` take
    ``strand="+"`` / ``"-"``, ``genotypes`` reports the forward counts and can ask for both strands (``min_alt_strand``)."""

    COLUMNS = _native.PILEUP_COLUMNS
    GENOTYPE_COLUMNS = _native.GENOTYPE_COLUMNS
    CALL_CODES = _native.CALL_CODES
    SITE_COLUMNS = _native.SITE_COLUMNS
    INSERTION_COLUMNS = _native.INSERTION_COLUMNS
    DELETION_COLUMNS = _native.DELETION_COLUMNS
    _OWNS = "_pileup"

    def __init__(self, native_pileup, score, status, aligner=None):
        self._pileup = native_pileup
        self.score = score
        self.status = status
        self._aligner = aligner

    def _open(self):
        if self._pileup is None or not self._pileup._h:
            raise ValueError("pileup is closed")
        return self._pileup

    def __len__(self):
        return self._open().n

    def counts(self, j, start=0, stop=None, strand=None):
        """int32 array of shape (stop - start, 8): the rows [start, stop) of text ``j`` (to its end when ``stop`` is None).
        ``strand``: None, every read; ``"+"`` / ``"-"``, the forward / the reverse reads only (a pileup made with ``strands=True``,
        else ValueError; the reverse counts are the total minus the forward ones)."""
        p = self._open()
        if strand is not None:
            if strand not in ("+", "-"):
                raise ValueError(f"strand = {strand!r}: \"+\", \"-\" or None")
            if not p.strands:
                raise ValueError("this pileup was not made to track strands: make it with pileup(..., strands=True)")
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 0 <= int(j) < p.n:
            raise ValueError(f"j = {j!r} is out of range for {p.n} text sequences")
        have = int(p.length[int(j)])
        start = int(start)
        stop = have if stop is None else int(stop)
        if not 0 <= start <= stop <= have:
            raise ValueError(f"rows [{start}, {stop}) are out of range for text sequence {int(j)} ({have} bases)")
        return p.read(int(j), start, stop - start, None if strand is None else int(strand == "-"))

    def depth(self, j, start=0, stop=None, strand=None):
        """The sum of the columns A, C, G, T, other and del: the contributing reads whose aligned core covers each base (``strand``
        as for ``counts``)."""
        return self.counts(j, start, stop, strand)[:, :6].sum(axis=1, dtype=np.int32)

    def quality_sums(self, j, start=0, stop=None):
        """int32 array of shape (stop - start, 8): the rows [start, stop) of text ``j`` of the QUALITY table of a pileup made with
        ``qualities=`` (else ValueError).  The columns are those of ``counts``; a cell is the sum of min(quality, ``quality_cap``)
        over the reads ``counts`` holds there: the base's own quality under a letter and under ``mismatch``, the smaller of the two
        neighbouring bases' under ``del``, the first inserted base's under ``ins``."""
        p = self._open()
        if not p.qualities:
            raise ValueError("this pileup was not made to track qualities: make it with pileup(..., qualities=...)")
        seq, start, stop = self._range(p, j, start, stop)
        return p.read_quality(seq, start, stop - start)

    def _range(self, p, j, start, stop):
        """The checked rows [start, stop) of text ``j`` (the wording of ``counts``)."""
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 0 <= int(j) < p.n:
            raise ValueError(f"j = {j!r} is out of range for {p.n} text sequences")
        have = int(p.length[int(j)])
        start = int(start)
        stop = have if stop is None else int(stop)
        if not 0 <= start <= stop <= have:
            raise ValueError(f"rows [{start}, {stop}) are out of range for text sequence {int(j)} ({have} bases)")
        return int(j), start, stop

    def _with_texts(self, p, texts, min_depth, run):
        """``run(native set)`` on the reference letters: a ``SequenceSet`` as it is, a list of ``str`` uploaded for this call."""
        if isinstance(min_depth, bool) or not isinstance(min_depth, (int, np.integer)) or not 1 <= int(min_depth) < 2**31:
            raise ValueError(f"min_depth = {min_depth!r} is out of range (an integer, at least 1)")
        al = self._aligner
        if al is None:
            raise ValueError("this Pileup was made without its aligner: calls and sites need it")
        if not isinstance(texts, (SequenceSet, list)):
            texts = list(texts)
        if len(texts) != p.n:
            raise ValueError(f"texts holds {len(texts)} sequences, the pileup was made over {p.n}")
        if isinstance(texts, list):
            for k, t in enumerate(texts):
                if len(t) != int(p.length[k]):
                    raise ValueError(f"texts[{k}] has {len(t)} bases, the pileup was made over {int(p.length[k])}")
        al._sync_wildcard()
        sets, mine = al._open_sets(texts, None)
        try:
            return run(sets[0])
        finally:
            for s in mine:
                s.close()

    def calls(self, texts, j, start=0, stop=None, min_depth=1):
        """The consensus call of the rows [start, stop) of text ``j``, made on the GPU (one byte per base comes back):
        dict(code=uint8 array, ins=bool array).  ``code`` indexes ``CALL_CODES``: the column among A, C, G, T, other, del with the most
        reads (among equals the reference's own letter, else the first), or 6, "no call", below ``min_depth`` covering reads; ``ins``:
        more than half of the covering reads insert in front of the base.  ``texts``: the ``SequenceSet`` or the list of ``str`` the
        pileup was made over (its letters are not kept by the pileup; a list is uploaded for the call)."""
        p = self._open()
        j, start, stop = self._range(p, j, start, stop)
        raw = self._with_texts(p, texts, min_depth, lambda t: p.calls(t, j, start, stop - start, int(min_depth)))
        return dict(code=raw & 7, ins=(raw & _native.CALL_INS) != 0)

    def _tracking(self):
        """The open native pileup, which must have been made with ``insertions=True``."""
        p = self._open()
        if not p.tracking:
            raise ValueError("this pileup was not made to track insertions: make it with pileup(..., insertions=True)")
        return p

    def consensus(self, texts, j, start=0, stop=None, min_depth=1, insertions=False):
        """The called sequence of the rows [start, stop) of text ``j`` as a ``str``: A, C, G, T; N for another letter and for no call;
        deleted bases are left out.  ``insertions=False``: the insertion flag of ``calls`` is ignored.  ``insertions=True`` (a pileup
        made with ``insertions=True``): in front of every base of the range whose ``calls()["ins"]`` is set — the first of the range
        and a base that is itself called deleted included — the allele most of the inserting reads carry (``insertions`` under the
        majority rule) is spliced in; a row over ``WFA_HIP_INS_MAX_READS`` splices nothing.  The splice is made on the host from the
        two small results."""
        if not insertions:
            code = self.calls(texts, j, start, stop, min_depth)["code"]
            return _CALL_LETTERS[code[code != 5]].tobytes().decode()
        p = self._tracking()
        j, start, stop = self._range(p, j, start, stop)

        def both(t):
            return p.calls(t, j, start, stop - start, int(min_depth)), p.insertions(t, j, start, stop - start, int(min_depth), 0)

        raw, (_, rows, _, letters) = self._with_texts(p, texts, min_depth, both)
        code = raw & 7
        # a row's letters go in front of its base; then the deleted bases (not the letters in front of them) are dropped
        at = np.repeat(rows[:, 1] - start, rows[:, 5])
        seq = np.insert(_CALL_LETTERS[code], at, letters)
        return seq[np.insert(code != 5, at, True)].tobytes().decode()

    def insertions(self, texts, j=None, start=0, stop=None, min_depth=1, min_frac=0.5):
        """What the reads insert, reduced on the GPU to one allele per site (a pileup made with ``insertions=True``): a dict of int32
        arrays ``INSERTION_COLUMNS`` in ascending (j, pos), plus ``seq``, a list of ``str``: per row the inserted bases (A, C, G, T, N
        for another letter) in front of base ``pos`` of text ``j``.  Rows: the bases covered by at least ``min_depth`` reads where at
        least ``min_frac`` of them insert (the ``ins`` condition of ``sites``; ``min_frac``, ``j``, ``start``, ``stop`` as there).  The
        allele is the inserted sequence most of the row's inserting reads carry (``allele_count`` of ``ins_count``; ties go to the
        shorter, then to the alphabetically smaller in the order A C G T N); ``alleles``: how many different ones they carry.  A row
        with more than ``WFA_HIP_INS_MAX_READS`` (4096) inserting reads has ``overflow`` = 1, zeros and ``""``.  Multi-base
        substitutions, a strand per inserting read and more than one allele per row are out of scope."""
        p = self._tracking()
        if isinstance(min_frac, bool) or not isinstance(min_frac, (int, float, np.integer, np.floating)) or not 1 <= round(float(min_frac) * 1000) <= 1000:
            raise ValueError(f"min_frac = {min_frac!r} is out of range (0.001 .. 1)")
        permille = int(round(float(min_frac) * 1000))
        if j is None:
            if start != 0 or stop is not None:
                raise ValueError("j = None takes every text: start and stop go with one text")
            seq, start, length = -1, 0, -1
        else:
            seq, start, stop = self._range(p, j, start, stop)
            length = stop - start
        _, rows, _, letters = self._with_texts(p, texts, min_depth, lambda t: p.insertions(t, seq, start, length, int(min_depth), permille))
        out = _columns(rows, self.INSERTION_COLUMNS)
        text = letters.tobytes().decode()
        ends = np.cumsum(rows[:, 5].astype(np.int64))
        out["seq"] = [text[int(e - n):int(e)] for e, n in zip(ends, rows[:, 5])]
        return out

    def _tracking_deletions(self):
        """The open native pileup, which must have been made with ``deletions=True``."""
        p = self._open()
        if not p.deletions_tracked:
            raise ValueError("this pileup was not made to track deletions: make it with pileup(..., deletions=True)")
        return p

    def deletions(self, texts, j=None, start=0, stop=None, min_depth=1, min_frac=0.5):
        """What the reads delete, reduced on the GPU to one deletion per site (a pileup made with ``deletions=True``): a dict of int32
        arrays ``DELETION_COLUMNS`` in ascending (j, pos).  ``pos`` is the first deleted base of text ``j``, 0-based (VCF anchors the
        event one base earlier); ``del_count`` the reads whose deletion starts there.  Rows: the bases covered by at least
        ``min_depth`` reads where at least ``min_frac`` of them start a deletion (``min_frac``, rounded to permille, ``j``, ``start``,
        ``stop`` as for ``sites``; ``min_frac=0``: more than half of them).  A row is selected by where it starts, so its deleted bases
        may reach past ``stop``.  ``allele_len`` is the length most of those reads delete (``allele_count`` of ``del_count``; ties go
        to the shorter); ``alleles``: how many different lengths they delete.  A row with more than ``WFA_HIP_DEL_MAX_READS`` (4096)
        such reads has ``overflow`` = 1 and zeros.  The deleted letters are the reference's: ``texts[j][pos:pos + allele_len]``.
        Multi-base substitutions, genotypes and strand counts per deletion allele and more than one allele per row are out of scope."""
        p = self._tracking_deletions()
        if isinstance(min_frac, bool) or not isinstance(min_frac, (int, float, np.integer, np.floating)) or not 0 <= round(float(min_frac) * 1000) <= 1000:
            raise ValueError(f"min_frac = {min_frac!r} is out of range (0 .. 1)")
        permille = int(round(float(min_frac) * 1000))
        if j is None:
            if start != 0 or stop is not None:
                raise ValueError("j = None takes every text: start and stop go with one text")
            seq, start, length = -1, 0, -1
        else:
            seq, start, stop = self._range(p, j, start, stop)
            length = stop - start
        _, rows = self._with_texts(p, texts, min_depth, lambda t: p.deletions(t, seq, start, length, int(min_depth), permille))
        return _columns(rows, self.DELETION_COLUMNS)

    def deletion_starts(self, j, start=0, stop=None):
        """int32 array of length stop - start: how many reads' deletions START at each of the rows [start, stop) of text ``j`` (a
        pileup made with ``deletions=True``, else ValueError).  The reads that delete a base at all are ``counts(j)[:, 5]``."""
        p = self._tracking_deletions()
        seq, start, stop = self._range(p, j, start, stop)
        return p.deletion_starts(seq, start, stop - start)

    def sites(self, texts, j=None, start=0, stop=None, min_depth=1, min_frac=0.5):
        """The bases where the reads disagree with the reference, found on the GPU (only their rows come back): a dict of int32 arrays
        ``SITE_COLUMNS`` in ascending (j, pos).  Among bases covered by at least ``min_depth`` reads, a site is one whose strongest
        column other than the reference's letter holds at least ``min_frac`` of the covering reads (``alt`` its column in
        ``CALL_CODES``, 5 = deleted; ``alt_count``), or where at least ``min_frac`` of them insert in front of the base (``ins_count``;
        ``alt`` = -1 and ``alt_count`` = 0 when only this holds).  ``min_frac`` is rounded to permille.  ``j=None``: every text (then
        ``start`` / ``stop`` must be left alone); otherwise the rows [start, stop) of text ``j``.  A deletion of several
        bases is a site per base here and one event in ``deletions``, on a pileup made with ``deletions=True``; multi-base substitutions are
        out of scope; base qualities: ``pileup(..., qualities=)``; what was inserted: ``insertions``, on a pileup made with ``insertions=True``; strands and genotypes:
        ``genotypes``."""
        p = self._open()
        if isinstance(min_frac, bool) or not isinstance(min_frac, (int, float, np.integer, np.floating)) or not 1 <= round(float(min_frac) * 1000) <= 1000:
            raise ValueError(f"min_frac = {min_frac!r} is out of range (0.001 .. 1)")
        permille = int(round(float(min_frac) * 1000))
        if j is None:
            if start != 0 or stop is not None:
                raise ValueError("j = None takes every text: start and stop go with one text")
            seq, start, length = -1, 0, -1
        else:
            seq, start, stop = self._range(p, j, start, stop)
            length = stop - start
        _, rows = self._with_texts(p, texts, min_depth, lambda t: p.sites(t, seq, start, length, int(min_depth), permille))
        return _columns(rows, self.SITE_COLUMNS)

    def genotypes(self, texts, j=None, start=0, stop=None, min_depth=8, min_frac=0.2, err_q=20, min_alt_strand=0, qualities=False):
        """The sites with a diploid genotype each, made on the GPU: a dict of int32 arrays ``GENOTYPE_COLUMNS`` in ascending (j, pos).
        The first eight are the columns of ``sites`` (same ``texts``, ``j``, ``start``, ``stop``, ``min_depth``, ``min_frac``).
        ``gt`` / ``gq``: 0, 1 or 2 copies of ``alt`` and a confidence 0..99, from ``ref_count`` and ``alt_count`` alone — the
        smallest of err_q * alt_count (0/0), 3 * (ref_count + alt_count) (0/1) and err_q * ref_count (1/1), and its distance to the
        next; a documented confidence, not a calibrated likelihood (no qualities enter it).  ``ins_gt`` / ``ins_gq``: the same for
        the insertion in front of the base, from ``ins_count`` and the reads that cover the base without one.  A pair is -1, -1 where
        the site has no such event.  ``depth_fwd``, ``ref_fwd``, ``alt_fwd``, ``ins_fwd``: the forward reads among ``depth``,
        ``ref_count``, ``alt_count``, ``ins_count`` (a pileup made with ``strands=True``; -1 otherwise) — the reverse ones are the
        difference, the strand test is the caller's.  ``min_alt_strand`` > 0 (needs ``strands=True``): an event counts only when at
        least that many reads of EACH strand carry it.  ``qualities=True`` (a pileup made with ``qualities=``, else ValueError): the
        costs come from ``quality_sums`` instead of ``err_q`` — the summed qualities of the alt reads (0/0) and of the ref reads
        (1/1); for the insertion those of the inserting reads (0/0), while reads that do not insert keep ``err_q`` each (1/1).
        More than one alternate allele per site and ploidy other than 2 are out of scope."""
        p = self._open()
        if qualities and not p.qualities:
            raise ValueError("qualities=True needs a pileup made to track qualities: make it with pileup(..., qualities=...)")
        if isinstance(min_frac, bool) or not isinstance(min_frac, (int, float, np.integer, np.floating)) or not 1 <= round(float(min_frac) * 1000) <= 1000:
            raise ValueError(f"min_frac = {min_frac!r} is out of range (0.001 .. 1)")
        permille = int(round(float(min_frac) * 1000))
        if isinstance(err_q, bool) or not isinstance(err_q, (int, np.integer)) or not 1 <= int(err_q) <= 60:
            raise ValueError(f"err_q = {err_q!r} is out of range (an integer, 1 .. 60)")
        if isinstance(min_alt_strand, bool) or not isinstance(min_alt_strand, (int, np.integer)) or not 0 <= int(min_alt_strand) < 2**31:
            raise ValueError(f"min_alt_strand = {min_alt_strand!r} is out of range (an integer, at least 0)")
        if int(min_alt_strand) > 0 and not p.strands:
            raise ValueError("min_alt_strand > 0 needs a pileup made to track strands: make it with pileup(..., strands=True)")
        if j is None:
            if start != 0 or stop is not None:
                raise ValueError("j = None takes every text: start and stop go with one text")
            seq, start, length = -1, 0, -1
        else:
            seq, start, stop = self._range(p, j, start, stop)
            length = stop - start
        _, rows = self._with_texts(p, texts, min_depth,
                                   lambda t: p.genotypes(t, seq, start, length, int(min_depth), permille, int(err_q), int(min_alt_strand),
                                                         qualities=bool(qualities)))
        return _columns(rows, self.GENOTYPE_COLUMNS)


class SequenceSet(_Closing):
    """Sequences kept on the GPU, uploaded and packed once (``WavefrontAligner.sequence_set``): pass it wherever ``score_matrix``,
    ``completed_pairs``, ``nearest`` and ``align_pairs`` take a list of sequences.  ``len()`` is the number of sequences; ``close()``
    (or leaving the ``with`` block) releases the device memory.  Results already returned stay valid."""

    _OWNS = "_set"

    def __init__(self, aligner, native_set):
        self._aligner = aligner
        self._set = native_set

    def __len__(self):
        if self._set is None:
            raise ValueError("sequence set is closed")
        return self._set.n


class QualitySet(_Closing):
    """The base qualities of a set of reads kept on the GPU, a byte per base, uploaded once (``WavefrontAligner.quality_set``): pass
    it as ``pileup(..., qualities=)`` with the reads it was made for.  ``len()`` is the number of reads; ``close()`` (or leaving the
    ``with`` block) releases the device memory."""

    _OWNS = "_set"

    def __init__(self, aligner, native_set):
        self._aligner = aligner
        self._set = native_set

    def __len__(self):
        if self._set is None:
            raise ValueError("quality set is closed")
        return self._set.n


def _quality_blob(quals, lengths, offset):
    """The qualities of ``len(lengths)`` reads as the library takes them, (uint8 blob of raw phred, int64 offsets, int32 lengths), or
    ValueError naming the first offending entry.  An entry: ``str`` / ``bytes`` of phred + ``offset`` (the fourth line of a FASTQ
    record), or a uint8 array of raw phred (``offset`` plays no part)."""
    if isinstance(offset, bool) or not isinstance(offset, (int, np.integer)) or not 0 <= int(offset) <= 255 - _native.MAX_QUALITY:
        raise ValueError(f"offset = {offset!r} is out of range (an integer, 0 .. {255 - _native.MAX_QUALITY})")
    if isinstance(quals, (str, bytes, np.ndarray)) or not hasattr(quals, "__len__"):
        raise ValueError("qualities must be a list with one entry per read (str, bytes or a uint8 array each)")
    n = len(lengths)
    if len(quals) != n:
        raise ValueError(f"qualities has {len(quals)} entries, the reads are {n}")
    parts = []
    for k, q in enumerate(quals):
        if isinstance(q, str):
            try:
                q = q.encode("ascii")
            except UnicodeEncodeError:
                raise ValueError(f"qualities[{k}] holds a character outside ASCII") from None
        if isinstance(q, (bytes, bytearray)):
            a = np.frombuffer(bytes(q), np.uint8).astype(np.int32) - int(offset)
        elif isinstance(q, np.ndarray) and q.dtype == np.uint8 and q.ndim == 1:
            a = q.astype(np.int32)
        else:
            raise ValueError(f"qualities[{k}] must be a str, bytes or a one-dimensional uint8 array, got {type(q).__name__}")
        if a.shape[0] != int(lengths[k]):
            raise ValueError(f"qualities[{k}] has {a.shape[0]} values, read {k} has {int(lengths[k])} bases")
        bad = np.flatnonzero((a < 0) | (a > _native.MAX_QUALITY))
        if len(bad):
            x = int(bad[0])
            raise ValueError(f"qualities[{k}][{x}] = {int(a[x])} is out of range (phred 0 .. {_native.MAX_QUALITY})")
        parts.append(a.astype(np.uint8))
    length = np.asarray(lengths, dtype=np.int32)
    off = np.zeros(n, np.int64)
    if n:
        off[1:] = np.cumsum(length[:-1], dtype=np.int64)
    blob = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return blob, off, length


def _quality_param(name, value, lo):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= _native.MAX_QUALITY:
        raise ValueError(f"{name} = {value!r} is out of range (an integer, {lo} .. {_native.MAX_QUALITY})")
    return int(value)


def _seed_param(name, value, lo, hi=None):
    """An integer parameter of the seed finder inside its range, or ValueError naming it and its value."""
    want = f"{lo} .. {hi}" if hi is not None else f"at least {lo}"
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name} must be an integer ({want}), got {value!r}")
    if value < lo or (hi is not None and value > hi):
        raise ValueError(f"{name} = {value} is out of range ({want})")
    return int(value)


class SeedIndex(_Closing):
    """An exact-match k-mer index over text sequences, kept on the GPU (``WavefrontAligner.seed_index``): ``seeds(patterns)`` finds
    every read's best candidate windows on both strands, in the shape ``align_windows`` and ``pileup`` take.  ``stats()``:
    dict(positions=, masked_kmers=, table_bytes=, build_ms=, query_ms=).  The index takes 4^k * 4 bytes plus 8 bytes per indexed
    position until ``close()`` (or the end of the ``with`` block) and stays valid after the texts' set is closed."""

    _OWNS = "_index"

    def __init__(self, aligner, native_index):
        self._aligner = aligner
        self._index = native_index

    def _open(self):
        if self._index is None or not self._index._h:
            raise ValueError("seed index is closed")
        return self._index

    def __len__(self):
        return self._open().n

    @property
    def k(self):
        """The k-mer length of the index."""
        return self._open().params()["k"]

    @property
    def w(self):
        """The minimizer window of the index, ``None`` for a stride index."""
        return self._open().params()["w"] or None

    @property
    def stride(self):
        """The stride of the index (1 for a minimizer index)."""
        return self._open().params()["stride"]

    def seeds(self, patterns, n=4, min_hits=2, gap=16, pad=16, max_hits=2048):
        """The ``n`` best clusters of exact k-mer hits of every read: dict of int32 arrays of shape (M, n) ``j`` (the text),
        ``reverse`` (1: the read's reverse complement matches), ``text_start`` / ``text_len`` (the window) and ``hits``, best
        first, rows padded with ``j = -1`` (as ``nearest`` pads), and ``overflow`` (uint8, M): 1 for a read with more than
        ``max_hits`` hits, which gets no seeds.  A cluster is a run of hits on one strand of one text whose diagonals
        (text position - read position) lie within ``gap`` of their neighbours; clusters below ``min_hits`` are dropped; the window
        spans the cluster's diagonals plus the read's length and ``pad`` on both sides, cut to the text.  ``patterns``: a list of
        ``str`` or a ``SequenceSet``.  ``n``: 1 .. 16, ``max_hits``: 1 .. 4096.  Under a minimizer index (``seed_index(w=...)``) only
        the read's own minimizers are looked up, so ``hits`` counts minimizers, about 2 / (w + 1) of what a dense index gives:
        ``min_hits`` wants a lower value than for a dense index."""
        index = self._open()
        n = _seed_param("n", n, 1, _native.SEED_MAX_N)
        min_hits = _seed_param("min_hits", min_hits, 1)
        gap = _seed_param("gap", gap, 0)
        pad = _seed_param("pad", pad, 0)
        max_hits = _seed_param("max_hits", max_hits, 1, _native.SEED_MAX_HITS)
        for name, v in (("min_hits", min_hits), ("gap", gap), ("pad", pad)):
            if v >= 2**31:
                raise ValueError(f"{name} = {v} does not fit 32 bits")
        a = self._aligner
        if not isinstance(patterns, (SequenceSet, list)):
            patterns = list(patterns)
        a._sync_wildcard()
        sets, mine = a._open_sets(patterns, None)
        try:
            return index.query(sets[0], n, min_hits, gap, pad, max_hits)
        finally:
            for s in mine:
                s.close()

    def chains(self, patterns, n=4, min_hits=3, min_score=40, lookback=32, max_dist=5000, band=500, pad=64, max_anchors=16384):
        """The ``n`` best co-linear chains of exact k-mer anchors of every read, for reads too long or too divergent for ``seeds``:
        dict of int32 arrays of shape (M, n) ``j``, ``reverse``, ``text_start`` / ``text_len`` (the text window, of the shape of a
        seed's), ``hits`` (the chain's anchors), ``score`` and ``pattern_start`` / ``pattern_len`` (the part of the stored read the
        chain spans), best first, rows padded with ``j = -1``, and ``overflow`` (uint8, M): 1 for a read with more than
        ``max_anchors`` anchors, which gets no chains.  All of it goes into ``align_windows`` / ``pileup`` as it is.  An anchor is an
        exact k-mer match of read position r and text position t; along the read an anchor joins the best of the ``lookback``
        anchors before it that lies on the same strand and text, at most ``max_dist`` behind it on both sequences and at most
        ``band`` off its diagonal; chains below ``min_hits`` anchors or ``min_score`` are dropped, and a chain inside the window of a
        better one is not reported again (the rule: include/wfa_hip.h, "chains").  ``patterns``: a list of ``str`` or a
        ``SequenceSet``.  ``n``: 1 .. 16, ``lookback``: 1 .. 64, ``max_dist``: 1 .. 2^20, ``band``: 0 .. 2^16, ``max_anchors``:
        1 .. 65536; the anchors take 32 bytes x ``max_anchors`` per resident workgroup of GPU memory, kept on the index.  Under a
        minimizer index (``seed_index(w=...)``) the anchors are minimizer matches, so ``hits`` and ``score`` count minimizers, about
        2 / (w + 1) of a dense index's anchors: ``min_hits`` and ``min_score`` want lower values than for a dense index."""
        index = self._open()
        n = _seed_param("n", n, 1, _native.SEED_MAX_N)
        min_hits = _seed_param("min_hits", min_hits, 1)
        min_score = _seed_param("min_score", min_score, 0)
        lookback = _seed_param("lookback", lookback, 1, _native.CHAIN_MAX_LOOKBACK)
        max_dist = _seed_param("max_dist", max_dist, 1, 1 << 20)
        band = _seed_param("band", band, 0, 1 << 16)
        pad = _seed_param("pad", pad, 0)
        max_anchors = _seed_param("max_anchors", max_anchors, 1, _native.CHAIN_MAX_ANCHORS)
        for name, v in (("min_hits", min_hits), ("min_score", min_score), ("pad", pad)):
            if v >= 2**31:
                raise ValueError(f"{name} = {v} does not fit 32 bits")
        a = self._aligner
        if not isinstance(patterns, (SequenceSet, list)):
            patterns = list(patterns)
        a._sync_wildcard()
        sets, mine = a._open_sets(patterns, None)
        try:
            return index.chain(sets[0], n, min_hits, min_score, lookback, max_dist, band, pad, max_anchors)
        finally:
            for s in mine:
                s.close()

    def stats(self):
        """dict(positions=, masked_kmers=, table_bytes=, build_ms=, query_ms=) and, of the last ``chains()``, chain_ms= and
        chain_workspace_bytes=."""
        index = self._open()
        st, ch = index.stats(), index.chain_stats()
        st.update(chain_ms=ch["kernel_ms"], chain_workspace_bytes=ch["workspace_bytes"])
        return st


class _Windows:
    """One call's window list (``WavefrontAligner._windows``).  Made: the arguments are checked (ValueError, nothing is uploaded) —
    ``arrays`` (i, j, pattern_start, pattern_len, text_start, text_len, reverse), ``wlen``, ``nreads`` (the patterns).  Entered: the
    wildcard is pushed and the sets are open — ``pset``, ``tset`` (None: one set), ``text_set`` (the set ``j`` points into) and
    ``run(**how)``.  Left: the sets this call uploaded are closed, a caller's ``SequenceSet`` stays open."""

    def __init__(self, aligner, *window_args):
        self._aligner = aligner
        self._patterns, self._texts, self.arrays, self.wlen = aligner._window_lists(*window_args)
        self.nreads = len(self._patterns)
        self._mine, self._attached, self._keep = [], None, False

    def __enter__(self):
        self._aligner._sync_wildcard()
        sets, self._mine = self._aligner._open_sets(self._patterns, self._texts)
        self.pset, self.text_set = sets[0], sets[-1]
        self.tset = sets[-1] if self._texts is not None else None
        return self

    def attach(self, handle, keep=False):
        """``handle`` (a table, a placer) is closed when the body is left; ``keep``: only when it raises."""
        self._attached, self._keep = handle, keep
        return handle

    def run(self, **how):
        return self._aligner._run_windows(self.pset, self.tset, self.arrays, self.wlen, **how)

    def __exit__(self, exc_type, *exc):
        if self._attached is not None and not (self._keep and exc_type is None):
            self._attached.close()
        for s in self._mine:
            s.close()
        return False


class WavefrontAligner:
    """Drop-in for ``pywfa.WavefrontAligner`` on the GPU. If a pattern is supplied it is cached.

    **Cost of a call.**  Every alignment, a single pair included, runs on the GPU (there is no CPU path).  One
    ``wavefront_align(text)`` of 150 bp reads costs about 14 us at the C ABI (``wfa_hip_align_pair``: host packs the pair into a
    pinned block, one wave aligns it, the host polls a completion flag), 19 us with the op string, a few us more through this
    class — against 1-2 us for pywfa on a host core.  A loop of single calls is exact but 10x slower than the reference's; the
    additive batch forms (``wavefront_align_batch``, ``align_batch``, ``align_batch_results``) are what this class is for:
    from about 32 pairs per call the GPU is ahead of one host core, at 10 M pairs per call by 300x (3 G alignments/s resident,
    0.3 G/s from host memory).
    """

    def __init__(self, pattern=None, distance="affine", memory_mode="high", match=0, mismatch=4,
                 gap_opening=6, gap_extension=2, gap_opening2=24, gap_extension2=1, scope="full",
                 span="ends-free", pattern_begin_free=0, pattern_end_free=0, text_begin_free=0,
                 text_end_free=0, heuristic=None, min_wavefront_length=10,
                 max_distance_threshold=50, steps_between_cutoffs=1, xdrop=20, wildcard=None,
                 max_steps=0, device=0, devices=None):
        self.pattern_len = 0
        self.text_len = 0
        self.alignment_score = 0
        self._pattern = None
        self._bpattern = None
        self._text = None
        if pattern:
            self._set_pattern(pattern)
        self._wildcard = None
        self._bwildcard = -1
        self.wildcard = wildcard
        cfg = _native.default_config()
        if distance not in _native.DIST:
            raise NotImplementedError(f"{distance} distance not implemented")
        cfg.distance = _native.DIST[distance]
        cfg.match, cfg.mismatch = int(match), int(mismatch)
        cfg.gap_opening, cfg.gap_extension = int(gap_opening), int(gap_extension)
        cfg.gap_opening2, cfg.gap_extension2 = int(gap_opening2), int(gap_extension2)
        if scope not in _native.SCOPE:
            raise ValueError(f"{scope} scope not understood")
        cfg.scope = _native.SCOPE[scope]
        if memory_mode not in _native.MEM:
            raise ValueError("memory_mode must be one of 'high', 'medium', 'low', 'biwfa'")
        cfg.memory_mode = _native.MEM[memory_mode]
        cfg.pattern_begin_free, cfg.pattern_end_free = int(pattern_begin_free), int(pattern_end_free)
        cfg.text_begin_free, cfg.text_end_free = int(text_begin_free), int(text_end_free)
        if span not in _native.SPAN:
            raise NotImplementedError(f"{span} span not implemented")
        cfg.span = _native.SPAN[span]
        if heuristic not in _native.HEUR:
            raise NotImplementedError(f"{heuristic} heuristic not implemented")
        cfg.heuristic = _native.HEUR[heuristic]
        cfg.min_wavefront_length = int(min_wavefront_length)
        cfg.max_distance_threshold = int(max_distance_threshold)
        cfg.steps_between_cutoffs = int(steps_between_cutoffs)
        cfg.xdrop = int(xdrop)
        cfg.max_steps = int(max_steps) if int(max_steps) > 0 else 0
        cfg.wildcard = self._bwildcard
        self._cfg = cfg
        self._native = _native.Aligner(cfg, device)  # raises if no library / no GPU / bad config
        self._host_scratch = {}   # buffers of the compiled host's batch marshalling (pywfa_amd/host/_host.pyx), kept between calls
        # devices=[...] (additive): batches given to wavefront_align_batch / align_batch are sharded over these GPUs of the
        # node (contiguous shards balanced by bases, one host thread per device, no collective); single pairs and resident
        # batches stay on `device`
        self._multi = _native.MultiAligner(cfg, devices) if devices is not None and len(devices) > 1 else None
        # last single-pair result (the reference keeps it inside the C aligner object)
        self._status = -1
        self._score = -2147483648
        self._ops = _NO_OPS

    # ------------------------------------------------------------------ helpers
    def _set_pattern(self, pattern):
        self._pattern = pattern.upper()
        self._bpattern = self._pattern.encode("ascii")
        self.pattern_len = len(self._bpattern)

    def _push(self):
        # (the wildcard set through its setter goes with the push; _cfg records it only once the library took the configuration,
        # so that a refused setter leaves the pending wildcard pending)
        cfg = self._cfg.copy()
        cfg.wildcard = self._bwildcard
        self._native.set_config(cfg)
        if self._multi is not None:
            self._multi.set_config(cfg)
        self._cfg.wildcard = self._bwildcard

    def _sync_wildcard(self):
        """Push a wildcard set through the setter that the library does not have yet (every entry point calls this first)."""
        if self._cfg.wildcard != self._bwildcard:
            self._push()

    # ------------------------------------------------------------------ single pair
    def wavefront_align(self, text, pattern=None):
        """Align one pair; returns the score (align.pyx:421-443)."""
        if pattern is not None:
            self._set_pattern(pattern)
        t = text.upper().encode("ascii")
        self._text = text
        self.text_len = len(t)
        if self._bpattern is None:
            raise AttributeError("pattern has not been set")
        self._sync_wildcard()
        # one pair per call: wfa_hip_align_pair (no arrays on the way; about 14 us per 150 bp call at the C ABI, 19 us with the op
        # string — the reference takes 1-2 us on a host core: loops of single calls work and are exact, throughput needs
        # wavefront_align_batch)
        full = self._cfg.scope == 1
        score, status, ops = self._native.align_pair(self._bpattern, t, full)
        self._score = score
        self._status = status
        self._ops = np.frombuffer(ops, np.uint8) if ops else _NO_OPS
        self.alignment_score = self._score
        return self._score

    def __call__(self, text, pattern=None, clip_cigar=False, min_aligned_bases_left=1,
                 min_aligned_bases_right=1, elide_mismatches=False, supress_sequences=False):
        """Align ``text`` to ``pattern`` and return an AlignmentResult (align.pyx:835-879)."""
        if pattern is None:
            p = self._pattern
            if not p:
                raise ValueError("pattern is None")
            lp = len(self._pattern)
            score = self.wavefront_align(text)
        else:
            lp = len(pattern)
            p = pattern
            score = self.wavefront_align(text, pattern)
        ct = self.cigartuples
        locs = self.locations
        status = self.status
        if supress_sequences:
            res = AlignmentResult(lp, len(text), locs[0], locs[1], locs[2], locs[3], ct, score, "", "", status)
        else:
            res = AlignmentResult(lp, len(text), locs[0], locs[1], locs[2], locs[3], ct, score, p, text, status)
        # as committed in the reference the test is inverted: clip / elide only act when the scope is
        # NOT "full", i.e. on an empty CIGAR (align.pyx:874-878)
        if not self.scope == "full":
            if clip_cigar:
                res = clip_cigartuples(res, min_aligned_bases_left, min_aligned_bases_right)
            if elide_mismatches:
                res.cigartuples = elide_mismatches_from_cigar(res.cigartuples)
        return res

    # ------------------------------------------------------------------ batches (additive API)
    def wavefront_align_batch(self, texts, patterns=None, *, summary=False):
        """Align many pairs on the GPU. ``patterns`` None = the cached pattern for every text.

        Returns dict(score=int32[n], status=int32[n], cigarstrings=sequence of str, cigar_ops=sequence of uint8 arrays
        (scope full; built from the GPU's run-length encoding when an item is read)).  ``summary=True``: see ``align_batch``."""
        if summary:
            _need_full_for_summary(self._cfg)
        texts = texts if type(texts) is list else list(texts)
        if patterns is None:
            if self._bpattern is None:
                raise ValueError("pattern is None")
            patterns = self._bpattern  # stored once in the batch: every pair points to it
        else:
            patterns = patterns if type(patterns) is list else list(patterns)
        self._sync_wildcard()
        # the compiled host reads the objects' buffers in place and upper-cases on OpenMP threads (pywfa_amd/host/_host.pyx); objects
        # it does not take (non-ASCII text, other types) and builds without the extension go through datagen.from_strings, which
        # raises what the reference raises (align.pyx:432,435)
        host = _native.compiled_host()
        # (its blob and offset arrays are kept between calls: align_batch below returns only after the upload, and keeps nothing of the batch)
        batch = host.from_strings(patterns, texts, self._host_scratch) if host is not None else None
        if batch is None:
            batch = datagen.from_strings(patterns, texts, upper=True)
        return self.align_batch(batch, summary=True) if summary else self.align_batch(batch)

    def align_batch(self, batch, *, summary=False):
        """Align a prepared batch dict (see ``pywfa_amd.datagen``): ASCII blob + offsets + lengths.

        ``summary=True`` (scope full only, else ValueError): no op string leaves the GPU; returns dict(score=, status=, summary=),
        ``summary`` a dict of int32 arrays ``M``, ``X``, ``I``, ``D`` (ops of each kind per pair), ``I_runs``, ``D_runs`` (maximal
        runs) and ``locations`` of shape (n, 4) (pattern_start, pattern_end, text_start, text_end), reduced on the device
        (csrc/wfa_summary.hpp).  Always one resident batch on this aligner's device."""
        if summary:
            _need_full_for_summary(self._cfg)
            self._sync_wildcard()
            rb = self._native.batch(batch)
            try:
                rb.run()
                rb.sync()
                score, status, _ = rb.results(False)
                rows = rb.summary()
            finally:
                rb.close()
            return {"score": score, "status": status, "summary": _summary_dict(rows)}
        self._sync_wildcard()
        full = self._cfg.scope == 1
        if full and self._multi is None and len(batch["p_len"]) <= 1024:
            # a small batch: the single-call form of the library (one launch, results polled in a pinned block); the CIGAR
            # strings are run-length encoded when they are read
            score, status, (ops, cbeg, clen) = self._native.align_batch(batch, True)
            return {"score": score, "status": status, "cigar_ops": _OpsSequence(ops, cbeg, clen, "ops"),
                    "cigarstrings": _OpsSequence(ops, cbeg, clen, "str")}
        if full and self._multi is None:
            # one device: the op strings stay on the GPU, their run-length encoding comes back (csrc/wfa_rle.hpp); the Python
            # strings / op arrays are built when they are read
            rb = self._native.batch(batch)
            try:
                rb.run()
                rb.sync()
                score, status, _ = rb.results(False)
                off, code, rlen, _locs = rb.rle()
            finally:
                rb.close()
            return {"score": score, "status": status, "cigar_ops": _RunSequence(off, code, rlen, "ops"),
                    "cigarstrings": _RunSequence(off, code, rlen, "str")}
        score, status, cig = (self._multi or self._native).align_batch(batch, full)
        out = {"score": score, "status": status}
        if full:
            ops, cbeg, clen = cig
            out["cigar_ops"] = [ops[cbeg[i]:cbeg[i] + clen[i]] for i in range(len(score))]
            out["cigarstrings"] = [_ops_to_string(o) for o in out["cigar_ops"]]
        return out

    def align_batch_results(self, batch, patterns_texts=None):
        """Align a batch (scope must be "full") and return a ``BatchResults``: scores, statuses, and the
        cigartuples / locations of every pair computed on the GPU (what ``__call__`` derives per pair)."""
        if self._cfg.scope != 1:
            raise ValueError("align_batch_results needs scope='full'")
        self._sync_wildcard()
        rb = self._native.batch(batch)
        try:
            rb.run()
            rb.sync()
            score, status, _ = rb.results(False)
            off, code, rlen, locs = rb.rle()
        finally:
            rb.close()
        return BatchResults(batch, score, status, off, code, rlen, locs)

    def resident_batch(self, batch):
        """Upload + 2-bit pack a batch into HBM once; ``.run()`` it many times (bench.py).  The batch keeps the configuration
        (wildcard included) that is in force when it is created."""
        self._sync_wildcard()
        return self._native.batch(batch)

    # ------------------------------------------------------------------ score matrices (additive API)
    def _seqset(self, seqs):
        """Upload one set of sequences (upper-cased and checked like ``wavefront_align_batch``), packed once on the device."""
        seqs = seqs if type(seqs) is list else list(seqs)
        host = _native.compiled_host()
        # (the compiled host's batch blob with an empty shared pattern: the texts are the set; a fresh scratch dict, the set's upload
        # is over when seqset() returns)
        batch = host.from_strings(b"", seqs, {}) if host is not None else None
        if batch is None:
            batch = datagen.from_strings(b"", seqs, upper=True)
        return self._native.seqset(batch["seqs"], batch["t_off"], batch["t_len"])

    def sequence_set(self, seqs):
        """Upload a list of sequences once and keep them on the GPU: a ``SequenceSet`` (``len()``, ``close()``, context manager) that
        ``score_matrix``, ``completed_pairs``, ``nearest`` and ``align_pairs`` accept wherever they accept a list of ``str``.  The set
        is packed under the wildcard in force now; after ``wildcard`` changes, make a new one."""
        self._sync_wildcard()
        return SequenceSet(self, self._seqset(seqs))

    def _read_lengths(self, patterns):
        """The lengths of ``patterns`` (a list of ``str`` or a ``SequenceSet`` of this aligner, open)."""
        if isinstance(patterns, SequenceSet):
            if patterns._aligner is not self:
                raise ValueError("sequence set of another aligner")
            if patterns._set is None or not patterns._set._h:
                raise ValueError("sequence set is closed")
            return patterns._set.length
        return np.fromiter((len(s) for s in patterns), np.int32, len(patterns))

    def quality_set(self, patterns, quals, offset=33):
        """Upload the base qualities of the reads ``patterns`` (a ``SequenceSet`` or a list of ``str``) once and keep them on the
        GPU: a ``QualitySet`` (``len()``, ``close()``, context manager) for ``pileup(..., qualities=)``.  ``quals``: one entry per
        read, a ``str`` or ``bytes`` of phred + ``offset`` as in FASTQ, or a uint8 array of raw phred (``offset`` ignored); one
        value per base, phred 0 .. 93.  ValueError, before anything is uploaded, names the first offending entry."""
        if not isinstance(patterns, (SequenceSet, list)):
            patterns = list(patterns)
        blob, off, length = _quality_blob(quals, self._read_lengths(patterns), offset)
        sets, mine = self._open_sets(patterns, None)
        try:
            return QualitySet(self, self._native.qualset(sets[0], blob, off, length))
        finally:
            for s in mine:
                s.close()

    def seed_index(self, texts, k=13, stride=1, max_occ=64, w=None):
        """Index the k-mers of ``texts`` (a list of ``str`` or a ``SequenceSet``) on the GPU: a ``SeedIndex`` (``seeds()``,
        ``stats()``, ``close()``, context manager), the seed source of ``align_windows`` / ``pileup`` for reads without an index of
        your own.  Every position ``t`` with ``t % stride == 0`` whose ``k`` letters are all of ACGT is indexed; a k-mer that occurs
        more than ``max_occ`` times in the texts yields no hits (the repeat mask).  ``k``: 8 .. 15; the table takes 4^k * 4 bytes of
        HBM (k = 13: 256 MiB, k = 15: 4 GiB) plus 8 bytes per indexed position.  With ``devices=[...]`` the first device holds it.
        ``w`` (1 .. 32; not together with a ``stride`` other than 1): a minimizer index instead.  The texts and the reads are sampled
        by one rule, the (w,k)-minimizers under a hash of the canonical k-mer (include/wfa_hip.h, "minimizers"): about 2 / (w + 1) of
        the positions are indexed, a read looks up only its own minimizers, and an exact match of w + k - 1 bases always shares one.
        ``SeedIndex.k`` / ``.w`` / ``.stride`` tell which index it is."""
        k = _seed_param("k", k, 8, 15)
        stride = _seed_param("stride", stride, 1)
        max_occ = _seed_param("max_occ", max_occ, 1)
        if w is not None:
            w = _seed_param("w", w, 1, _native.MINIMIZER_MAX_W)
            if stride != 1:
                raise ValueError(f"w = {w} goes with stride = 1 only (a minimizer index has no stride), got stride = {stride}")
        for name, v in (("stride", stride), ("max_occ", max_occ)):
            if v >= 2**31:
                raise ValueError(f"{name} = {v} does not fit 32 bits")
        if not isinstance(texts, (SequenceSet, list)):
            texts = list(texts)
        if len(texts) == 0:
            raise ValueError("texts = a set of 0 sequences is out of range (at least 1)")
        self._sync_wildcard()
        sets, mine = self._open_sets(texts, None)
        try:
            return SeedIndex(self, self._native.seed_index(sets[0], k, stride, max_occ, w))
        finally:
            for s in mine:
                s.close()

    def _open_sets(self, patterns, texts):
        """The native sets of ``patterns`` / ``texts`` (None: one set) and those of them this call uploaded (its to close)."""
        sets, mine = [], []
        try:
            for x in ((patterns,) if texts is None else (patterns, texts)):
                if isinstance(x, SequenceSet):
                    if x._aligner is not self:
                        raise ValueError("sequence set of another aligner")
                    if x._set is None or not x._set._h:
                        raise ValueError("sequence set is closed")
                    sets.append(x._set)
                else:
                    sets.append(self._seqset(x))
                    mine.append(sets[-1])
        except BaseException:
            for s in mine:
                s.close()
            raise
        return sets, mine

    def _cross(self, patterns, texts, want, k=None):
        self._sync_wildcard()
        sets, mine = self._open_sets(patterns, texts)
        try:
            run = self._native.cross(sets[0], sets[1] if texts is not None else None, want, k)
            try:
                if want == _native.CROSS_TOPK:
                    return run.topk()
                return run.dense() if want == _native.CROSS_DENSE else run.completed()
            finally:
                run.close()
        finally:
            for s in mine:
                s.close()

    # ------------------------------------------------------------------ index pairs over resident sets (additive API)
    @staticmethod
    def _check_pair_indices(i, j, m, n):
        """The index arrays of ``align_pairs`` as int32, or ValueError: before anything is uploaded."""
        out = []
        for name, a, size in (("i", i, m), ("j", j, n)):
            if a is None:
                raise ValueError(f"align_pairs needs the index arrays i= and j= ({name} is missing)")
            a = np.asarray(a)
            if a.ndim != 1:
                raise ValueError(f"{name} must be a one-dimensional array of indices")
            if a.size == 0:
                a = a.astype(np.int32)
            if a.dtype.kind not in "iu":
                raise ValueError(f"{name} must hold integers, got dtype {a.dtype}")
            if a.size:
                if int(a.min()) < 0:
                    raise ValueError(f"{name}[{int(np.flatnonzero(a < 0)[0])}] is negative: filter such rows out first "
                                     "(nearest() pads its rows with j = -1)")
                if int(a.max()) >= size:
                    q = int(np.flatnonzero(a >= size)[0])
                    raise ValueError(f"{name}[{q}] = {int(a[q])} is out of range for a set of {size} sequences")
            out.append(np.ascontiguousarray(a, dtype=np.int32))
        if out[0].shape[0] != out[1].shape[0]:
            raise ValueError(f"i and j differ in length: {out[0].shape[0]} and {out[1].shape[0]}")
        return out

    def align_pairs(self, patterns, texts=None, *, i=None, j=None, summary=False, left_align=False, sam=False, eqx=False,
                    clip_mismatches=False):
        """Align the listed pairs (patterns[i[q]], texts[j[q]]) on the GPU, each sequence uploaded once however many pairs name it;
        ``texts=None``: both indices into ``patterns``.  ``patterns`` / ``texts``: lists of ``str`` (uploaded and released inside
        the call) or ``SequenceSet`` handles of ``sequence_set`` (left open).  ``i`` / ``j``: integer arrays of equal length, every
        value inside its set (ValueError before anything is uploaded otherwise: rows of ``nearest`` padded with ``j = -1`` must be
        filtered out first).  Duplicates, ``i == j`` and empty sequences are fine.

        Returns what ``wavefront_align_batch`` returns for those pairs under this aligner's configuration, in list order:
        dict(score=, status=) and, with scope full, cigarstrings= / cigar_ops=.  With ``devices=[...]`` the first device runs it.
        ``summary=True`` (scope full only): dict(score=, status=, summary=) as ``align_batch`` describes, no op strings.
        ``left_align=True`` (scope full only, else ValueError): the op strings are left-aligned on the GPU before anything is read
        (``left_align_ops`` states the rule); ``cigarstrings``, ``cigar_ops`` and ``summary`` are then those of the rewritten
        strings, the scores stay WFA's.
        ``sam=True`` (scope full only): the SAM fields of every pair are made on the GPU (after the left alignment, when both are
        asked for) and no op string is returned: dict(score=, status=, sam=dict(pos=, ref_len=, clip_left=, clip_right=, nm=,
        query_len=, cigar=, md=)), with ``summary=True`` also summary=.  The six numbers are int32 arrays, ``cigar`` and ``md`` lazy
        sequences of ``str``.  The CIGAR is SAM's: the library's ``D`` (the read inserts) reads ``I`` and its ``I`` reads ``D``;
        free ends and, with ``clip_mismatches=True``, the mismatches outside the aligned core are soft clips; ``eqx=True`` writes
        ``=`` and ``X`` for ``M``.  ``pos`` is 0-based in the text of the pair, -1 for a pair without an alignment (its strings are
        empty).  ``eqx`` or ``clip_mismatches`` without ``sam=True``: ValueError.  (include/wfa_hip.h, "SAM fields", has the rule.)"""
        if summary:
            _need_full_for_summary(self._cfg)
        if left_align:
            _need_full_for_summary(self._cfg, "left_align=True")
        sam_flags = _sam_flags(self._cfg, sam, eqx, clip_mismatches) if sam or eqx or clip_mismatches else None
        if not isinstance(patterns, (SequenceSet, list)):
            patterns = list(patterns)
        if texts is not None and not isinstance(texts, (SequenceSet, list)):
            texts = list(texts)
        m = len(patterns)
        n = m if texts is None else len(texts)
        i, j = self._check_pair_indices(i, j, m, n)
        self._sync_wildcard()
        full = self._cfg.scope == 1
        npairs = i.shape[0]
        sets, mine = self._open_sets(patterns, texts)
        try:
            pset, tset = sets[0], sets[-1]
            # lists too long for one batch run in consecutive chunks: a pair budget (WFA_HIP_PAIRS_BAND pairs, as WFA_HIP_CROSS_BAND caps
            # a band of a cross run) and the library's bound on the words of one batch (2^32; half of it here)
            budget = max(1, int(os.environ.get("WFA_HIP_PAIRS_BAND", "0") or 0) or (1 << 24))
            longest = ((int(pset.length.max()) + 15) >> 4) + ((int(tset.length.max()) + 15) >> 4) if npairs else 0
            cuts = [0]
            if npairs <= budget and npairs * longest < (1 << 31):
                cuts.append(npairs)   # (one batch whatever the pairs: no need to sum their words)
            words = None
            while cuts[-1] < npairs:
                if words is None:
                    words = np.cumsum(((pset.length[i].astype(np.int64) + 15) >> 4) + ((tset.length[j].astype(np.int64) + 15) >> 4))
                lo = cuts[-1]
                before = int(words[lo - 1]) if lo else 0
                hi = min(lo + budget, int(np.searchsorted(words, before + (1 << 31), side="right")))
                cuts.append(max(hi, lo + 1))
            return self._run_lists(npairs, cuts, lambda lo, hi: self._native.batch_indexed(
                pset, tset if texts is not None else None, i[lo:hi], j[lo:hi]), summary=summary, left_align=bool(left_align), sam=sam_flags)
        finally:
            for s in mine:
                s.close()

    def _run_lists(self, npairs, cuts, make, summary=False, each=None, left_align=False, sam=None):
        """Run the resident batches ``make(lo, hi)`` of the consecutive chunks ``cuts`` of a pair list and join their results.
        ``summary``: the per-pair summary rows instead of op strings.  ``each(rb, lo, hi, score, status)``: called on every chunk's
        batch after its run instead of fetching op strings (``pileup``).  ``left_align``: every chunk's op strings are left-aligned
        on the GPU after its run, before anything is read from the batch.  ``sam``: the flags of ``sam=True`` — the SAM fields of
        every chunk instead of op strings (beside the summary rows, when both are asked for) — or None."""
        full = self._cfg.scope == 1
        score = np.zeros(npairs, np.int32)
        status = np.zeros(npairs, np.int32)
        strings = not summary and each is None and sam is None   # op strings are wanted: as they are for a small list, run-length encoded otherwise
        small = strings and full and npairs <= 1024 and len(cuts) <= 2
        rows = np.zeros((npairs, _native.SUMMARY_COLS), np.int32) if summary else None
        ops_res, runs, sams = None, [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            rb = make(lo, hi)
            try:
                rb.run()
                rb.sync()
                if left_align:
                    rb.left_align()
                sc, st, cig = rb.results(small)
                score[lo:hi] = sc
                status[lo:hi] = st
                if summary:
                    rows[lo:hi] = rb.summary()
                if sam is not None:
                    sams.append(rb.sam(sam))
                if each is not None:
                    each(rb, lo, hi, sc, st)
                elif small:
                    ops_res = cig
                elif strings and full:
                    runs.append(rb.rle()[:3])
            finally:
                rb.close()
        out = {"score": score, "status": status}
        if summary:
            out["summary"] = _summary_dict(rows)
        if sam is not None:
            parts = list(zip(*sams)) if sams else [[np.zeros((0, _native.SAM_COLS), np.int32)], [np.zeros(0, np.uint8)], [np.zeros(0, np.uint8)]]
            out["sam"] = _sam_dict(*(np.concatenate(p) for p in parts))
        if not strings:
            return out
        if small or (full and npairs == 0):
            ops, cbeg, clen = ops_res if ops_res is not None else (np.zeros(1, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int32))
            out["cigar_ops"] = _OpsSequence(ops, cbeg, clen, "ops")
            out["cigarstrings"] = _OpsSequence(ops, cbeg, clen, "str")
        elif full:
            # the op strings stayed on the GPU, their run-length encoding came back (as align_batch); chunks joined end to end
            off = np.zeros(npairs + 1, np.int64)
            base = 0
            for (o, _c, _l), lo, hi in zip(runs, cuts[:-1], cuts[1:]):
                off[lo + 1:hi + 1] = o[1:] + base
                base += int(o[-1])
            code = np.concatenate([r[1] for r in runs])
            rlen = np.concatenate([r[2] for r in runs])
            out["cigar_ops"] = _RunSequence(off, code, rlen, "ops")
            out["cigarstrings"] = _RunSequence(off, code, rlen, "str")
        return out

    # ------------------------------------------------------------------ windows of resident sequences (additive API)
    @staticmethod
    def _window_array(name, a, npairs, boolean=False):
        """One optional per-pair array of ``align_windows``, checked, or ValueError naming the array and the position."""
        if a is None:
            return None
        a = np.asarray(a)
        if a.ndim != 1:
            raise ValueError(f"{name} must be a one-dimensional array")
        if a.size == 0:
            a = a.astype(np.uint8 if boolean else np.int32)
        if a.dtype.kind not in ("biu" if boolean else "iu"):
            raise ValueError(f"{name} must hold {'booleans or 0 / 1' if boolean else 'integers'}, got dtype {a.dtype}")
        if a.shape[0] != npairs:
            raise ValueError(f"{name} and i differ in length: {a.shape[0]} and {npairs}")
        if boolean:
            if a.dtype.kind != "b" and a.size and ((a != 0) & (a != 1)).any():
                q = int(np.flatnonzero((a != 0) & (a != 1))[0])
                raise ValueError(f"{name}[{q}] = {int(a[q])} is neither 0 nor 1")
            return np.ascontiguousarray(a != 0, dtype=np.uint8)
        if a.size and int(a.min()) < 0:
            q = int(np.flatnonzero(a < 0)[0])
            raise ValueError(f"{name}[{q}] = {int(a[q])} is negative")
        if a.size and int(a.max()) >= 2**31:
            q = int(np.flatnonzero(a >= 2**31)[0])
            raise ValueError(f"{name}[{q}] = {int(a[q])} does not fit 32 bits")
        return np.ascontiguousarray(a, dtype=np.int32)

    def _window_lists(self, patterns, texts, i, j, pattern_start, pattern_len, text_start, text_len, reverse):
        """The arguments of ``align_windows`` / ``pileup`` checked (ValueError before anything is uploaded): the sequences (lists or
        handles), the int32 index arrays, the optional window arrays, and the windows' lengths (int64) of patterns and texts."""
        if not isinstance(patterns, (SequenceSet, list)):
            patterns = list(patterns)
        if texts is not None and not isinstance(texts, (SequenceSet, list)):
            texts = list(texts)
        m = len(patterns)
        n = m if texts is None else len(texts)
        i, j = self._check_pair_indices(i, j, m, n)
        npairs = i.shape[0]
        ps = self._window_array("pattern_start", pattern_start, npairs)
        pl = self._window_array("pattern_len", pattern_len, npairs)
        ts = self._window_array("text_start", text_start, npairs)
        tl = self._window_array("text_len", text_len, npairs)
        rev = self._window_array("reverse", reverse, npairs, boolean=True)

        def lengths(x):
            if isinstance(x, SequenceSet):
                if x._aligner is not self:
                    raise ValueError("sequence set of another aligner")
                if x._set is None or not x._set._h:
                    raise ValueError("sequence set is closed")
                return x._set.length
            return np.fromiter((len(s) for s in x), np.int32, len(x))

        plen_seq = lengths(patterns)
        tlen_seq = plen_seq if texts is None else lengths(texts)
        wlen = []
        for what, seq_len, idx, start, length in (("pattern", plen_seq, i, ps, pl), ("text", tlen_seq, j, ts, tl)):
            have = seq_len[idx].astype(np.int64) if npairs else np.zeros(0, np.int64)
            s0 = start.astype(np.int64) if start is not None else 0
            ln = length.astype(np.int64) if length is not None else have - s0
            over = np.flatnonzero((s0 + ln > have) | (ln < 0))
            if len(over):
                q = int(over[0])
                raise ValueError(f"{what}_start[{q}] + {what}_len[{q}] = {int(s0[q]) if start is not None else 0} + "
                                 f"{int(ln[q]) if length is not None else 'the rest'} runs past the end of {what} sequence "
                                 f"{int(idx[q])} ({int(have[q])} bases)")
            wlen.append(ln)
        return patterns, texts, (i, j, ps, pl, ts, tl, rev), wlen

    def _run_windows(self, pset, tset, arrays, wlen, **how):
        """The windowed batches of a checked list over two native sets (``tset`` None: one set), in chunks as ``align_pairs`` cuts
        them, by the words of the WINDOWS; ``how`` goes to ``_run_lists``."""
        i, j, ps, pl, ts, tl, rev = arrays
        npairs = i.shape[0]
        budget = max(1, int(os.environ.get("WFA_HIP_PAIRS_BAND", "0") or 0) or (1 << 24))
        words = np.cumsum(((wlen[0] + 15) >> 4) + ((wlen[1] + 15) >> 4)) if npairs else np.zeros(0, np.int64)
        cuts = [0]
        while cuts[-1] < npairs:
            lo = cuts[-1]
            before = int(words[lo - 1]) if lo else 0
            hi = min(lo + budget, int(np.searchsorted(words, before + (1 << 31), side="right")))
            cuts.append(max(hi, lo + 1))

        def cut(a, lo, hi):
            return None if a is None else a[lo:hi]

        return self._run_lists(npairs, cuts, lambda lo, hi: self._native.batch_windows(
            pset, tset, i[lo:hi], j[lo:hi], cut(ps, lo, hi), cut(pl, lo, hi),
            cut(ts, lo, hi), cut(tl, lo, hi), cut(rev, lo, hi)), **how)

    def _windows(self, *window_args):
        """The session of one call over a window list: ``_Windows`` of (patterns, texts, i, j, pattern_start, pattern_len, text_start,
        text_len, reverse)."""
        return _Windows(self, *window_args)

    def _placement(self, min_score, full_gap, **pair_only):
        """``(min_score, full_gap)`` of ``place_windows`` / ``place_pairs`` as the ints the library takes, defaults filled in, after
        the check that they (and the integers only ``place_pairs`` has) are integers at all."""
        for name, v in dict(min_score=min_score, full_gap=full_gap, **pair_only).items():
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
                raise ValueError(f"{name} must be an integer{'' if name.endswith('insert') else ' or None'}, got {v!r}")
        if min_score is not None and not -2**31 <= int(min_score) < 2**31:
            raise ValueError(f"min_score = {min_score} does not fit 32 bits")
        if full_gap is None:
            full_gap = 6 * int(self._cfg.mismatch) if self._cfg.distance >= 2 else 6
        if not 1 <= int(full_gap) < 2**31:
            raise ValueError(f"full_gap = {full_gap} is out of range (at least 1)")
        return _native.INT32_MIN if min_score is None else int(min_score), int(full_gap)

    @staticmethod
    def _hits_into(placer, arrays):
        """The ``each`` of ``_run_lists`` that adds every chunk's pairs to ``placer`` as hits of the listed windows."""
        ii, jj, ts, rev = arrays[0], arrays[1], arrays[4], arrays[6]

        def add(rb, lo, hi, score, status):
            placer.add(rb, ii[lo:hi], jj[lo:hi], None if ts is None else ts[lo:hi], None if rev is None else rev[lo:hi])

        return add

    def align_windows(self, patterns, texts=None, *, i=None, j=None, pattern_start=None, pattern_len=None,
                      text_start=None, text_len=None, reverse=None, summary=False, left_align=False, sam=False, eqx=False,
                      clip_mismatches=False):
        """Align windows of resident sequences on the GPU: pair q is bases [pattern_start[q], + pattern_len[q]) of patterns[i[q]],
        reverse-complemented where ``reverse[q]``, against bases [text_start[q], + text_len[q]) of texts[j[q]] (never reversed);
        ``texts=None``: both indices into ``patterns``.  A start left out is 0 for every pair, a length left out runs to the end of
        the sequence, ``reverse`` left out means forward.  The complement is A<->T, C<->G (either case), any other letter stays.
        ``patterns`` / ``texts``: lists of ``str`` or ``SequenceSet`` handles, as for ``align_pairs``; the windows are cut, reversed
        and complemented on the device, only the index and window arrays are uploaded.

        Returns what ``wavefront_align_batch`` returns for the materialised strings under this aligner's configuration, in list
        order, as ``align_pairs`` does: dict(score=, status=) and, with scope full, cigarstrings= / cigar_ops= (coordinates relative
        to the windows: add the starts).  ValueError, before anything is uploaded, for arrays that are not one-dimensional integer
        arrays of one length, negative values, a window that ends behind its sequence, or a ``reverse`` that is not boolean / 0-1.
        ``summary=True`` (scope full only): dict(score=, status=, summary=) as ``align_batch`` describes, no op strings.
        ``left_align=True`` (scope full only): as for ``align_pairs``; the letters are the windows', a reversed pattern on the
        text's strand, and no gap moves left of its window.
        ``sam=True``, ``eqx``, ``clip_mismatches`` (scope full only): as for ``align_pairs``; ``pos`` is in the coordinates of the
        text SEQUENCE (the window's start is added; -1 stays -1), the read is the window on the text's strand, and the MD letters are
        the window's."""
        if summary:
            _need_full_for_summary(self._cfg)
        if left_align:
            _need_full_for_summary(self._cfg, "left_align=True")
        sam_flags = _sam_flags(self._cfg, sam, eqx, clip_mismatches) if sam or eqx or clip_mismatches else None
        with self._windows(patterns, texts, i, j, pattern_start, pattern_len, text_start, text_len, reverse) as w:
            out = w.run(summary=summary, left_align=bool(left_align), sam=sam_flags)
            if sam_flags is not None and w.arrays[4] is not None:
                pos = out["sam"]["pos"]
                out["sam"]["pos"] = np.where(pos >= 0, pos + w.arrays[4], pos).astype(np.int32)
            return out

    def pileup(self, patterns, texts=None, *, i=None, j=None, pattern_start=None, pattern_len=None, text_start=None,
               text_len=None, reverse=None, min_score=None, insertions=False, left_align=False, strands=False, qualities=None,
               min_base_quality=0, quality_cap=40, deletions=False):
        """Align the listed windows as ``align_windows`` does (same arguments, same checks; scope must be "full") and pile the
        alignments up over the TEXT sequences on the GPU: the patterns are reads, the texts references.  Every pair whose status is
        0 (and whose score is at least ``min_score``, when given) adds the ops of its aligned core — first M to last M — to the
        text bases they cover; neither op strings nor their run-length encoding leave the device (csrc/wfa_pileup.hpp).
        ``texts=None`` piles up over ``patterns``.  ``insertions=True``: the pileup also keeps what the reads insert (a log on the
        GPU, about 24 bytes per insertion and 1 byte per inserted base, and a second pass over the op strings), for
        ``Pileup.insertions`` and ``Pileup.consensus(insertions=True)``.  ``deletions=True``: the pileup also keeps every deletion
        as one event with its start and length (a log on the GPU, 16 bytes per deletion and 4 bytes per text base, and one more pass
        over the op strings), for ``Pileup.deletions`` and ``Pileup.deletion_starts``; it combines freely with the other options.
        ``left_align=True``: every op string is left-aligned on
        the GPU before it is piled up (``left_align_ops`` states the rule), so a gap inside a homopolymer or tandem repeat is
        counted at the left end of the repeat, where VCF puts it, and reads that stopped at different places of one repeat agree
        as far as their own letters allow; tables, ``sites``, ``insertions``, ``deletions`` and ``consensus(insertions=True)`` follow.
        ``strands=True``: the pileup also counts the forward reads (``reverse[q]`` == 0; every read when ``reverse`` is None) in a
        second table of 32 more bytes per text base, for ``counts(strand=...)`` and the strand columns and filter of
        ``Pileup.genotypes``; without it nothing more is allocated or launched.
        ``qualities``: the reads' base qualities, a ``QualitySet`` made for ``patterns`` or what ``quality_set`` takes (a list of
        FASTQ-style ``str`` / ``bytes`` at offset 33, or of uint8 arrays of raw phred).  A read base whose quality is under
        ``min_base_quality`` (0 .. 93) is not counted at all, neither under its letter nor as a mismatch; deletions and insertions
        count whatever the qualities.  A third table of 32 more bytes per text base sums min(quality, ``quality_cap``) (1 .. 93)
        of what is counted, for ``Pileup.quality_sums`` and ``Pileup.genotypes(qualities=True)``.  It combines freely with
        ``insertions``, ``strands``, ``left_align`` and ``min_score``; ``min_base_quality`` / ``quality_cap`` without
        ``qualities`` are a ValueError.

        Returns a ``Pileup`` (``score``, ``status``, ``counts(j)``, ``depth(j)``, ``calls()``, ``consensus()``, ``sites()``,
        ``genotypes()``, ``insertions()``, ``deletions()``, ``quality_sums(j)``, ``close()``; a context manager), which stays
        valid after the sets are closed.  With ``devices=[...]`` the first device runs it."""
        if self._cfg.scope != 1:
            raise ValueError("pileup needs scope='full'")
        if min_score is not None and (isinstance(min_score, bool) or not isinstance(min_score, (int, np.integer))):
            raise ValueError(f"min_score must be an integer or None, got {min_score!r}")
        if qualities is None:
            if min_base_quality != 0 or quality_cap != 40:
                raise ValueError("min_base_quality and quality_cap go with qualities=: this pileup was asked for without base qualities")
        else:
            min_base_quality = _quality_param("min_base_quality", min_base_quality, 0)
            quality_cap = _quality_param("quality_cap", quality_cap, 1)
        w = self._windows(patterns, texts, i, j, pattern_start, pattern_len, text_start, text_len, reverse)
        qblob = None
        if isinstance(qualities, QualitySet):
            if qualities._aligner is not self:
                raise ValueError("quality set of another aligner")
            if qualities._set is None or not qualities._set._h:
                raise ValueError("quality set is closed")
            have = self._read_lengths(w._patterns)
            if qualities._set.n != len(have) or not np.array_equal(qualities._set.length, have):
                raise ValueError(f"the quality set was made for other reads: {qualities._set.n} entries for {len(have)} patterns, or "
                                 "lengths that differ")
        elif qualities is not None:
            qblob = _quality_blob(qualities, self._read_lengths(w._patterns), 33)
        with w:
            ii, jj, ps, ts = w.arrays[0], w.arrays[1], w.arrays[2], w.arrays[4]
            table = w.attach(self._native.pileup(w.text_set), keep=True)
            rev = w.arrays[6]
            if insertions:
                table.track_insertions(True)
            if deletions:
                table.track_deletions(True)
            if strands:
                table.track_strands(True)
            qset = None
            if qualities is not None:
                table.track_qualities(True)
                if qblob is None:
                    qset = qualities._set
                else:
                    qset = self._native.qualset(w.pset, *qblob)
                    w._mine.append(qset)   # (this call's upload: closed with the sets when the body is left)

            def cut(a, lo, hi):
                return None if a is None else a[lo:hi]

            def add(rb, lo, hi, score, status):
                keep = None if min_score is None else (score >= int(min_score))
                if qset is not None:
                    table.add_quals(rb, jj[lo:hi], qset, ii[lo:hi], cut(ts, lo, hi), keep, cut(rev, lo, hi), cut(ps, lo, hi),
                                    min_base_quality, quality_cap)
                elif strands:
                    table.add(rb, jj[lo:hi], None if ts is None else ts[lo:hi], keep, None if rev is None else rev[lo:hi])
                else:
                    table.add(rb, jj[lo:hi], None if ts is None else ts[lo:hi], keep)

            out = w.run(each=add, left_align=bool(left_align))
            return Pileup(table, out["score"], out["status"], self)

    def _dup_options(self, duplicates, dup_ends, dup_qualities, dup_min_quality):
        """The duplicate options of ``place_windows`` / ``place_pairs``, checked before anything is uploaded: (unclipped,
        min_quality)."""
        if not isinstance(duplicates, (bool, np.bool_)):
            raise ValueError(f"duplicates must be True or False, got {duplicates!r}")
        if dup_ends not in ("core", "unclipped"):
            raise ValueError(f"dup_ends must be 'core' or 'unclipped', got {dup_ends!r}")
        if not duplicates:
            for name, given in (("dup_ends", dup_ends != "core"), ("dup_qualities", dup_qualities is not None),
                                ("dup_min_quality", isinstance(dup_min_quality, (bool, np.bool_)) or dup_min_quality != 15)):
                if given:
                    raise ValueError(f"{name} goes with duplicates=True")
            return False, 15
        if dup_ends == "unclipped" and self._cfg.scope != 1:
            raise ValueError("dup_ends='unclipped' needs scope='full': under scope score a hit's interval is its whole window and has no clips")
        if dup_qualities is None:
            if isinstance(dup_min_quality, (bool, np.bool_)) or dup_min_quality != 15:
                raise ValueError("dup_min_quality goes with dup_qualities=: the representative was asked for by alignment score")
            return dup_ends == "unclipped", 15
        return dup_ends == "unclipped", _quality_param("dup_min_quality", dup_min_quality, 0)

    def _dup_quality_blob(self, w, dup_qualities):
        """``dup_qualities`` against the reads of the window list ``w``, before anything is uploaded: None for a ``QualitySet`` (or no
        qualities), else the blob of ``_quality_blob``."""
        if dup_qualities is None:
            return None
        if isinstance(dup_qualities, QualitySet):
            if dup_qualities._aligner is not self:
                raise ValueError("quality set of another aligner")
            if dup_qualities._set is None or not dup_qualities._set._h:
                raise ValueError("quality set is closed")
            have = self._read_lengths(w._patterns)
            if dup_qualities._set.n != len(have) or not np.array_equal(dup_qualities._set.length, have):
                raise ValueError(f"the quality set was made for other reads: {dup_qualities._set.n} entries for {len(have)} patterns, or "
                                 "lengths that differ")
            return None
        return _quality_blob(dup_qualities, self._read_lengths(w._patterns), 33)

    def _mark_duplicates(self, w, placer, mates, how, unclipped, dup_qualities, qblob, min_quality):
        """``placer.duplicates`` inside the entered window list ``w``; a blob of this call is uploaded and closed with the sets."""
        qset = None
        if dup_qualities is not None:
            if qblob is None:
                qset = dup_qualities._set
            else:
                qset = self._native.qualset(w.pset, *qblob)
                w._mine.append(qset)
        return placer.duplicates(w.text_set, mates, *how, unclipped=unclipped, qualities=qset, min_quality=min_quality)

    def place_windows(self, patterns, texts=None, *, i=None, j=None, pattern_start=None, pattern_len=None, text_start=None,
                      text_len=None, reverse=None, min_score=None, full_gap=None, duplicates=False, dup_ends="core",
                      dup_qualities=None, dup_min_quality=15):
        """Align the listed windows as ``align_windows`` does (same arguments, same checks; either scope) and decide on the GPU where
        every PATTERN sequence goes: the patterns are reads, each window one candidate hit of read ``i[q]``.  The rule is that of
        include/wfa_hip.h ("placement"), integers only.  A hit is eligible when its status is 0 and its score at least ``min_score``
        (None: every hit of status 0); a read's primary is its eligible hit of greatest score, the first in list order on a tie; an
        eligible hit on the same text and strand whose text interval overlaps the primary's by at least half of the shorter of the
        two is the same locus found again; the runner-up is the best eligible hit elsewhere.  The interval is the aligned core
        (first M to last M) under scope full, the whole text window under scope score.  ``mapq`` is 60 without a runner-up, else
        min(60, 60 * (score - second) // full_gap): a documented confidence, not a calibrated probability.  ``full_gap=None``: six
        times the mismatch penalty (6 for edit / indel), a runner-up six mismatches behind.

        Returns dict(score=, status=, flag=, reads=): the first three per hit in list order, ``flag`` uint8 (0 not eligible, 1
        eligible at another locus, 2 at the primary's locus, 3 the primary); ``reads`` a dict of int32 arrays of length
        ``len(patterns)``: hit (the primary's list position, -1 for a read without an eligible hit), score, second (-2**31 without
        a runner-up), mapq, hits (eligible), ties (runner-ups that equal the primary's score), text_start, text_end (the primary's
        interval on its text).  Neither scores nor locations are grouped on the host: 32 bytes per read and a byte per hit come
        back (csrc/wfa_place.hpp).  With ``devices=[...]`` the first device runs it.

        ``duplicates=True``: DUPLICATE MARKING, single-end (include/wfa_hip.h, "duplicates"; ``place_pairs`` describes it).  Every
        read whose primary has a non-empty interval is a unit with the key (text, strand, 5' end); ``reads`` gains the int32 arrays
        ``dup``, ``dup_rep``, ``dup_size`` and ``dup_overflow``.  ``dup_ends``, ``dup_qualities`` and ``dup_min_quality`` are those of
        ``place_pairs``.  ``duplicates=False`` returns exactly the keys above and neither allocates nor launches anything more."""
        min_score, full_gap = self._placement(min_score, full_gap)
        unclipped, min_quality = self._dup_options(duplicates, dup_ends, dup_qualities, dup_min_quality)
        w = self._windows(patterns, texts, i, j, pattern_start, pattern_len, text_start, text_len, reverse)
        qblob = self._dup_quality_blob(w, dup_qualities)
        with w:
            placer = w.attach(self._native.placer(w.nreads))
            out = w.run(each=self._hits_into(placer, w.arrays))
            rows, out["flag"] = placer.run(min_score, full_gap)
            out["reads"] = _columns(rows, _native.PLACE_COLUMNS)
            if duplicates:
                read_rows, _ = self._mark_duplicates(w, placer, 0, (min_score, full_gap), unclipped, dup_qualities, qblob, min_quality)
                out["reads"].update(_dup_columns(read_rows))
            return out

    def place_pairs(self, patterns, texts=None, *, i=None, j=None, pattern_start=None, pattern_len=None, text_start=None,
                    text_len=None, reverse=None, mates=None, min_insert=0, max_insert=1000, unpaired=None, min_score=None,
                    full_gap=None, rescue=False, rescue_pad=16, rescue_mapq=0, duplicates=False, dup_ends="core", dup_qualities=None,
                    dup_min_quality=15):
        """``place_windows`` for paired-end reads (same arguments, same checks; either scope): the listed windows are aligned, every
        read is placed on its own, and then the hits of the two mates of every fragment are joined on the GPU.  The rule is that of
        include/wfa_hip.h ("pairing"), integers only.  ``mates``: an (F, 2) integer array of indices into ``patterns``, fragment f
        being the reads ``mates[f, 0]`` (mate 1) and ``mates[f, 1]`` (mate 2), no read in two fragments; None: interleaved, reads
        2 f and 2 f + 1, ``len(patterns)`` even.  A pairing of an eligible hit of each mate is proper when the two lie on one text
        and on opposite strands, the forward one starts and ends no later than the reverse one (they face each other, neither
        extends past the other) and ``min_insert <= insert <= max_insert``, ``insert`` running from the forward hit's start to the
        reverse hit's end.  A fragment is proper when its best proper pairing is at most ``unpaired`` score points behind the two
        single-end primaries taken together (None: ``full_gap``); its reads then go to that pairing, otherwise to their single-end
        primaries.  ``mapq`` of a proper fragment is 60 without a proper pairing at another place, else
        min(60, 60 * (score - second) // full_gap); a mate's own mapq is never below it.  A fragment with more than 65 536 pairings
        of eligible hits is not joined (``overflow``).  The interval of a hit is the aligned core under scope full and the WHOLE
        TEXT WINDOW under scope score: there ``insert`` and the order test are as coarse as the windows are, so windows that are
        much longer than the reads call for wider insert bounds.

        Returns what ``place_windows`` returns, plus ``pair_flag`` (uint8 per hit: the flag relative to the hit its read was
        given, 3 that hit, 2 at its locus, 1 eligible elsewhere, 0 not eligible; the single-end flag for a read in no proper
        fragment) and ``pairs``, a dict of int32 arrays of length F: hit1, hit2 (list positions, -1 without one), proper, score,
        second (-2**31 when not proper or without a runner-up), mapq, mapq1, mapq2, insert, pairings (proper pairings), ties,
        overflow.  48 bytes per fragment more come back than from ``place_windows``, and a byte per hit.

        ``rescue=True`` (scope full and span ends-free only): MATE RESCUE.  A fragment without any proper pairing — a mate whose true
        place was never listed, because its seeds were masked, too few or overflowed — gets, from every mate whose single-end primary
        has a mapq of at least ``rescue_mapq`` (0 .. 60), one more window for the OTHER mate: on the anchor's text, on the opposite
        strand, as wide as the orientation rule and ``min_insert`` .. ``max_insert`` allow plus ``rescue_pad`` bases on either side
        (include/wfa_hip.h, "rescue").  The window list is made on the GPU where the hits lie (32 bytes per window come back), the
        windows are aligned under this aligner's configuration with ``text_begin_free`` and ``text_end_free`` set to
        F = (max_insert - min_insert) + 2 * rescue_pad for these alignments only (both are restored afterwards, also when the run
        raises; windows clipped below F bases by an end of their text are not made), their hits are added behind the n0 listed
        ones, and all hits are paired once.  A fragment that has proper pairings but lost to its single-end primaries is not
        rescued, only the primary anchors, and a rescue window may find a place the other mate already has a hit at: the
        same-locus rule absorbs it.  The rescue windows are wide, so they run in the general kernels: they cost far more per pair
        than the listed windows.  ``score``, ``status``, ``flag`` and ``pair_flag`` then cover the n0 listed hits followed by the
        rescue hits; ``pairs`` gains ``rescued`` (int32: 1 iff the fragment is proper and one of its chosen hits is a rescue hit),
        and ``rescue`` is added: dict(i=, j=, text_start=, text_len=, reverse=, fragment=, anchor=) of int32 arrays, possibly
        empty, hit ``n0 + q`` being window ``q`` of it (``anchor``: the hit number of the anchor).  ``rescue=False`` returns exactly
        the keys above.

        ``duplicates=True``: DUPLICATE MARKING (include/wfa_hip.h, "duplicates"), on the GPU after the final pairing, so after a
        rescue too.  A proper fragment is a unit with the key (text, start of its forward hit, end of its reverse hit, which mate is
        the forward one); a read in no proper fragment whose primary has a non-empty interval is a unit with the key (text, strand,
        5' end: the start of a forward primary, the last base of a reverse one).  Units of one kind with equal keys are a group; its
        representative is the unit of greatest score (pair score or single-end score), the smallest fragment / read number on a
        tie, and every other member is a duplicate.  ``pairs`` and ``reads`` each gain four int32 arrays: ``dup_rep`` (the
        representative's fragment / read number; -1 for what is no unit), ``dup_size`` (units in the group, 0 for no unit),
        ``dup`` (1: a duplicate) and ``dup_overflow`` (1: more than 4 096 units start at that base, none of them was resolved).
        The mates of a proper fragment are no units of their own, but their ``dup`` and ``dup_overflow`` repeat the fragment's:
        ``reads["dup"] == 0`` alone selects the reads to pile up.  16 bytes per read and per fragment come back; the device keeps
        4 bytes per base of the TEXT SET (a direct-addressed plane: its cost grows with the references, not with the reads) and
        65 per read.  ``dup_ends="core"`` keys a unit on the ends of the aligned core, so a copy whose first base mismatches, or
        that starts with a small insertion, starts a base later and misses its group; ``dup_ends="unclipped"`` (scope full only)
        keys it on the UNCLIPPED ends instead — where the read's first and last base would land if the bases in front of the
        first and behind the last match were laid down without gaps (include/wfa_hip.h, "placement": CLIPS).  A unit whose
        unclipped start hangs over an end of its text is alone.  Placement, pairing and ``insert`` keep the core either way.
        ``dup_qualities`` (a ``QualitySet`` made for ``patterns``, or what ``quality_set`` takes with offset 33): the
        representative is the unit with the greatest sum of base qualities of at least ``dup_min_quality`` (0 .. 93; 15 as in
        Picard and samtools markdup) over its read, or its two reads, instead of the greatest alignment score; one more kernel
        and 4 bytes per read.  The returned keys are the same under every option.  Any of the three without ``duplicates=True``
        is a ValueError.  Not done: matching a lone read against an end of a proper fragment, optical duplicates, UMIs, a library
        or read-group split, clips wider than 65 535 bases, qualities of a pattern window rather than of the whole read.
        ``duplicates=False`` returns exactly the keys above and neither allocates nor launches anything more."""
        min_score, full_gap = self._placement(min_score, full_gap, min_insert=min_insert, max_insert=max_insert, unpaired=unpaired)
        if min_insert is None or max_insert is None or not 0 <= int(min_insert) <= int(max_insert) < 2**31:
            raise ValueError(f"min_insert = {min_insert}, max_insert = {max_insert} are out of range (0 <= min_insert <= max_insert)")
        if unpaired is None:
            unpaired = full_gap
        if not 0 <= int(unpaired) < 2**31:
            raise ValueError(f"unpaired = {unpaired} is out of range (at least 0)")
        if not isinstance(rescue, (bool, np.bool_)):
            raise ValueError(f"rescue must be True or False, got {rescue!r}")
        unclipped, min_quality = self._dup_options(duplicates, dup_ends, dup_qualities, dup_min_quality)
        for name, v in (("rescue_pad", rescue_pad), ("rescue_mapq", rescue_mapq)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} must be an integer, got {v!r}")
        if int(rescue_pad) < 0:
            raise ValueError(f"rescue_pad = {rescue_pad} is out of range (at least 0)")
        if not 0 <= int(rescue_mapq) <= 60:
            raise ValueError(f"rescue_mapq = {rescue_mapq} is out of range (0 .. 60)")
        # the free ends of the rescue alignments: a bound on the insert range and the pad together, which only a rescue has
        free = (int(max_insert) - int(min_insert)) + 2 * int(rescue_pad)
        if rescue and free >= 2**31:
            raise ValueError(f"max_insert - min_insert = {int(max_insert) - int(min_insert)} with rescue_pad = {rescue_pad} is out of range "
                             "for a rescue ((max_insert - min_insert) + 2 * rescue_pad below 2^31)")
        if rescue and self._cfg.scope != 1:
            raise ValueError("rescue needs scope='full': under scope score a hit's interval is its whole window, and a rescue window "
                             "is as wide as the insert range")
        if rescue and self._cfg.span != 1:
            raise ValueError("rescue needs span='ends-free': the rescued mate lies somewhere inside its window")
        w = self._windows(patterns, texts, i, j, pattern_start, pattern_len, text_start, text_len, reverse)
        nreads = w.nreads
        if mates is None:
            if nreads % 2:
                raise ValueError(f"mates=None takes the reads as interleaved pairs: {nreads} reads are an odd number")
            mates = nreads // 2
        else:
            mates = np.asarray(mates)
            if mates.ndim != 2 or mates.shape[1] != 2 or (mates.size and not np.issubdtype(mates.dtype, np.integer)):
                raise ValueError(f"mates must be an integer array of shape (F, 2), got shape {mates.shape} of {mates.dtype}")
            m = mates.astype(np.int64).reshape(-1, 2)
            bad = np.flatnonzero(((m < 0) | (m >= nreads)).any(axis=1))
            if bad.size:
                raise ValueError(f"mates[{bad[0]}] = ({m[bad[0], 0]}, {m[bad[0], 1]}) is out of range ({nreads} reads)")
            bad = np.flatnonzero(m[:, 0] == m[:, 1])
            if bad.size:
                raise ValueError(f"mates[{bad[0]}] = ({m[bad[0], 0]}, {m[bad[0], 1]}): the two mates are one read")
            flat = m.ravel()
            order = np.argsort(flat, kind="stable")
            again = order[1:][flat[order][1:] == flat[order][:-1]]
            if again.size:
                f = int(again.min()) // 2
                raise ValueError(f"mates[{f}] = ({m[f, 0]}, {m[f, 1]}): read {flat[again.min()]} belongs to an earlier fragment")
        qblob = self._dup_quality_blob(w, dup_qualities)
        with w:
            placer = w.attach(self._native.placer(nreads))
            out = w.run(each=self._hits_into(placer, w.arrays))
            how = (min_score, full_gap, int(min_insert), int(max_insert), int(unpaired))
            n0 = w.arrays[0].shape[0]
            if rescue:
                _, found = placer.rescue(w.pset, w.text_set, mates, *how, pad=int(rescue_pad), min_len=free, anchor_mapq=int(rescue_mapq))
                ri, rj, rts, rtl, rrev, rfrag, ranchor = (np.ascontiguousarray(found[:, c]) for c in range(7))
                if found.shape[0]:
                    rrev8 = rrev.astype(np.uint8)
                    rescued = (ri, rj, None, None, rts, rtl, rrev8)
                    lens = [w.pset.length[ri].astype(np.int64), rtl.astype(np.int64)]
                    before = (self.text_begin_free, self.text_end_free)
                    try:
                        self.text_begin_free = free
                        self.text_end_free = free
                        more = self._run_windows(w.pset, w.tset, rescued, lens, each=self._hits_into(placer, rescued))
                    finally:
                        self.text_begin_free, self.text_end_free = before
                    out["score"] = np.concatenate([out["score"], more["score"]])
                    out["status"] = np.concatenate([out["status"], more["status"]])
            rows, flags, pair_rows, pair_flags = placer.run_pairs(mates, *how)
            out["flag"] = flags
            out["reads"] = _columns(rows, _native.PLACE_COLUMNS)
            out["pair_flag"] = pair_flags
            out["pairs"] = _columns(pair_rows, _native.PAIR_COLUMNS)
            if rescue:
                pairs = out["pairs"]
                pairs["rescued"] = ((pairs["proper"] == 1) & ((pairs["hit1"] >= n0) | (pairs["hit2"] >= n0))).astype(np.int32)
                out["rescue"] = dict(i=ri, j=rj, text_start=rts, text_len=rtl, reverse=rrev, fragment=rfrag, anchor=ranchor)
            if duplicates:
                read_rows, frag_rows = self._mark_duplicates(w, placer, mates, how, unclipped, dup_qualities, qblob, min_quality)
                out["reads"].update(_dup_columns(read_rows))
                out["pairs"].update(_dup_columns(frag_rows))
            return out

    def score_matrix(self, patterns, texts=None):
        """Score every pattern against every text on the GPU: returns ``(score, status)``, int32 arrays of shape (M, N).

        Cell (i, j) is what ``wavefront_align_batch`` gives for the pair (patterns[i], texts[j]) with ``scope="score"`` (this
        aligner's configuration otherwise; no CIGARs whatever its scope).  ``texts=None``: all-vs-all, the N x N matrix of
        ``patterns`` against itself, diagonal included.  Each sequence is uploaded and packed once, the M x N pairs are generated on
        the device.  With ``devices=[...]`` the run takes the first device only."""
        return self._cross(patterns, texts, _native.CROSS_DENSE)

    def completed_pairs(self, patterns, texts=None):
        """The cells of ``score_matrix`` whose status is 0, without the M x N matrix on either side: ``dict(i=, j=, score=)`` of
        int32 arrays in row-major order of (i, j).  ``texts=None``: all-vs-all, the pairs i < j only.  Meant for runs under
        ``max_steps`` (the pairs within that score: clustering, de-duplication, nearest candidates)."""
        return self._cross(patterns, texts, _native.CROSS_COMPLETED)

    def nearest(self, patterns, texts=None, k=1):
        """The ``k`` best cells of every row of ``score_matrix``, reduced on the GPU without the M x N matrix on either side:
        ``dict(j=, score=)`` of int32 arrays of shape (M, k), best first.  Only cells whose status is 0 count (those of
        ``completed_pairs``); best is the larger score, ties to the smaller j.  ``texts=None``: all-vs-all, row i takes every
        j != i (the diagonal is excluded).  A row with fewer than ``k`` such cells is padded with ``j = -1``, ``score = INT32_MIN``.
        ``k``: 1 .. 64.  Meant for runs under ``max_steps`` (the nearest candidates of every query, with a bounded output)."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"k must be an integer in 1 .. {_native.CROSS_MAX_K}, got {k!r}")
        if not 1 <= int(k) <= _native.CROSS_MAX_K:
            raise ValueError(f"k must be in 1 .. {_native.CROSS_MAX_K}, got {k}")
        return self._cross(patterns, texts, _native.CROSS_TOPK, int(k))

    # ------------------------------------------------------------------ results
    @property
    def status(self):
        return self._status

    @property
    def score(self):
        return self._score

    @property
    def cigarstring(self):
        return _ops_to_string(self._ops)

    @property
    def cigartuples(self):
        return _ops_to_tuples(self._ops)

    @property
    def locations(self):
        """(pattern_start, pattern_end, text_start, text_end) (align.pyx:788-833)."""
        if self.scope == "score":
            return [0, 0, 0, 0]
        ct = self.cigartuples
        if not ct or self.text_len == 0 or self.pattern_len == 0:
            return [0, 0, 0, 0]
        _, _, ps, pe, ts, te = _flank_scan(ct, 1, 1, self.text_len, self.pattern_len)
        return ps, pe, ts, te

    def cigar_print_pretty(self, file_name=None):
        """ALIGNMENT / ETRACE / CIGAR + three alignment rows: the text of cigar_print_pretty
        (WFA2_lib/alignment/cigar.c:778-863, called by align.pyx:445-459) from the C ABI's wfa_hip_cigar_sprint_pretty."""
        out = _native.cigar_sprint_pretty(self._ops, self._bpattern, self._text.encode("ascii"))
        if file_name:
            with open(file_name, "w") as f:
                f.write(out)
        else:
            sys.stdout.write(out)

    # ------------------------------------------------------------------ configuration properties
    def _int_prop(name):  # noqa: N805
        def getter(self):
            return getattr(self._cfg, name)

        def setter(self, value):
            old = getattr(self._cfg, name)
            setattr(self._cfg, name, int(value))
            try:
                self._push()
            except Exception:
                setattr(self._cfg, name, old)
                raise
        return property(getter, setter)

    pattern_begin_free = _int_prop("pattern_begin_free")
    pattern_end_free = _int_prop("pattern_end_free")
    text_begin_free = _int_prop("text_begin_free")
    text_end_free = _int_prop("text_end_free")
    min_wavefront_length = _int_prop("min_wavefront_length")
    max_distance_threshold = _int_prop("max_distance_threshold")
    steps_between_cutoffs = _int_prop("steps_between_cutoffs")
    xdrop = _int_prop("xdrop")
    mismatch_penalty = _int_prop("mismatch")
    gap_opening_penalty = _int_prop("gap_opening")
    gap_extension_penalty = _int_prop("gap_extension")
    gap_opening2_penalty = _int_prop("gap_opening2")
    gap_extension2_penalty = _int_prop("gap_extension2")
    match_score = _int_prop("match")
    del _int_prop

    def _enum_prop(name, table, exc, msg, canon=None):  # noqa: N805
        inv = {v: k for k, v in (canon or table).items()}

        def getter(self):
            return inv[getattr(self._cfg, name)]

        def setter(self, value):
            if value not in table:
                raise exc(msg.format(value))
            old = getattr(self._cfg, name)
            setattr(self._cfg, name, table[value])
            try:
                self._push()
            except Exception:
                setattr(self._cfg, name, old)
                raise
        return property(getter, setter)

    scope = _enum_prop("scope", _native.SCOPE, ValueError, "{} scope not understood")
    span = _enum_prop("span", _native.SPAN, NotImplementedError, "{} span not implemented")
    heuristic = _enum_prop("heuristic", _native.HEUR, NotImplementedError, "{} heuristic not implemented")
    distance = _enum_prop("distance", _native.DIST, NotImplementedError, "{} distance not implemented")
    # the reference's setter accepts "med" where the constructor wants "medium" (align.pyx:547-549)
    memory_mode = _enum_prop("memory_mode", dict(_native.MEM, med=1), NotImplementedError,
                             "{} memory_mode not implemented", canon=_native.MEM)
    del _enum_prop

    @property
    def wildcard(self):
        return self._wildcard

    @wildcard.setter
    def wildcard(self, wildcard):
        if wildcard is not None:
            if not isinstance(wildcard, str):
                raise TypeError(f"expected wildcard to be a string, but it is {type(wildcard)}")
            if len(wildcard) > 1:
                raise ValueError(f"wildcard must have length 1, but has length {len(wildcard)}")
            self._wildcard = wildcard
            self._bwildcard = wildcard.upper().encode("ascii")[0]
        else:
            self._wildcard = None
            self._bwildcard = -1

    @property
    def max_steps(self):
        return self._cfg.max_steps if self._cfg.max_steps > 0 else _INT_MAX

    @max_steps.setter
    def max_steps(self, steps):
        steps = int(steps)
        old = self._cfg.max_steps
        self._cfg.max_steps = steps if 0 < steps < _INT_MAX else 0
        try:
            self._push()
        except Exception:
            self._cfg.max_steps = old
            raise

    def close(self):
        self._native.close()
        if self._multi is not None:
            self._multi.close()
