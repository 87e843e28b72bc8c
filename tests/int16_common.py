"""Corpus of tests/test_int16_range_gpu.py (test infrastructure): pairs whose END carries the work, at exact lengths, and pairs
that share no base (a known score after a known number of steps).

Every kernel that keeps offsets or history entries in int16 does so under a host condition on the longest read of the batch
(DESIGN §3.5 "The int16 forms and their limits").  The largest offsets of an alignment are its last ones, so the edits sit in the
last 16 bases: the last extension, the termination test and the first entries of a walk run at offsets L - 16 ... L."""
import numpy as np

from pywfa_amd import datagen

KINDS = ("mismatch", "insertion", "deletion", "ragged")
_OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def end_pair(plen, tlen, kind, seed):
    """One pair of exactly (plen, tlen) bases at 1 % divergence, cut from the END of a generated pair so that the two tails line up.
    The last 64 bases of the text are the pattern's, then: `mismatch` = the last base differs; `insertion` = 1 - 3 extra bases in the
    text 7 bases before its end; `deletion` = 1 - 2 bases of the text missing 9 bases before its end."""
    b = datagen.generate(1, max(plen, tlen) + 256, 0.01, seed)
    p, t = datagen.pair_strings(b, 0)
    t = t[:-64] + p[-64:]
    if kind == "mismatch":
        t = t[:-1] + _OTHER[t[-1]]
    elif kind == "insertion":
        n = 1 + seed % 3
        t = t[:-7] + (_OTHER[t[-7]] + _OTHER[t[-8]] + _OTHER[t[-7]])[:n] + t[-7:]
    elif kind == "deletion":
        n = 1 + seed % 2
        t = t[:-9 - n] + t[-9:]
    assert len(p) >= plen and len(t) >= tlen
    return p[len(p) - plen:], t[len(t) - tlen:]


def length_batch(L, seed, kinds=KINDS):
    """The four pairs of a length case: L is the longer sequence of every pair, and only the mismatch pair ends on diagonal 0."""
    pats, txts = [], []
    for j, kind in enumerate(kinds):
        s = seed + 7 * j
        if kind == "mismatch": p, t = end_pair(L, L, kind, s)
        elif kind == "insertion": p, t = end_pair(L - (1 + s % 3), L, kind, s)
        elif kind == "deletion": p, t = end_pair(L, L - (1 + s % 2), kind, s)
        else: p, t = end_pair(L, L, "mismatch", s); t = t[:-50]   # ragged: the last 50 bases of the pattern have no text
        assert max(len(p), len(t)) == L
        pats.append(p); txts.append(t)
    return datagen.from_strings(pats, txts)


def shape_batch(plen, tlen, seed):
    """The pairs of a (plen, tlen) case of the wide kernel: the three end edits at exactly these lengths (what the edit adds or removes is
    made up at the front of the pair), and the ragged pair (plen, plen - 50); the longest sequence of the batch is max(plen, tlen)."""
    pats, txts = [], []
    for j, kind in enumerate(KINDS):
        p, t = end_pair(plen, tlen, kind, seed + 7 * j) if kind != "ragged" else end_pair(plen, plen, "mismatch", seed + 7 * j)
        if kind == "ragged": t = t[:-50]
        pats.append(p); txts.append(t)
    b = datagen.from_strings(pats, txts)
    assert int(max(b["p_len"].max(), b["t_len"].max())) == max(plen, tlen)
    return b


def step_batch(n, seed=77):
    """`A` x n against `C` x n — no base matches, so under (4, 6, 2) the score is -4 n after 2 n steps of 2 — and the same with one
    random 200-mer appended to both: an extension of 200 bases after the long run of steps."""
    rng = np.random.default_rng(seed)
    r = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 200)].tobytes().decode()
    return datagen.from_strings(["A" * n, "A" * n + r], ["C" * n, "C" * n + r])
