"""Seeded corpora that more than one test module uses (test infrastructure)."""
import numpy as np

from pywfa_amd import datagen


def ragged_batch(n, length, error, seed):
    """`n` pairs of about `length` bases with length differences, a few short / empty ones mixed in."""
    rng = np.random.default_rng(seed)
    b = datagen.generate(n, length, error, seed)
    pats, txts = [], []
    for i in range(n):
        p, t = datagen.pair_strings(b, i)
        k = i % 9
        if k == 1: p = p[:len(p) - int(rng.integers(1, 200))]
        if k == 2: t = t[int(rng.integers(1, 200)):]
        if k == 3: p = p[:int(rng.integers(0, 40))]
        if k == 4 and i % 36 == 4: p, t = "", t[:17]
        pats.append(p); txts.append(t)
    return datagen.from_strings(pats, txts)


def special_mini(sp):
    """64 pairs of the special corpus `sp` (tools/validate_oracle.py corpus_special): the empty / length-1 / identical / unrelated
    block, then homopolymers, two-letter reads, reads with N, long gaps, windows."""
    n_sp = len(sp["p_len"])
    pick = list(range(27)) + [27 + 30 * i for i in range(10)] + [327 + 33 * i for i in range(6)] + [527 + 12 * i for i in range(8)] + \
           [627 + 25 * i for i in range(8)] + [827 + 40 * i for i in range(5)]
    pick = [i for i in pick if i < n_sp]
    pats = [bytes(sp["seqs"][sp["p_off"][i]:sp["p_off"][i] + sp["p_len"][i]]).decode() for i in pick]
    txts = [bytes(sp["seqs"][sp["t_off"][i]:sp["t_off"][i] + sp["t_len"][i]]).decode() for i in pick]
    return datagen.from_strings(pats, txts)
