"""Every WavefrontAligner entry point runs the configuration its getters report (CPU: the native aligners are recording fakes).

The setters push a new configuration to the library at once, except the wildcard, which is pushed when the next call needs it; a
call that did not look for it ran the previous wildcard.  The fakes keep a copy of the configuration they were given (Python passes
its own Config by reference) and record it with every call."""
import numpy as np
import pytest

from pywfa_amd import _native, datagen
import pywfa_amd
from pywfa_amd.align import _INT_MAX

FIELDS = [n for n, _ in _native.Config._fields_]
PATS = ["ACGTACGTAC", "ACGTTCGTAC", "ACGNACGTAC"]
TXTS = ["ACGTACGTAC", "ACGTACGTAC", "ACGTNCGTAC"]
BATCH = datagen.from_strings(PATS, TXTS)


def _snap(cfg):
    return {n: getattr(cfg, n) for n in FIELDS}


class _Run:
    def __init__(self, n, k):
        self.n, self.k = n, k

    def dense(self):
        return np.zeros((self.n, self.n), np.int32), np.zeros((self.n, self.n), np.int32)

    def completed(self):
        return {"i": np.zeros(0, np.int32), "j": np.zeros(0, np.int32), "score": np.zeros(0, np.int32)}

    def topk(self):
        return {"j": np.full((self.n, self.k), -1, np.int32), "score": np.zeros((self.n, self.k), np.int32)}

    def close(self):
        pass


class _Set:
    def __init__(self, n):
        self.n = n

    def close(self):
        pass


class _Resident:
    def __init__(self, owner, batch):
        self.owner, self.n = owner, len(batch["p_len"])
        owner.record("batch")

    def run(self, stream=None):
        pass

    def sync(self):
        pass

    def results(self, want_cigar):
        z = np.zeros(self.n, np.int32)
        return z, z.copy(), ((np.zeros(1, np.uint8), np.zeros(self.n, np.int64), np.zeros(self.n, np.int32)) if want_cigar else None)

    def rle(self):
        return np.zeros(self.n + 1, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros((self.n, 4), np.int32)

    def close(self):
        pass


class _Fake:
    """Stands in for _native.Aligner / _native.MultiAligner: validates like the library (wfa_hip_config_validate) and records the
    configuration it holds at every call."""
    log = []
    refuse_next = False

    def __init__(self, cfg, *args):
        self._cfg = self._take(cfg)

    def _take(self, cfg):
        rc, msg = _native.validate(cfg)
        if rc != _native.OK:
            raise ValueError(msg)
        return cfg.copy()

    def record(self, what):
        _Fake.log.append((type(self).__name__, what, _snap(self._cfg)))

    def set_config(self, cfg):
        if _Fake.refuse_next:
            _Fake.refuse_next = False
            raise RuntimeError("refused")
        self._cfg = self._take(cfg)

    def get_config(self):
        return self._cfg.copy()

    def close(self):
        pass

    def align_pair(self, pattern, text, want_cigar):
        self.record("align_pair")
        return 0, 0, (b"M" * len(pattern) if want_cigar else None)

    def align_batch(self, batch, want_cigar, out=None):
        self.record("align_batch")
        n = len(batch["p_len"])
        z = np.zeros(n, np.int32)
        return z, z.copy(), ((np.zeros(1, np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int32)) if want_cigar else None)

    def batch(self, batch):
        return _Resident(self, batch)

    def seqset(self, seqs, off, length):
        self.record("seqset")
        return _Set(len(length))

    def cross(self, patterns, texts=None, want=None, k=None):
        self.record("cross")
        return _Run(patterns.n, k or 1)


class _FakeMulti(_Fake):
    pass


@pytest.fixture
def fakes(monkeypatch):
    monkeypatch.setattr(_native, "Aligner", _Fake)
    monkeypatch.setattr(_native, "MultiAligner", _FakeMulti)
    _Fake.log = []
    _Fake.refuse_next = False
    return _Fake.log


def reported(a):
    """The configuration the getters of ``a`` report, as Config fields."""
    c = {n: getattr(a._cfg, n) for n in FIELDS}   # (fields without a getter of their own: reserved)
    c.update(distance=_native.DIST[a.distance], match=a.match_score, mismatch=a.mismatch_penalty,
             gap_opening=a.gap_opening_penalty, gap_extension=a.gap_extension_penalty, gap_opening2=a.gap_opening2_penalty,
             gap_extension2=a.gap_extension2_penalty, scope=_native.SCOPE[a.scope], span=_native.SPAN[a.span],
             pattern_begin_free=a.pattern_begin_free, pattern_end_free=a.pattern_end_free, text_begin_free=a.text_begin_free,
             text_end_free=a.text_end_free, heuristic=_native.HEUR[a.heuristic], min_wavefront_length=a.min_wavefront_length,
             max_distance_threshold=a.max_distance_threshold, steps_between_cutoffs=a.steps_between_cutoffs, xdrop=a.xdrop,
             memory_mode=_native.MEM[a.memory_mode], max_steps=0 if a.max_steps == _INT_MAX else a.max_steps,
             wildcard=-1 if a.wildcard is None else ord(a.wildcard.upper()))
    return c


ENTRIES = {
    "wavefront_align": lambda a: a.wavefront_align(TXTS[1], PATS[1]),
    "wavefront_align_batch": lambda a: a.wavefront_align_batch(TXTS, PATS),
    "align_batch": lambda a: a.align_batch(BATCH),
    "align_batch_results": lambda a: a.align_batch_results(BATCH),
    "resident_batch": lambda a: a.resident_batch(BATCH).close(),
    "score_matrix": lambda a: a.score_matrix(PATS),
    "completed_pairs": lambda a: a.completed_pairs(PATS, TXTS),
    "nearest": lambda a: a.nearest(PATS, k=2),
}

SETTERS = [("wildcard", "N"), ("wildcard", "n"), ("scope", "score"), ("distance", "levenshtein"), ("match_score", -1),
           ("mismatch_penalty", 3), ("span", "end-to-end"), ("text_end_free", 2), ("heuristic", "adaptive"), ("max_steps", 7),
           ("memory_mode", "biwfa"), ("xdrop", 33)]


def _assert_calls_follow_getters(a, log, entry):
    log.clear()
    ENTRIES[entry](a)
    assert log, entry
    want = reported(a)
    for who, what, cfg in log:
        assert cfg == want, f"{entry}: {who}.{what} ran {_diff(cfg, want)}"


def _diff(got, want):
    return ", ".join(f"{k}={got[k]} (getters: {want[k]})" for k in FIELDS if got[k] != want[k])


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("setter,value", SETTERS)
def test_entry_point_runs_what_the_getters_report(fakes, entry, setter, value):
    a = pywfa_amd.WavefrontAligner(PATS[0])
    ENTRIES["wavefront_align"](a)        # (a first call: anything pushed lazily has been pushed)
    setattr(a, setter, value)
    if entry == "align_batch_results" and setter == "scope":
        with pytest.raises(ValueError):   # (scope full only)
            ENTRIES[entry](a)
        return
    _assert_calls_follow_getters(a, fakes, entry)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_wildcard_set_and_cleared_reaches_every_entry_point(fakes, entry):
    a = pywfa_amd.WavefrontAligner(PATS[0], wildcard="N")
    ENTRIES[entry](a)
    a.wildcard = None
    _assert_calls_follow_getters(a, fakes, entry)
    a.wildcard = "A"
    _assert_calls_follow_getters(a, fakes, entry)


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("refused,value", [("mismatch_penalty", 0), ("scope", "half"), ("distance", "hamming"),
                                           ("pattern_begin_free", -1)])
def test_wildcard_then_a_refused_setter(fakes, entry, refused, value):
    """A refused setter does not count the pending wildcard as pushed."""
    a = pywfa_amd.WavefrontAligner(PATS[0])
    ENTRIES["wavefront_align"](a)
    a.wildcard = "N"
    with pytest.raises((ValueError, NotImplementedError)):
        setattr(a, refused, value)
    _assert_calls_follow_getters(a, fakes, entry)


@pytest.mark.parametrize("entry", ["wavefront_align_batch", "align_batch"])
def test_multi_device_entry_follows_the_getters(fakes, entry):
    a = pywfa_amd.WavefrontAligner(PATS[0], devices=[0, 0])
    ENTRIES[entry](a)
    assert any(who == "_FakeMulti" for who, _, _ in fakes)
    for setter, value in SETTERS:
        if setter == "memory_mode":
            continue
        setattr(a, setter, value)
        _assert_calls_follow_getters(a, fakes, entry)


def test_a_refused_push_takes_every_setter_back(fakes):
    """A push the library refuses leaves the getters — max_steps included — at what the library still runs."""
    a = pywfa_amd.WavefrontAligner(PATS[0], max_steps=5)
    ENTRIES["wavefront_align"](a)
    for setter, value in [("max_steps", 9), ("max_steps", 0), ("mismatch_penalty", 3), ("scope", "score"), ("wildcard", "N")]:
        old = getattr(a, setter)
        _Fake.refuse_next = True
        if setter == "wildcard":
            a.wildcard = value    # (pushed by the next call: that call raises, and the wildcard stays pending)
            with pytest.raises(RuntimeError):
                ENTRIES["align_batch"](a)
            a.wildcard = old
        else:
            with pytest.raises(RuntimeError):
                setattr(a, setter, value)
        assert getattr(a, setter) == old, setter
        _assert_calls_follow_getters(a, fakes, "align_batch")
