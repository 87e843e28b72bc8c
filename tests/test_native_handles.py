"""The resident handles of pywfa_amd._native over a fake library: what a NULL create raises, that the destroy symbol is called
once, and how a non-OK code of a method becomes an exception.  No GPU and no libwfa_hip.so: ``_native._lib`` is swapped for an
object that records calls and returns scripted handles, codes and error strings."""
import gc

import numpy as np
import pytest

from pywfa_amd import _native

HANDLE = 0x1000
ERROR_SOURCES = ("wfa_hip_last_error", "wfa_hip_multi_last_error", "wfa_hip_global_error")


class FakeLib:
    """Every ``wfa_hip_*`` attribute is a function that records its name and returns ``returns[name]``; by default a create symbol
    returns a handle, a destroy symbol None and anything else 0 (WFA_HIP_OK).  ``errors``: what each error source returns."""

    def __init__(self):
        self.calls = []
        self.returns = {}
        self.errors = {name: name.encode() for name in ERROR_SOURCES}   # (each source tells its own name unless scripted)
        self.validate = (_native.OK, "")

    def __getattr__(self, name):
        if not name.startswith("wfa_hip_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append(name)
            if name in self.errors:
                return self.errors[name]
            if name == "wfa_hip_config_validate":
                args[1].value = self.validate[1].encode()
                return self.validate[0]
            if name in self.returns:
                return self.returns[name]
            if name.endswith("_destroy"):
                return None
            return HANDLE if name in CREATES else 0

        return call


@pytest.fixture
def fake():
    saved, _native._lib = _native._lib, FakeLib()
    try:
        yield _native._lib
    finally:
        _native._lib = saved


def _set(al):
    return _native.SeqSet(al, np.frombuffer(b"ACGTACGT", np.uint8), np.array([0, 4]), np.array([4, 4]))


def _batch():
    return dict(seqs=np.frombuffer(b"ACGTACGA", np.uint8), p_off=np.array([0]), p_len=np.array([4]), t_off=np.array([4]),
                t_len=np.array([4]))


# class name -> (create symbol, destroy symbol, constructor given the aligner, one method and the symbol it calls)
HANDLES = {
    "SeqSet": ("wfa_hip_seqset_create", "wfa_hip_seqset_destroy", _set, None, None),
    "CrossRun": ("wfa_hip_cross_run", "wfa_hip_cross_destroy", lambda al: _native.CrossRun(al, _set(al)),
                 lambda h: h.dense(), "wfa_hip_cross_dense"),
    "Pileup": ("wfa_hip_pileup_create", "wfa_hip_pileup_destroy", lambda al: _native.Pileup(al, _set(al)),
               lambda h: h.clear(), "wfa_hip_pileup_clear"),
    "Placer": ("wfa_hip_placer_create", "wfa_hip_placer_destroy", lambda al: _native.Placer(al, 3),
               lambda h: h.clear(), "wfa_hip_placer_clear"),
    "SeedIndex": ("wfa_hip_seed_index_create", "wfa_hip_seed_index_destroy", lambda al: _native.SeedIndex(al, _set(al), 5),
                  lambda h: h.stats(), "wfa_hip_seed_index_stats"),
    "MultiAligner": ("wfa_hip_multi_create", "wfa_hip_multi_destroy", lambda al: _native.MultiAligner(_native.Config(), [0, 1]),
                     lambda h: h.set_config(_native.Config()), "wfa_hip_multi_set_config"),
    "ResidentBatch": ("wfa_hip_batch_create", "wfa_hip_batch_destroy", lambda al: _native.ResidentBatch(al, _batch()),
                      lambda h: h.sync(), "wfa_hip_batch_sync"),
}
CREATES = {"wfa_hip_create"} | {spec[0] for spec in HANDLES.values()}


@pytest.fixture
def aligner(fake):
    al = _native.Aligner(_native.Config())
    yield al
    al.close()


def _script_null(fake, name, message):
    """``name``'s create returns NULL and the error source it reads says ``message``."""
    fake.returns[HANDLES[name][0]] = None
    fake.errors["wfa_hip_global_error" if name == "MultiAligner" else "wfa_hip_last_error"] = message.encode()


@pytest.mark.parametrize("name", HANDLES)
def test_null_create_with_a_validation_message_is_a_value_error(fake, aligner, name):
    create, destroy, make, _, _ = HANDLES[name]
    _script_null(fake, name, "invalid arguments")
    if name == "MultiAligner":   # (its validation message is that of wfa_hip_config_validate, which it raises as it is)
        fake.validate = (_native.EINVAL, "mismatch must be positive")
    with pytest.raises(ValueError) as e:
        make(aligner)
    assert not isinstance(e.value, _native.NativeError)
    assert str(e.value) == ("mismatch must be positive" if name == "MultiAligner" else f"{create}: invalid arguments")
    del e
    gc.collect()
    assert create in fake.calls and destroy not in fake.calls   # (the half-constructed object has nothing to destroy)


@pytest.mark.parametrize("name", HANDLES)
def test_null_create_with_a_device_failure_is_a_native_error(fake, aligner, name):
    create, destroy, make, _, _ = HANDLES[name]
    message = "hipMalloc(&p, n) failed: out of memory (api.hip:1)"
    _script_null(fake, name, message)
    with pytest.raises(_native.NativeError) as e:
        make(aligner)
    assert str(e.value) == (f"{create} failed: {message}" if name == "MultiAligner" else f"{create}: {message}")
    del e
    gc.collect()
    assert create in fake.calls and destroy not in fake.calls


def test_multi_create_refused_as_not_supported(fake):
    _script_null(fake, "MultiAligner", "unused")
    fake.validate = (_native.ENOTSUP, "biwfa with free ends")
    with pytest.raises(NotImplementedError, match="^biwfa with free ends$"):
        _native.MultiAligner(_native.Config(), [0, 1])


def test_seqset_device_failure_without_a_colon_is_a_native_error(fake, aligner):
    """``hipSetDevice failed``, the one device failure of wfa_hip_seqset_create that carries no colon: NativeError, as from every
    other handle class."""
    _script_null(fake, "SeqSet", "hipSetDevice failed")
    with pytest.raises(_native.NativeError, match="^wfa_hip_seqset_create: hipSetDevice failed$"):
        _set(aligner)


def test_windowed_batch_refused_is_always_a_native_error(fake, aligner):
    s = _set(aligner)
    fake.returns["wfa_hip_batch_create_windows"] = None
    fake.errors["wfa_hip_last_error"] = b"t_start[0] + t_len[0] runs past the sequence"
    with pytest.raises(_native.NativeError, match="^wfa_hip_batch_create_windows: t_start"):
        _native.ResidentBatch.windows(aligner, s, None, [0], [1])


@pytest.mark.parametrize("name", HANDLES)
def test_destroy_is_called_once(fake, aligner, name):
    _, destroy, make, _, _ = HANDLES[name]
    h = make(aligner)
    assert h._h == HANDLE
    assert destroy not in fake.calls
    h.close()
    assert h._h is None
    h.close()
    del h
    gc.collect()
    assert fake.calls.count(destroy) == 1


@pytest.mark.parametrize("name", [n for n in HANDLES if n != "MultiAligner"])
def test_closing_the_aligner_closes_its_open_handles(fake, name):
    _, destroy, make, _, _ = HANDLES[name]
    al = _native.Aligner(_native.Config())
    h = make(al)
    assert h.aligner is al and h in al._batches
    al.close()
    assert h._h is None and fake.calls.count(destroy) == 1
    assert fake.calls.index(destroy) < fake.calls.index("wfa_hip_destroy")   # (the handles go first)
    h.close()
    assert fake.calls.count(destroy) == 1


@pytest.mark.parametrize("code,exc", [(_native.EINVAL, ValueError), (_native.ENOTSUP, NotImplementedError),
                                      (_native.EDEVICE, _native.NativeError), (-7, _native.NativeError)])
@pytest.mark.parametrize("name", [n for n in HANDLES if HANDLES[n][3] is not None])
def test_a_code_of_a_method_becomes_its_exception(fake, aligner, name, code, exc):
    _, _, make, method, symbol = HANDLES[name]
    h = make(aligner)
    fake.returns[symbol] = code
    fake.errors["wfa_hip_last_error"] = b"the aligner's last error"
    fake.errors["wfa_hip_multi_last_error"] = b"the multi aligner's last error"
    with pytest.raises(exc) as e:
        method(h)
    assert type(e.value) is exc
    source = "the multi aligner's last error" if name == "MultiAligner" else "the aligner's last error"
    assert str(e.value) == f"{symbol}: {source}"
    fake.returns[symbol] = _native.OK
    method(h)
    h.close()


@pytest.mark.parametrize("code,exc", [(_native.EINVAL, ValueError), (_native.ENOTSUP, NotImplementedError),
                                      (_native.EDEVICE, _native.NativeError)])
def test_a_code_of_the_aligner_becomes_its_exception(fake, aligner, code, exc):
    fake.returns["wfa_hip_set_config"] = code
    fake.errors["wfa_hip_last_error"] = b"gap_extension must be positive"
    with pytest.raises(exc) as e:
        aligner.set_config(_native.Config())
    assert type(e.value) is exc and str(e.value) == "wfa_hip_set_config: gap_extension must be positive"


def test_pileup_rows_to_the_end_of_the_sequence(fake, aligner):
    p = _native.Pileup(aligner, _set(aligner))
    assert p.read(1, 1).shape == (3, _native.PILEUP_COLS)
    assert p.calls(_set(aligner), 0).shape == (4,)
    assert p.read(0, 1, 2).shape == (2, _native.PILEUP_COLS)
    for call in (lambda: p.read(2), lambda: p.calls(_set(aligner), -1)):
        with pytest.raises(ValueError, match="is out of range for a set of 2"):
            call()


def test_symbols_are_unique_and_all_have_a_signature():
    assert len(set(_native.SYMBOLS)) == len(_native.SYMBOLS)
    assert list(_native.SIGNATURES) == _native.SYMBOLS
    for name, sig in _native.SIGNATURES.items():
        assert isinstance(sig, tuple) and len(sig) == 2, name
