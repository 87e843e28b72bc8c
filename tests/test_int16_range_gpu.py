"""The int16 offset rows and history entries at their limits: reads of 16 000 / 32 000 bases and runs of 16 000 / 32 000 steps.

Every long-read kernel keeps offsets in int16 where the host judges that safe, each under a condition of its own (DESIGN §3.5,
"The int16 forms and their limits").  The pairs here are 1 % divergent with the work at their END (tests/int16_common.py): the last
extension, the termination test and the start of the walk run at the largest offsets the form is allowed to see; the step cases
share no base at all, so the dead cells of a row drift for as many steps as the form is allowed to run.  Expected values: the real
library where it was built (oracle/_ref), the plain oracle otherwise — computed once per batch and configuration."""
import functools

import pytest

import common
import int16_common
from oracle import loader
from pywfa_amd import _native

pytestmark = pytest.mark.gpu


# every configuration of this module (the tests add the scope where they run both)
KWS = {
    "exact": dict(span="end-to-end"),
    "adaptive": dict(span="end-to-end", scope="full", heuristic="adaptive"),
    "adaptive-ends-free": dict(span="ends-free", scope="full", heuristic="adaptive", text_end_free=40),
    "adaptive-2p": dict(distance="affine2p", span="end-to-end", scope="full", heuristic="adaptive"),
    "biwfa": dict(span="end-to-end", scope="full", memory_mode="biwfa"),
}


def _checker():
    return loader.reference() if loader.have_reference() else loader.oracle()


_length_batch = functools.lru_cache(maxsize=None)(int16_common.length_batch)
_shape_batch = functools.lru_cache(maxsize=None)(int16_common.shape_batch)
_step_batch = functools.lru_cache(maxsize=None)(int16_common.step_batch)
_expected = {}


def expected(key, batch, kw):
    k = (key, tuple(sorted(kw.items())))
    if k not in _expected:
        oc, _ = common.configs_pair(**kw)
        _expected[k] = loader.run(_checker(), oc, batch)
    return _expected[k]


def run_resident(kw, batch):
    """score, status, op strings (full scope) and the number of pairs left to the general kernel."""
    oc, nc = common.configs_pair(**kw)
    full = oc.scope == 1
    al = _native.Aligner(nc)
    try:
        rb = al.batch(batch)
        rb.run(); rb.sync()
        score, status, cig = rb.results(full)
        left = rb.fallback_pairs()
        rb.close()
    finally:
        al.close()
    cigars = None
    if full:
        ops, cb, cl = cig
        cigars = [ops[cb[i]:cb[i] + cl[i]].tobytes() for i in range(len(score))]
    return score, status, cigars, left


def check(key, batch, kw, ctx, staged=True):
    o = expected(key, batch, kw)
    score, status, cigars, left = run_resident(kw, batch)
    common.assert_same(o, score, status, cigars, batch, ctx)
    if staged:
        assert left == 0, f"{ctx}: {left} pairs were left to the general kernel"


@pytest.mark.parametrize("scope", ["score", "full"])
@pytest.mark.parametrize("tile32", ["0", "1"])
@pytest.mark.parametrize("L", [31999, 32000, 32001])
def test_exact_reads_at_the_tiled_rows_limit(gpu, L, tile32, scope, monkeypatch):
    """Exact, end-to-end, default route: up to 32 000 bases the tiled kernel's int16 rows (NULL = -32768), at 32 001 its int32 form
    (WFA_HIP_TILE32=1) or the wide kernel's int32 rows (0).  The host picks by the longest read, the kernel checks every pair against
    the same limit: nothing may be left to the general kernel."""
    monkeypatch.setenv("WFA_HIP_TILE32", tile32)
    kw = dict(KWS["exact"], scope=scope)
    check(("len", L), _length_batch(L, 3100 + L % 100), kw, f"exact L={L} tile32={tile32} {scope}")


@pytest.mark.parametrize("scope", ["score", "full"])
@pytest.mark.parametrize("plen,tlen", [(16000, 16000), (16001, 15999), (16001, 16000), (15999, 16001)])
def test_exact_reads_at_the_wide_rows_limit(gpu, plen, tlen, scope, monkeypatch):
    """WFA_HIP_TILE=0: the step-by-step wide kernel's own forms.  int16 rows (NULL = -16384) while twice the longest read of the
    batch is at most 32 000, int32 rows beyond — so (16 001, 15 999), whose sum the kernel's own per-pair test would accept, gets int32."""
    monkeypatch.setenv("WFA_HIP_TILE", "0")
    kw = dict(KWS["exact"], scope=scope)
    check(("shape", plen, tlen), _shape_batch(plen, tlen, 3300 + plen % 10 + tlen % 10), kw, f"wide ({plen}, {tlen}) {scope}")


@pytest.mark.parametrize("variant", ["default", "explicit", "ends-free"])
@pytest.mark.parametrize("L", [31999, 32000])
def test_adaptive_reads_at_the_history_limit(gpu, L, variant, monkeypatch):
    """wf-adaptive with CIGARs on the banded kernels: the piggy-back history (default), the explicit entries (WFA_HIP_BAND_PB=0:
    4 x int16 below 32 000 bases, 4 x int32 at 32 000), and one ends-free run that may leave up to 40 bases of the text."""
    if variant == "explicit":
        monkeypatch.setenv("WFA_HIP_BAND_PB", "0")
    kw = KWS["adaptive-ends-free"] if variant == "ends-free" else KWS["adaptive"]
    check(("len", L), _length_batch(L, 3100 + L % 100), kw, f"adaptive L={L} {variant}")


@pytest.mark.parametrize("L", [15999, 16000, 16001, 31999, 32000])
def test_adaptive_2p_reads_at_the_doubled_offset_limits(gpu, L):
    """gap-affine-2p under wf-adaptive: the slim kernel keeps doubled offsets in int16 for pairs of up to 16 000 bases and hands longer
    ones on (16 001); the banded kernel takes batches whose longest read is below 32 000 (31 999), the stages behind it the rest."""
    kw = KWS["adaptive-2p"]
    check(("len", L), _length_batch(L, 3100 + L % 100), kw, f"adaptive 2p L={L}", staged=False)


@pytest.mark.parametrize("bilevel", ["1", "0"])
@pytest.mark.parametrize("L", [32000, 32001])
def test_biwfa_reads_at_the_ring_limit(gpu, L, bilevel, monkeypatch):
    """BiWFA with CIGARs: the level kernels' rings are int16 (stores clamped to [-16384, 32767]) up to 32 000 bases, int32 beyond;
    WFA_HIP_BILEVEL=0 is the depth-first kernel."""
    monkeypatch.setenv("WFA_HIP_BILEVEL", bilevel)
    kw = KWS["biwfa"]
    check(("len", L), _length_batch(L, 3100 + L % 100), kw, f"biwfa L={L} bilevel={bilevel}", staged=False)


@pytest.mark.parametrize("scope", ["score", "full"])
def test_wide_int16_rows_beyond_16384_steps(gpu, scope, monkeypatch):
    """`A` x 8 200 against `C` x 8 200 (and both + one random 200-mer): score -32 800 after 16 400 steps of 2.  A dead cell of the wide
    kernel's int16 rows starts at -16 384 and gains at most 1 per step, so by then it would read as a live offset: the kernel hands the
    pair on at step 16 000, and what takes it must return the oracle's result.  (Full scope: 8 200 X; the real library needs 3 s and
    2.4 GB for the two op strings on one core, the plain oracle 6 s; score only 1.3 s / 5 s.)"""
    monkeypatch.setenv("WFA_HIP_TILE", "0")
    batch = _step_batch(8200)
    kw = dict(KWS["exact"], scope=scope)
    o = expected(("steps", 8200), batch, kw)
    assert list(o["score"]) == [-32800, -32800]
    check(("steps", 8200), batch, kw, f"16 400 steps, wide rows, {scope}", staged=False)


def test_tiled_int16_rows_beyond_32000_steps(gpu):
    """`A` x 16 001 against `C` x 16 001 (and both + one random 200-mer) on the default route: score -64 004 after 32 002 steps, more
    than the 32 000 the tiled kernel's int16 rows run (a dead cell starts at -32 768).  The pair must come back right from whatever
    takes it behind the guard.  Score only: the history of 5 x 10^8 cells fits neither the checkers' memory on a test's budget (about
    10 GB) nor a test's time.  The plain oracle needs 20 s for the two pairs on one core, so the real library (5 s) is used where it
    was built."""
    batch = _step_batch(16001)
    kw = dict(KWS["exact"], scope="score")
    o = expected(("steps", 16001), batch, kw)
    assert list(o["score"]) == [-64004, -64004]
    check(("steps", 16001), batch, kw, "32 002 steps, default route", staged=False)
