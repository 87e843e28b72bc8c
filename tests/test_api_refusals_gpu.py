"""Refusal parity of the resident-set entries (csrc/api_*.hip, wfa_hip_batch_summary): the walk of bad calls of
tools/make_api_refusals.py against the current library, compared case by case with tests/golden/api_refusals.json — the return code
(or the null handle) and both error channels, ``wfa_hip_last_error(al)`` and ``wfa_hip_global_error()``, for equality.  The golden
file was recorded from the library before the entries were rewritten on their shared helpers, so a refusal that
changed its code, its text, its place among the checks or its channel shows here.

The walk uses two sets of three sequences of 14 - 40 bases and runs two batches of three pairs (what "a finished batch" takes), two
3 x 3 cross runs and one seed index, for the handles whose read-out entries refuse; every other call is refused before it launches.
A creator that came back with a handle is recorded as such.  The walk ends by destroying every handle and then the aligner, under no
live handle: the C ABI has no getter for an aligner's handle count, so what a refused create must not do to it is pinned by the
creators going through one adopt step (host_sets.hpp) and by tests/test_handles_gpu.py."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def walk(gpu):
    spec = importlib.util.spec_from_file_location("make_api_refusals", os.path.join(ROOT, "tools", "make_api_refusals.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "tests", "golden", "api_refusals.json")) as f:
        golden = json.load(f)
    return tool, golden, tool.record()


def test_the_walk_is_the_recorded_one(walk):
    tool, golden, got = walk
    assert [(c["entry"], c["case"]) for c in got] == [(c["entry"], c["case"]) for c in golden["cases"]]
    assert [list(s) for s in tool.SKIPPED] == [[s["entry"], s["branch"], s["reason"]] for s in golden["skipped"]]


def test_every_refusal_keeps_its_code_and_both_messages(walk):
    _, golden, got = walk
    different = [(g, w) for g, w in zip(got, golden["cases"]) if g != w]
    assert not different, "\n".join(f"{w['entry']} ({w['case']}):\n  recorded {w}\n  now      {g}" for g, w in different)


def test_the_walk_refuses(walk):
    """The recorded walk itself: every case a refusal (no handle, no OK), and the entries it reaches."""
    _, golden, _ = walk
    cases = golden["cases"]
    assert all(c["rc"] == "null" or (isinstance(c["rc"], int) and c["rc"] < 0) for c in cases), [c for c in cases if c["rc"] in (0, "handle")]
    # 38 entries in the five units and the summary entry; the five destroys and wfa_hip_placer_count refuse nothing
    assert len({c["entry"] for c in cases}) == 38 + 1 - 5 - 1
