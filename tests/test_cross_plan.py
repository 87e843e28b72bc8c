"""The band planner of the score matrices (wfa_hip_plan_cross_bands, host only): every cell of the rectangle or of the upper
triangle lies in exactly one band, bands are whole rows and stay within the budget (a longer row is a band of its own)."""
import numpy as np
import pytest

from pywfa_amd import _native


def _cells(row_begin, m, n, triangle):
    seen = np.zeros((m, n), np.int32)
    for k in range(len(row_begin) - 1):
        r0, r1 = int(row_begin[k]), int(row_begin[k + 1])
        assert r1 > r0
        for i in range(r0, r1):
            seen[i, (i if triangle else 0):] += 1
    return seen


@pytest.mark.parametrize("m,n", [(1, 1), (1, 7), (7, 1), (13, 29), (29, 13), (64, 64), (100, 3), (3, 100)])
@pytest.mark.parametrize("budget", [1, 2, 5, 17, 64, 1000, 10 ** 9])
def test_rectangle_cover(m, n, budget):
    rb = _native.plan_cross_bands(m, n, False, budget)
    assert rb[0] == 0 and rb[-1] == m and np.all(np.diff(rb) > 0)
    seen = _cells(rb, m, n, False)
    assert np.all(seen == 1)
    for k in range(len(rb) - 1):
        rows = int(rb[k + 1] - rb[k])
        assert rows * n <= budget or rows == 1


@pytest.mark.parametrize("n", [1, 2, 7, 31, 64, 101])
@pytest.mark.parametrize("budget", [1, 2, 3, 10, 50, 1000, 10 ** 9])
def test_triangle_cover(n, budget):
    rb = _native.plan_cross_bands(n, n, True, budget)
    assert rb[0] == 0 and rb[-1] == n and np.all(np.diff(rb) > 0)
    seen = _cells(rb, n, n, True)
    upper = np.triu(np.ones((n, n), np.int32))
    assert np.array_equal(seen, upper)
    for k in range(len(rb) - 1):
        r0, r1 = int(rb[k]), int(rb[k + 1])
        pairs = sum(n - i for i in range(r0, r1))
        assert pairs <= budget or r1 == r0 + 1
        if k + 2 < len(rb):   # (greedy: the next row would not have fitted)
            assert pairs + (n - r1) > budget


def test_empty_and_invalid():
    assert list(_native.plan_cross_bands(0, 5, False, 10)) == [0]
    assert list(_native.plan_cross_bands(5, 0, False, 10)) == [0]
    assert list(_native.plan_cross_bands(0, 0, True, 10)) == [0]
    with pytest.raises(ValueError):
        _native.plan_cross_bands(3, 3, False, 0)
    with pytest.raises(ValueError):
        _native.plan_cross_bands(-1, 3, False, 10)


def test_header_declares_cross_abi():
    for s in ("wfa_hip_seqset_create", "wfa_hip_seqset_destroy", "wfa_hip_cross_run", "wfa_hip_cross_dense",
              "wfa_hip_cross_completed", "wfa_hip_cross_kernel_ms", "wfa_hip_cross_destroy", "wfa_hip_plan_cross_bands"):
        assert s in _native.SYMBOLS
        assert hasattr(_native.lib(), s)
