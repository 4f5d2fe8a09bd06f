"""The range search's numpy models (tests/kcheck_range.py), pinned by hand-derived cases without a
GPU: the threshold from the radius, the in-range selection, the result order and the overflow
rule.  tests/test_gpu_kernels_range.py holds the kernels to these models."""
import numpy as np
import pytest

import kcheck_range as kr
from kcheck_exact import IDX_NONE, NEG_INF, POS_INF, dist_key, exclusion_bound

F = np.float32
NO_APPROX = 2  # kQueryNoApprox (kernels.hpp; the GPU tests check it against the library's)


def ulps_up(x, k):
    for _ in range(k):
        x = np.nextafter(F(x), POS_INF)
    return F(x)


def test_threshold_plain_radius():
    """E = 0, |b| = 1, r = 0.1: the bound 1 - t - 2.5e-7 must exceed 0.1, so t sits just below
    0.9 - 2.5e-7 (the identical-row clause, t < 0.9999, is far away)."""
    t = kr.range_threshold(F(0.1), F(0), F(1))
    assert t.dtype == np.float32
    assert abs(float(t) - (0.9 - 2.5e-7)) < 2e-7
    assert exclusion_bound(t, F(0), F(1)) > F(0.1)
    assert not (exclusion_bound(ulps_up(t, 4), F(0), F(1)) > F(0.1))


def test_threshold_identical_row_clause_binds_at_radius_zero():
    """r = 0 with E = 0.01: the bound alone would allow t up to 0.99 - 2.5e-7, but rows identical to
    the query (distance 0, always in range) must be emitted: t < 1 - E - 1e-4 - 6e-9 / |b|."""
    e = F(0.01)
    lim = ((1.0 - float(e)) - 1e-4) - 6e-9
    t = kr.range_threshold(F(0), e, F(1))
    assert float(t) < lim <= float(np.nextafter(t, POS_INF))
    assert exclusion_bound(t, e, F(1)) > F(0)
    assert exclusion_bound(np.nextafter(t, POS_INF), e, F(1)) == NEG_INF
    # a tiny query magnitude lowers the clause: 6e-9 / 1e-6 = 6e-3
    t6 = kr.range_threshold(F(0), e, F(1e-6))
    lim6 = ((1.0 - float(e)) - 1e-4) - 6e-9 / float(F(1e-6))
    assert float(t6) < lim6 <= float(np.nextafter(t6, POS_INF))
    assert 0.9838 < float(t6) < 0.984


def test_threshold_not_positive_means_scan():
    """1 - r - E - 2.5e-7 <= 0: no positive threshold, the query is scanned."""
    assert kr.range_threshold(F(1), F(0), F(1)) == POS_INF
    assert kr.range_threshold(F(2), F(0), F(1)) == POS_INF
    assert kr.range_threshold(POS_INF, F(0), F(1)) == POS_INF
    assert kr.range_threshold(F(0.1), F(0.95), F(1)) == POS_INF
    assert kr.range_threshold(F(0), F(0), F(0)) == POS_INF      # (6e-9 / 0: the clause is -inf)
    # just positive: r = 0.999, E = 0 leaves about 1e-3 - 2.5e-7
    t = kr.range_threshold(F(0.999), F(0), F(1))
    assert 0.00099 < float(t) < 0.001
    assert exclusion_bound(t, F(0), F(1)) > F(0.999)
    assert not (exclusion_bound(ulps_up(t, 4), F(0), F(1)) > F(0.999))


@pytest.mark.parametrize("nb", [1.0, 1e-6])
@pytest.mark.parametrize("eb", [0.0, 0.01, 0.999, 1.0])
@pytest.mark.parametrize("r", [-1.0, 0.0, 1e-7, 0.1, 0.999, 1.0, 2.0, np.inf])
def test_threshold_grid_safe_and_tight(r, eb, nb):
    """The grid the kernel test walks: wherever the model filters, its threshold is safe
    (exclusion_bound > r) and tight (4 ulps further it no longer is)."""
    tau, scan, nan = kr.range_tau_model([r], [eb], [nb], [0], NO_APPROX)
    assert not nan
    if r < 0:
        assert tau[0] == POS_INF and not scan[0]
    elif eb >= 1 or 1.0 - r - eb - 2.5e-7 <= 0:
        assert tau[0] == POS_INF and scan[0]
    if tau[0] < POS_INF:
        assert tau[0] > 0 and not scan[0]
        assert exclusion_bound(tau[0], F(eb), F(nb)) > F(r)
        assert not (exclusion_bound(ulps_up(tau[0], 4), F(eb), F(nb)) > F(r))


def test_tau_model_flags_and_nan():
    tau, scan, nan = kr.range_tau_model([0.1, 0.1, np.nan, -0.5, 0.1], [0.01, 0.01, 0.01, 0.01, np.nan],
                                        [1, 1, 1, 1, 1], [0, NO_APPROX, 0, NO_APPROX, 0], NO_APPROX)
    assert nan
    assert tau[0] < POS_INF and not scan[0]
    assert tau[1] == POS_INF and scan[1]          # the filter cannot serve the query
    assert tau[2] == POS_INF and not scan[2]      # NaN radius: the call fails, nothing is scanned
    assert tau[3] == POS_INF and not scan[3]      # radius < 0: count 0 whatever the flags
    assert tau[4] == POS_INF and scan[4]          # a NaN bound certifies nothing


def test_in_range_selection_is_inclusive_and_drops_deleted_rows():
    d = np.array([0.0, 0.1, np.nextafter(F(0.1), POS_INF), 1.0, 0.1], F)
    rows = np.array([9, 4, 5, 6, 2], np.uint64)
    got = kr.in_range_keys(d, rows, F(0.1))
    assert list(got) == list(dist_key(F([0.0, 0.1, 0.1]), np.array([9, 2, 4], np.uint64)))
    below = np.nextafter(F(0.1), NEG_INF)
    assert list(kr.in_range_keys(d, rows, below)) == list(dist_key(F([0.0]), np.array([9], np.uint64)))
    dead = np.zeros(10, bool)
    dead[[9, 4]] = True
    assert list(kr.in_range_keys(d, rows, F(0.1), dead)) == list(dist_key(F([0.1]), np.array([2], np.uint64)))
    assert len(kr.in_range_keys(d, rows, F(-1))) == 0
    assert len(kr.in_range_keys(d, rows, F(np.nan))) == 0
    assert len(kr.in_range_keys(d, rows, POS_INF)) == 5


def test_finish_orders_by_distance_then_index_and_pads():
    keys = dist_key(F([0.5, 0.25, 0.5, 0.0]), np.array([7, 30, 3, 12], np.uint64))
    idx, dist, cnt = kr.finish_model(np.concatenate([keys, [np.uint64(123)]]), 4, 6, 1000)
    assert cnt == 4
    assert list(idx) == [1012, 1030, 1003, 1007, int(IDX_NONE), int(IDX_NONE)]
    assert list(dist[:4]) == [0.0, 0.25, 0.5, 0.5] and np.isposinf(dist[4:]).all()
    idx, dist, cnt = kr.finish_model(keys, 0, 3, 5)
    assert cnt == 0 and (idx == IDX_NONE).all() and np.isposinf(dist).all()


def test_finish_overflow_is_count_only():
    keys = dist_key(F([0.1, 0.2, 0.3]), np.array([1, 2, 3], np.uint64))
    idx, dist, cnt = kr.finish_model(keys, 3, 2, 0)
    assert cnt == 3 and (idx == IDX_NONE).all() and np.isposinf(dist).all()
    idx, dist, cnt = kr.finish_model(keys, 3, 3, 0)     # exactly full: returned
    assert cnt == 3 and list(idx) == [1, 2, 3]
    idx, dist, cnt = kr.finish_model(keys, 3000, 2, 0)  # the exact count survives, far above the list
    assert cnt == 3000 and (idx == IDX_NONE).all()


def test_range_cap_model():
    assert [kr.range_cap_model(c) for c in (1, 64, 512, 513, 1000, 4095, 4096)] == \
        [1024, 1024, 1024, 1088, 2048, 8192, 8192]


def test_pack_dead():
    dead = np.zeros(130, bool)
    dead[[0, 63, 64, 129]] = True
    w = kr.pack_dead(dead)
    assert [int(x) for x in w] == [1 | (1 << 63), 1, 1 << 1]
