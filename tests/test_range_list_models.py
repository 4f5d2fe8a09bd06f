"""The numpy models of tests/kcheck_range_list.py pinned by hand-derived cases (CPU): the GPU tests
compare the kernels with these models, so the models themselves are checked here."""
import numpy as np

import kcheck_range_list as kl

INF = np.float32(np.inf)


def test_route_model():
    #            0: filters   1: listed already  2: radius < 0  3: NaN    4: not routed  5: filters, radius 0
    radius = np.array([0.1, 1.5, -1.0, np.nan, 0.2, 0.0], np.float32)
    tau = np.array([0.8, INF, INF, INF, 0.7, 0.9], np.float32)
    to_list = [1, 1, 1, 1, 0, 1]
    t, on, fail, fail2 = kl.route_model(to_list, radius, tau, {1}, 1)
    assert list(t) == [INF, INF, INF, INF, np.float32(0.7), INF]
    assert on == {0, 1, 5} and fail == 3 and fail2 == 3
    # nothing routed: nothing changes
    t, on, fail, fail2 = kl.route_model([0] * 6, radius, tau, {1}, 1)
    assert np.array_equal(t, tau) and on == {1} and (fail, fail2) == (1, 1)


def test_seg_model():
    mask = np.array([1, 0, 1, 1, 0, 1, 1, 1], bool)
    dead = np.array([0, 0, 0, 1, 0, 0, 0, 0], bool)
    # the allowed live rows: 0, 2, 5, 6, 7
    assert list(kl.seg_model(mask, dead, 0, 5)) == [0, 2, 5, 6, 7]
    assert list(kl.seg_model(mask, dead, 1, 2)) == [2, 5]
    assert list(kl.seg_model(mask, dead, 4, 3)) == [7]      # fewer left than asked for
    assert list(kl.seg_model(mask, dead, 2, 0)) == []
    assert list(kl.seg_model(mask, np.zeros(8, bool), 2, 2)) == [3, 5]
    assert kl.SEG_DESC.itemsize == 24 and kl.SEG_DESC.names == ("off", "mask", "first", "n_list", "pad_")
