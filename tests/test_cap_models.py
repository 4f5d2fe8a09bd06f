"""The capped search's model (tests/kcheck_cap.py), pinned by hand-worked cases in dimension 2-3 (the
distances are worked out by hand or exact by construction: identical rows give 0, orthogonal rows 1,
opposite rows 2; the kept rows and their order follow from the contract), by its two formulations
against each other, by its identities with the collapsed search's model (m = 1) and the plain top-k
(m >= k), and the simulation of the capped scan's insert cascade under random interleavings."""
import numpy as np
import pytest

import kcheck_cap as kp
import kcheck_collapse as kl
from kcheck_exact import IDX_NONE

F = np.float32
# query (1, 0); the angles grow with the row id: distances 0, 0.2, 0.4, 1
FAN = [[1, 0], [4, 3], [3, 4], [0, 1]]


def _dist(oracle_mod, rows, q):
    return oracle_mod.np_cosine_distances(np.asarray(rows, F), np.asarray(q, F))


def _check(got, idx, groups, count, k):
    gi, gd, gg, gc = got
    assert gc == count
    assert list(gi[:count]) == idx and list(gg[:count]) == groups
    assert (gi[count:] == IDX_NONE).all() and np.isposinf(gd[count:]).all() and (gg[count:] == kp.GROUP_NONE).all()
    assert len(gi) == len(gd) == len(gg) == k
    assert (np.diff(gd[:count]) >= 0).all()


def _both(d, groups, k, m, **kw):
    a = kp.cap_model(d, groups, k, m, **kw)
    b = kp.cap_model_ranked(d, groups, k, m, **kw)
    assert a[3] == b[3] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    return a


def test_two_groups_interleaved(oracle_mod):
    rows = FAN + [[-3, 4], [-1, 0]]  # two more rows: distances 1.6 and 2
    d = _dist(oracle_mod, rows, [1, 0])
    assert d[0] == 0 and d[3] == 1 and d[5] == 2 and (np.diff(d) > 0).all()
    assert abs(float(d[1]) - 0.2) < 1e-6 and abs(float(d[2]) - 0.4) < 1e-6 and abs(float(d[4]) - 1.6) < 1e-6
    g = [0, 1, 0, 1, 0, 1]
    # m = 2: two of each group, in distance order; rows 4 and 5 are third in their groups
    got = _both(d, g, 6, 2)
    _check(got, [0, 1, 2, 3], [0, 1, 0, 1], 4, 6)
    assert got[1][0] == d[0] and got[1][1].view(np.uint32) == d[1].view(np.uint32)
    # k cuts the kept rows, not the rows
    _check(_both(d, g, 3, 2), [0, 1, 2], [0, 1, 0], 3, 3)
    # m = 1: the heads; m = 3: everything
    _check(_both(d, g, 6, 1), [0, 1], [0, 1], 2, 6)
    _check(_both(d, g, 6, 3), [0, 1, 2, 3, 4, 5], g, 6, 6)
    # an offset is added to the ids, not to the groups
    _check(_both(d, g, 3, 2, offset=1000), [1000, 1001, 1002], [0, 1, 0], 3, 3)


def test_the_m_plus_first_row_lies_between_kept_rows(oracle_mod):
    # group 0 holds rows 0, 1, 2 (the three nearest), group 1 row 3, group 2 rows 4, 5: with m = 2
    # row 2 is dropped though rows farther than it are kept
    rows = FAN + [[-3, 4], [-1, 0]]
    d = _dist(oracle_mod, rows, [1, 0])
    _check(_both(d, [0, 0, 0, 1, 2, 2], 4, 2), [0, 1, 3, 4], [0, 0, 1, 2], 4, 4)
    _check(_both(d, [0, 0, 0, 1, 2, 2], 6, 2), [0, 1, 3, 4, 5], [0, 0, 1, 2, 2], 5, 6)


def test_ties_inside_a_group_and_between_groups(oracle_mod):
    # rows 1, 2, 3, 4 are the query's vector: 1, 2 and 4 in group 0, row 3 in group 1; row 0 is
    # farther.  Ties go to the smaller index, so group 0 keeps rows 1 and 2 (not 4) at m = 2.
    rows = [[0, 1, 0], [1, 1, 0], [1, 1, 0], [1, 1, 0], [1, 1, 0]]
    d = _dist(oracle_mod, rows, [1, 1, 0])
    assert d[1] == d[2] == d[3] == d[4] == 0 and d[0] > 0
    _check(_both(d, [2, 0, 0, 1, 0], 5, 2), [1, 2, 3, 0], [0, 0, 1, 2], 4, 5)
    _check(_both(d, [2, 0, 0, 1, 0], 2, 1), [1, 3], [0, 1], 2, 2)
    _check(_both(d, [2, 0, 0, 1, 0], 5, 3), [1, 2, 3, 4, 0], [0, 0, 1, 0, 2], 5, 5)


def test_fewer_keepable_rows_than_k(oracle_mod):
    d = _dist(oracle_mod, FAN, [1, 0])
    # groups 5 and 9 of n_groups = 10 (the ids need not be dense): min(2, 3) + min(2, 1) rows
    _check(_both(d, [5, 5, 5, 9], 4, 2), [0, 1, 3], [5, 5, 9], 3, 4)
    # all rows in one group: the top-min(m, k)
    _check(_both(d, [0, 0, 0, 0], 4, 3), [0, 1, 2], [0, 0, 0], 3, 4)
    _check(_both(d, [0, 0, 0, 0], 2, 3), [0, 1], [0, 0], 2, 2)


def test_deleted_kept_row(oracle_mod):
    d = _dist(oracle_mod, FAN, [1, 0])
    # group 0 = rows 0, 1, 2: with row 1 deleted, row 2 takes its place among the two kept
    _check(_both(d, [0, 0, 0, 1], 4, 2, live=[True, False, True, True]), [0, 2, 3], [0, 0, 1], 3, 4)
    _check(_both(d, [0, 0, 0, 1], 4, 2, live=[False, False, False, True]), [3], [1], 1, 4)


def test_mask_removes_a_group(oracle_mod):
    d = _dist(oracle_mod, FAN, [1, 0])
    _check(_both(d, [0, 1, 0, 1], 4, 2, allowed=[False, True, False, True]), [1, 3], [1, 1], 2, 4)
    # the mask and the tombstones combine
    _check(_both(d, [0, 1, 0, 1], 4, 1, live=[True, False, True, True], allowed=[True, True, False, True]),
           [0, 3], [0, 1], 2, 4)
    _check(_both(d, [0, 1, 0, 1], 2, 2, allowed=np.zeros(4, bool)), [], [], 0, 2)


def test_identities_and_batch(oracle_mod):
    rng = np.random.default_rng(20)
    rows = rng.uniform(-1, 1, (60, 3)).astype(F)
    rows[10:20] = rows[10]  # (a run of ties)
    qs = rng.uniform(-1, 1, (4, 3)).astype(F)
    dists = [_dist(oracle_mod, rows, q) for q in qs]
    live = rng.random(60) < 0.8
    masks = rng.random((4, 60)) < 0.6
    for rg in (np.arange(60) // 5, np.arange(60) % 3, np.zeros(60, np.int64), rng.integers(0, 7, 60)):
        for q in range(4):
            for k in (1, 4, 11):
                # m = 1: the collapsed search's model
                a = _both(dists[q], rg, k, 1, live=live, allowed=masks[q], offset=77)
                b = kl.collapse_model(dists[q], rg, k, live=live, allowed=masks[q], offset=77)
                assert a[3] == b[3] and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
                # m >= k: the plain top-k
                for m in (k, k + 1, 16):
                    wi, wd = oracle_mod.np_top_k(rows, qs[q], k)
                    gi, gd, gg, gc = _both(dists[q], rg, k, m)
                    assert gc == k and np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))
                    assert np.array_equal(gg, rg[wi.astype(np.int64)].astype(np.uint32))
                for m in (2, 3):
                    gi, gd, gg, gc = _both(dists[q], rg, k, m, live=live, allowed=masks[q])
                    ok = live & masks[q]
                    assert gc == min(k, sum(min(m, int(c)) for c in np.bincount(rg[ok])))
                    assert ok[gi[:gc].astype(np.int64)].all() and np.bincount(gg[:gc]).max(initial=0) <= m
    idx, dist, cnt, grp = kp.cap_batch(dists, np.arange(60) // 5, 10, 2, allowed=masks)
    for q in range(4):
        one = kp.cap_model(dists[q], np.arange(60) // 5, 10, 2, allowed=masks[q])
        assert np.array_equal(idx[q], one[0]) and cnt[q] == one[3] and np.array_equal(grp[q], one[2])


def test_merge_model_by_hand():
    # two lists of one query; index 7 is listed twice; group 1 is full after rows 3 and 7
    idx = np.array([[3, 7, 9], [7, 4, 8]], np.uint64)
    dist = np.array([[0.1, 0.2, 0.5], [0.2, 0.3, 0.4]], F)
    grp = np.array([[1, 1, 2], [1, 1, 2]], np.uint32)
    oi, od, og, c = kp.merge_model(idx, dist, grp, [3, 3], 4, 2)
    assert c == 4 and list(oi) == [3, 7, 8, 9] and list(og) == [1, 1, 2, 2]
    oi, od, og, c = kp.merge_model(idx, dist, grp, [3, 1], 4, 1)  # (a short second list: only its first entry)
    assert c == 2 and list(oi[:2]) == [3, 9] and oi[2] == IDX_NONE and np.isposinf(od[2]) and og[3] == kp.GROUP_NONE


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6])
def test_cascade_keeps_the_m_smallest(m):
    """cap_insert's steps under random interleavings: the entries end as the m smallest keys."""
    rng = np.random.default_rng(1000 + m)
    trials = 3400  # (6 values of m: 20400 trials)
    for _ in range(trials):
        n = int(rng.integers(0, 15))
        keys = rng.choice(1000, n, replace=False)  # (keys are distinct: a row is inserted once)
        want = sorted(keys.tolist())[:m] + [int(kp.KEY_NONE)] * max(0, m - n)
        assert kp.cascade_sim(keys, m, rng) == want, (m, keys)
