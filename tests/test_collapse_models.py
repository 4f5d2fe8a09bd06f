"""The collapsed search's model (tests/kcheck_collapse.py), pinned by hand-worked cases in dimension
2-3: the distances below are worked out by hand (or are exact by construction: identical rows give
0, orthogonal rows 1, opposite rows 2), the heads and their order follow from the contract."""
import numpy as np

import kcheck_collapse as kl
from kcheck_exact import IDX_NONE

F = np.float32


def _dist(oracle_mod, rows, q):
    return oracle_mod.np_cosine_distances(np.asarray(rows, F), np.asarray(q, F))


def _check(got, idx, groups, count, k):
    gi, gd, gg, gc = got
    assert gc == count
    assert list(gi[:count]) == idx and list(gg[:count]) == groups
    assert (gi[count:] == IDX_NONE).all() and np.isposinf(gd[count:]).all() and (gg[count:] == kl.GROUP_NONE).all()
    assert len(gi) == len(gd) == len(gg) == k
    assert (np.diff(gd[:count]) >= 0).all()


def test_two_groups_interleaved(oracle_mod):
    # query (1, 0); the angles grow with the row id, the groups alternate: 0 1 0 1
    rows = [[1, 0], [4, 3], [3, 4], [0, 1]]
    d = _dist(oracle_mod, rows, [1, 0])
    assert d[0] == 0 and d[3] == 1 and d[0] < d[1] < d[2] < d[3]
    assert abs(float(d[1]) - 0.2) < 1e-6 and abs(float(d[2]) - 0.4) < 1e-6  # 1 - 4/5, 1 - 3/5
    got = kl.collapse_model(d, [0, 1, 0, 1], 2)
    _check(got, [0, 1], [0, 1], 2, 2)
    assert got[1][0] == d[0] and got[1][1].view(np.uint32) == d[1].view(np.uint32)
    # with the groups swapped on the first two rows the heads are the same rows, the groups swap
    _check(kl.collapse_model(d, [1, 0, 0, 1], 2), [0, 1], [1, 0], 2, 2)
    # k = 1: the top-1
    _check(kl.collapse_model(d, [0, 1, 0, 1], 1), [0], [0], 1, 1)
    # an offset is added to the ids, not to the groups
    _check(kl.collapse_model(d, [0, 1, 0, 1], 2, offset=1000), [1000, 1001], [0, 1], 2, 2)


def test_ties_go_to_the_smaller_index(oracle_mod):
    # rows 1 and 3 are the same vector in two groups (a tie between heads); rows 1 and 2 the same
    # vector in one group (a tie within a group); row 0 is farther than all of them
    rows = [[0, 1, 0], [1, 1, 0], [1, 1, 0], [1, 1, 0], [2, 2, 0]]
    d = _dist(oracle_mod, rows, [1, 1, 0])
    assert d[1] == d[2] == d[3] == 0 and d[0] > 0
    got = kl.collapse_model(d, [2, 0, 0, 1, 1], 3)
    # group 0's head is row 1 (not row 2); group 1's head is row 3 (distance 0, before row 4); heads
    # 1 and 3 tie at distance 0 and the smaller index comes first; group 2's head is row 0
    _check(got, [1, 3, 0], [0, 1, 2], 3, 3)
    # (2, 2, 0) is parallel to the query but not identical: its distance may be a rounding away from 0
    assert d[4] >= 0 and d[4] < 1e-6


def test_one_group_only(oracle_mod):
    rows = [[0, 1], [1, 0], [1, 1]]
    d = _dist(oracle_mod, rows, [1, 0])
    _check(kl.collapse_model(d, [0, 0, 0], 3), [1], [0], 1, 3)


def test_fewer_groups_than_k(oracle_mod):
    rows = [[0, 1], [1, 0], [1, 1], [-1, 0]]
    d = _dist(oracle_mod, rows, [1, 0])
    assert d[3] == 2
    # groups 5 and 9 of n_groups = 10: the ids need not be dense
    _check(kl.collapse_model(d, [5, 5, 9, 9], 4), [1, 2], [5, 9], 2, 4)


def test_deleted_head(oracle_mod):
    rows = [[1, 0], [4, 3], [3, 4], [0, 1]]
    d = _dist(oracle_mod, rows, [1, 0])
    live = np.array([False, True, True, True])
    # group 0 = rows 0 and 2: with row 0 deleted its head is row 2, behind group 1's row 1
    _check(kl.collapse_model(d, [0, 1, 0, 1], 2, live=live), [1, 2], [1, 0], 2, 2)
    # every row of group 0 deleted: one group is left
    _check(kl.collapse_model(d, [0, 1, 0, 1], 2, live=[False, True, False, True]), [1], [1], 1, 2)


def test_mask_removes_a_whole_group(oracle_mod):
    rows = [[1, 0], [4, 3], [3, 4], [0, 1]]
    d = _dist(oracle_mod, rows, [1, 0])
    allowed = np.array([False, True, False, True])
    _check(kl.collapse_model(d, [0, 1, 0, 1], 2, allowed=allowed), [1], [1], 1, 2)
    # the mask and the tombstones combine
    _check(kl.collapse_model(d, [0, 1, 0, 1], 2, live=[True, False, True, True], allowed=[True, True, False, True]),
           [0, 3], [0, 1], 2, 2)
    # nothing allowed: no result
    _check(kl.collapse_model(d, [0, 1, 0, 1], 2, allowed=np.zeros(4, bool)), [], [], 0, 2)


def test_identity_and_batch(oracle_mod):
    rng = np.random.default_rng(5)
    rows = rng.uniform(-1, 1, (50, 3)).astype(F)
    qs = rng.uniform(-1, 1, (4, 3)).astype(F)
    dists = [_dist(oracle_mod, rows, q) for q in qs]
    # every row its own group: the plain top-k
    idx, dist, cnt, grp = kl.collapse_batch(dists, np.arange(50), 7)
    for q in range(4):
        wi, wd = oracle_mod.np_top_k(rows, qs[q], 7)
        assert np.array_equal(idx[q], wi) and np.array_equal(dist[q].view(np.uint32), wd.view(np.uint32))
        assert np.array_equal(grp[q], wi.astype(np.uint32)) and cnt[q] == 7
    # a mask per query
    masks = rng.random((4, 50)) < 0.5
    idx, dist, cnt, grp = kl.collapse_batch(dists, np.arange(50) // 5, 10, allowed=masks)
    for q in range(4):
        one = kl.collapse_model(dists[q], np.arange(50) // 5, 10, allowed=masks[q])
        assert np.array_equal(idx[q], one[0]) and cnt[q] == one[3]
        assert masks[q][idx[q][:cnt[q]].astype(np.int64)].all()
        assert len(set(grp[q][:cnt[q]].tolist())) == cnt[q]
