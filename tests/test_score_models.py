"""Hand-derived cases that pin the models of tests/kcheck_score.py (no GPU): which slots are
present, the aligned distances, the found count, the keys, and the rerank order with a tie and a
repeated id."""
import numpy as np

import kcheck_score as ks
from kcheck_exact import IDX_NONE, dist_key

F = np.float32
INF = F(np.inf)
PAD = 2 ** 64 - 1


def test_present_rows():
    dead = np.array([False, False, True, False])
    ids = [100, 103, 104, 99, PAD, 102, 2 ** 64 - 2, 0, 101]
    present, row = ks.present_rows(ids, 100, 4, dead)
    assert present.tolist() == [True, True, False, False, False, False, False, False, True]
    assert row.tolist() == [0, 3, 0, 0, 0, 2, 0, 0, 1]  # (a deleted row keeps its row; outside: 0)
    # an offset above 2^33, ids next to the interval's two ends; an empty shard has no present slot
    off = 2 ** 33 + 5
    present, row = ks.present_rows([off - 1, off, off + 3, off + 4, 5], off, 4)
    assert present.tolist() == [False, True, True, False, False] and row.tolist() == [0, 0, 3, 0, 0]
    assert not ks.present_rows([0, 1, PAD], 0, 0)[0].any()


def test_score_model_aligned_absent_found_and_keys():
    dist_rows = F([0.5, 0.25, 1.0, 0.0])
    dead = np.array([False, False, True, False])
    ids = [13, 11, 10, PAD, 12, 11, 9, 14]
    dist, found, keys = ks.score_model(dist_rows, ids, 10, dead)
    assert dist.tolist() == [0.0, 0.25, 0.5, INF, INF, 0.25, INF, INF]
    assert found == 4, "the repeated id counts twice; the deleted row and the outsiders do not"
    want = [dist_key(F(0.0), 3), dist_key(F(0.25), 1), dist_key(F(0.25), 1), dist_key(F(0.5), 0)]
    assert keys.tolist() == [int(k) for k in want]
    # without tombstones row 2 is present too
    dist, found, _ = ks.score_model(dist_rows, ids, 10)
    assert dist[4] == 1.0 and found == 5


def test_finish_model_dedupe_tail_and_count():
    keys = np.array([dist_key(F(0.5), 7), dist_key(F(0.25), 9), dist_key(F(0.25), 2), dist_key(F(0.5), 7),
                     dist_key(F(0.0), 100), 0xDEAD], np.uint64)
    idx, dist, cnt = ks.finish_model(keys, 5, 5, 1000)  # (the sixth key lies past the count)
    assert cnt == 4
    assert idx.tolist() == [1100, 1002, 1009, 1007, int(IDX_NONE)]
    assert dist.tolist() == [0.0, 0.25, 0.25, 0.5, INF]
    idx, dist, cnt = ks.finish_model(keys, 5, 2, 1000)
    assert cnt == 2 and idx.tolist() == [1100, 1002] and dist.tolist() == [0.0, 0.25]
    idx, dist, cnt = ks.finish_model(keys, 0, 3, 0)
    assert cnt == 0 and (idx == IDX_NONE).all() and np.isposinf(dist).all()


def test_rerank_model_tie_and_duplicate():
    # ids 40 and 20 tie at 0.25 (the lower id first); id 30 twice; an absent slot in between
    ids = [40, 30, PAD, 20, 30, 50]
    dist = F([0.25, 0.75, np.inf, 0.25, 0.75, 0.125])
    oi, od, cnt = ks.rerank_model(ids, dist, 6)
    assert cnt == 4
    assert oi.tolist() == [50, 20, 40, 30, int(IDX_NONE), int(IDX_NONE)]
    assert od.tolist() == [0.125, 0.25, 0.25, 0.75, INF, INF]
    oi, od, cnt = ks.rerank_model(ids, dist, 3)
    assert cnt == 3 and oi.tolist() == [50, 20, 40]
    # the two models agree: the rerank of the score model's output is the finish of its keys
    dist_rows = F([0.5, 0.25, 1.0, 0.0, 0.25])
    lst = [13, 11, 10, PAD, 14, 11, 9, 12]
    d, _, keys = ks.score_model(dist_rows, lst, 10)
    a = ks.rerank_model(lst, d, 8)
    b = ks.finish_model(keys, len(keys), 8, 10)
    assert a[2] == b[2] == 5 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0][:5].tolist() == [13, 11, 14, 10, 12]


def test_pack_dead():
    dead = np.zeros(130, bool)
    dead[[0, 63, 64, 129]] = True
    w = ks.pack_dead(dead)
    assert w.tolist() == [1 | (1 << 63), 1, 2]
