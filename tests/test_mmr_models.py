"""The MMR model (tests/kcheck_mmr.py) pinned by hand-derived cases, without a GPU.  Every expected
value below is worked out from the contract in include/bsr.h with explicit f32 operations -- none
comes from the model."""
import numpy as np

import kcheck_mmr as km

F = np.float32
ONE = F(1.0)


def f32(x):
    return F(x)


def test_pair_distance_identical_and_zero_rows(oracle_mod):
    # identical rows: the max |a - b| <= 1e-10 shortcut gives exactly 0, where the quotient would
    # not (sqrt(14) * sqrt(14) rounds to 14.000001 in f32, so 1 - 14 / that is 6e-8)
    rows = np.array([[1, 2, 3], [1, 2, 3], [3, 2, 1]], F)
    d = km.pair_distances(rows, 0)
    assert d[0] == 0.0 and d[1] == 0.0 and d[2] > 0
    n14 = np.sqrt(F(14.0))
    assert ONE - F(14.0) / F(n14 * n14) == F(2.0 ** -24)
    # a zero row: magnitude 0 gives exactly 1 to every other row, 0 to itself (identical)
    rows = np.array([[0, 0, 0], [1, 2, 3], [0, 0, 0]], F)
    assert list(km.pair_distances(rows, 0)) == [0.0, 1.0, 0.0]
    assert list(km.pair_distances(rows, 1)) == [1.0, 0.0, 1.0]


# Dimension 2.  Positions: 0 (1,0)  1 (1,0)  2 (3,4)  3 (0,1); dq = 0, 0, 0.25, 0.5.
# |(3,4)| = 5 exactly.  D(0,1) = 0 (identical); D(0,2) = 1 - 3/5; D(0,3) = 1 (dot 0);
# D(3,1) = 1; D(3,2) = 1 - 4/5; D(2,1) = D(2,0).
ROWS2 = np.array([[1, 0], [1, 0], [3, 4], [0, 1]], F)
DQ2 = np.array([0.0, 0.0, 0.25, 0.5], F)
D02 = ONE - F(3.0) / F(5.0)   # 0.39999998
D32 = ONE - F(4.0) / F(5.0)   # 0.19999999


def test_dim2_pair_distances(oracle_mod):
    assert list(km.pair_distances(ROWS2, 0)) == [0.0, 0.0, D02, 1.0]
    assert list(km.pair_distances(ROWS2, 3)) == [1.0, 1.0, D32, 0.0]
    # symmetric bit for bit
    for i in range(4):
        for j in range(4):
            assert km.pair_distances(ROWS2, i)[j].view(np.uint32) == km.pair_distances(ROWS2, j)[i].view(np.uint32)


def test_dim2_lambda_half(oracle_mod):
    # mu = lam = 0.5.  Pick 1 (after position 0): scores 1: 0.5*0 - 0 = 0; 2: 0.5*D02 - 0.125 =
    # 0.07499999; 3: 0.5*1 - 0.25 = 0.25 -> position 3.  Pick 2: mind_1 = min(0, 1) = 0 -> 0;
    # mind_2 = min(D02, D32) = D32 -> 0.5*D32 - 0.125 = -0.025 -> position 1.  Then position 2.
    picks, scores = km.mmr_model(ROWS2, DQ2, 4, 0.5)
    assert picks == [0, 3, 1, 2]
    assert np.isnan(scores[0])
    assert scores[1] == F(0.25)
    assert scores[2] == F(0.0) and not np.signbit(scores[2])
    assert scores[3] == F(F(0.5) * D32) - F(0.125) and scores[3] < 0
    # k cuts the same sequence
    assert km.mmr_model(ROWS2, DQ2, 2, 0.5)[0] == [0, 3]


def test_lambda_one_is_identity(oracle_mod):
    # mu = 0: score = (0 * mind) - dq = -dq: the list order, ties (positions 0 and 1) by position
    assert km.mmr_model(ROWS2, DQ2, 4, 1.0)[0] == [0, 1, 2, 3]
    assert km.mmr_model(ROWS2, DQ2, 3, 1.0)[0] == [0, 1, 2]


def test_lambda_zero_is_farthest_first(oracle_mod):
    # mu = 1, lam = 0: score = mind.  After 0: mind = (., 0, D02, 1) -> 3; then (., 0, D32, .) -> 2;
    # the duplicate of position 0 comes last
    picks, scores = km.mmr_model(ROWS2, DQ2, 4, 0.0)
    assert picks == [0, 3, 2, 1]
    assert scores[1:] == [F(1.0), D32, F(0.0)]


def test_score_tie_goes_to_the_lower_position(oracle_mod):
    # positions 1 and 2 hold (0,1) and (0,-1): D to (1,0) is 1 for both, dq equal: both score
    # 0.5*1 - 0.25 = 0.25; position 1 wins.  Then mind_2 = min(1, D((0,-1),(0,1)) = 2) = 1 again.
    rows = np.array([[1, 0], [0, 1], [0, -1]], F)
    dq = np.array([0.0, 0.5, 0.5], F)
    picks, scores = km.mmr_model(rows, dq, 3, 0.5)
    assert picks == [0, 1, 2] and scores[1] == F(0.25) and scores[2] == F(0.25)
    # two mutually identical rows with equal dq tie as well; the second then drops (mind = 0)
    rows = np.array([[1, 0], [0, 1], [0, 1], [1, 1]], F)
    dq = np.array([0.0, 0.5, 0.5, 0.6], F)
    picks, scores = km.mmr_model(rows, dq, 4, 0.5)
    assert picks[:2] == [0, 1]
    # position 2: 0.5*0 - 0.25 = -0.25; position 3: 0.5*min(D(3,0), D(3,1)) - 0.3 with
    # D = 1 - 1/(sqrt(2)) = 0.29289323 -> -0.15355338: position 3 first
    assert picks[2:] == [3, 2] and scores[3] == F(-0.25)


def test_dim3_lambda_03(oracle_mod):
    # rows of magnitude 3: (1,2,2), (2,1,2), (2,-2,1); dots 01 = 8, 02 = 0, 12 = 4
    rows = np.array([[1, 2, 2], [2, 1, 2], [2, -2, 1]], F)
    dq = np.array([0.1, 0.2, 0.3], F)
    d01 = ONE - F(8.0) / F(9.0)
    d12 = ONE - F(4.0) / F(9.0)
    assert list(km.pair_distances(rows, 0)) == [0.0, d01, 1.0]
    assert list(km.pair_distances(rows, 2)) == [1.0, d12, 0.0]
    lam = F(0.3)
    mu = ONE - lam
    # pick 1: position 1 scores mu*d01 - lam*0.2 = 0.018, position 2 mu*1 - lam*0.3 = 0.61
    s2 = F(mu * ONE) - F(lam * F(0.3))
    # pick 2: mind_1 = min(d01, d12) = d01
    s1 = F(mu * d01) - F(lam * F(0.2))
    picks, scores = km.mmr_model(rows, dq, 3, 0.3)
    assert picks == [0, 2, 1]
    assert scores[1].view(np.uint32) == F(s2).view(np.uint32)
    assert scores[2].view(np.uint32) == F(s1).view(np.uint32)


def test_fewer_candidates_than_k_and_none(oracle_mod):
    picks, _ = km.mmr_model(ROWS2[:2], DQ2[:2], 5, 0.5)
    assert picks == [0, 1]
    idx, dist, rank, c = km.mmr_outputs(picks, [40, 41], DQ2[:2], 5)
    assert c == 2 and list(idx) == [40, 41] + [km.IDX_NONE] * 3
    assert list(dist[:2]) == [0.0, 0.0] and np.isposinf(dist[2:]).all()
    assert list(rank) == [0, 1] + [km.RANK_NONE] * 3
    picks, scores = km.mmr_model(np.zeros((0, 2), F), np.zeros(0, F), 3, 0.5)
    assert picks == [] and scores == []
    idx, dist, rank, c = km.mmr_outputs(picks, [], [], 3)
    assert c == 0 and (idx == km.IDX_NONE).all() and np.isposinf(dist).all() and (rank == km.RANK_NONE).all()


def test_outputs_carry_ids_dq_and_positions(oracle_mod):
    picks, _ = km.mmr_model(ROWS2, DQ2, 3, 0.5)
    idx, dist, rank, c = km.mmr_outputs(picks, [100, 101, 102, 103], DQ2, 3)
    assert c == 3 and list(idx) == [100, 103, 101] and list(dist) == [0.0, 0.5, 0.0] and list(rank) == [0, 3, 1]
