"""The models of tests/kcheck_exact.py, pinned by hand-derived cases (no GPU): the kernel-level tests
of the exact stage compare the kernels with these models, so each must be right on its own."""
from fractions import Fraction

import numpy as np

import kcheck as kc
import kcheck_exact as kx

F = Fraction
KN = kx.KEY_NONE


def f32(x):
    return np.float32(x)


def below(x):
    return np.nextafter(f32(x), kx.NEG_INF)


def above(x):
    return np.nextafter(f32(x), kx.POS_INF)


# ---- the distance -------------------------------------------------------------------------
def test_exact_distance_is_the_oracles(oracle_mod):
    rng = np.random.default_rng(11)
    for dim in (1, 5, 64, 130):
        rows = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
        q = rng.uniform(-1, 1, dim).astype(np.float32)
        rows[3] = q
        rows[4] = 0
        rows[5] = -q
        rows[6] = q
        rows[6, 0] += f32(1e-3)
        na, nb = kc.seq_norm_f32(rows), kc.seq_norm_f32(q[None, :])[0]
        d = kx.exact_distance(rows, q, na, nb)
        want = oracle_mod.np_cosine_distances(rows, q)
        assert np.array_equal(d.view(np.uint32), want.view(np.uint32))
        for r in range(len(rows)):
            c = f32(oracle_mod.cosine_distance(rows[r], q))
            assert d[r].view(np.uint32) == c.view(np.uint32), (dim, r)
        assert d[3] == 0 and d[4] == 1 and d[5] == 2 and d[6] < 1e-3


def test_exact_distance_by_hand():
    # a = (3, 4, 0, 0), b = (4, 3, 0, 0): products 12, 12, 0, 0 -> dot 24 (exact); |a| = |b| = 5,
    # s = fl32(24 / 25), d = 1 - s exactly (Sterbenz: s in [1/2, 2]).
    a = np.array([[3, 4, 0, 0]], np.float32)
    b = np.array([4, 3, 0, 0], np.float32)
    d = kx.exact_distance(a, b, [5], 5)
    s = f32(0.96)  # the f32 nearest 24/25
    assert abs(F(float(s)) - F(24, 25)) <= F(1, 2 ** 25)  # within half an ulp (2^-24) of 24/25
    assert F(float(d[0])) == 1 - F(float(s))
    # the magnitudes are inputs: with |a| = 8, |b| = 4 the cosine is 24 / 32 = 3/4 exactly
    d2 = kx.exact_distance(a, b, [8], 4)
    assert d2[0] == f32(0.25)
    # a zero magnitude (given!) -> 1; identical within 1e-10 -> 0 whatever the magnitudes; a - b = 2e-10 is not
    assert kx.exact_distance(a, b, [0], 5)[0] == 1 and kx.exact_distance(a, b, [5], 0)[0] == 1
    t = np.array([[1e-9, 0.5, 0, 0]], np.float32)
    u = t[0].copy()
    assert kx.exact_distance(t, u, [0], 0)[0] == 0
    u[0] = f32(1e-9) + f32(5e-11)
    assert kx.exact_distance(t, u, [1], 1)[0] == 0
    u[0] = f32(1e-9) + f32(2e-10)
    assert kx.exact_distance(t, u, [1], 1)[0] == f32(0.75)  # (not identical: 1 - 0.25 / (1 * 1))
    # the sum is sequential: (2^24 + 1) + 1 in f32 is 2^24 + 2 only if the ones are added first
    a3 = np.array([[1, 1, 2 ** 24, 0]], np.float32)
    one = np.ones(4, np.float32)
    assert kx.exact_distance(a3, one, [1], [2.0 ** 25][0])[0] == 1 - f32((2 ** 24 + 2) / 2 ** 25)
    a4 = np.array([[2 ** 24, 1, 1, 0]], np.float32)  # 2^24 + 1 -> 2^24 (tie to even), twice
    assert kx.exact_distance(a4, one, [1], 2.0 ** 25)[0] == 1 - f32(2 ** 24 / 2 ** 25)
    # clamps: a dot above |a||b| gives 0, below -|a||b| gives 2
    assert kx.exact_distance(a, b, [1], 1)[0] == 0 and kx.exact_distance(a, -b, [1], 1)[0] == 2


def test_keys():
    d = np.array([0.0, 0.25, 0.25, 2.0], np.float32)
    k = kx.dist_key(d, [9, 4, 3, 0])
    assert k[0] == 9 and k[1] == (0x3E800000 << 32) | 4 and k[3] == 0x40000000 << 32
    assert np.array_equal(kx.key_dist(k).view(np.uint32), d.view(np.uint32))
    assert np.sort(k).tolist() == [k[0], k[2], k[1], k[3]]  # distance, then row
    got = kx.topk_keys([k[3], KN, k[1], k[2]], 2)
    assert got.tolist() == [k[2], k[1]]
    assert kx.topk_keys([k[3], KN], 3).tolist() == [k[3], KN, KN]


# ---- certification ------------------------------------------------------------------------
C2 = F(2.5e-7)   # the constants as the double the compiler reads
C3a, C3b = F(1e-4), F(6e-9)


def _kth(d):
    return kx.dist_key(f32(d), 17)


def test_certify_special_cases():
    assert kx.certify(kx.NEG_INF, KN, 0.5, 1.0)          # every row was a candidate: even an empty list
    assert kx.certify(kx.NEG_INF, _kth(1.5), np.nan, 0.0)
    assert not kx.certify(kx.POS_INF, _kth(0.0), 0.0, 1.0)
    assert not kx.certify(np.nan, _kth(0.0), 0.0, 1.0)
    assert not kx.certify(-0.5, KN, 0.0, 1.0)            # a finite bound, fewer than k keys
    assert not kx.certify(-0.5, _kth(0.0), np.nan, 1.0)
    assert not kx.certify(-0.5, _kth(0.0), 0.0, 0.0)     # 6e-9 / 0 = inf
    assert kx.certify(-0.5, _kth(0.0), 0.0, 1.0)


def test_certify_first_condition_ebound_below_one():
    # tx = -0.5: third condition -0.5 < 1 - E - 1e-4 - 6e-9 holds for E <= 1; second: dk = 0.25 < 1.5 - E - 2.5e-7
    e_in, e_out = below(1.0), f32(1.0)
    assert F(float(e_in)) < 1 and F(-0.5) < 1 - F(float(e_in)) - C3a - C3b and F(0.25) < F(1.5) - F(float(e_in)) - C2
    assert kx.certify(-0.5, _kth(0.25), e_in, 1.0)
    assert F(-0.5) < 1 - F(float(e_out)) - C3a - C3b and F(0.25) < F(1.5) - F(float(e_out)) - C2  # only E < 1 fails
    assert not kx.certify(-0.5, _kth(0.25), e_out, 1.0)


def test_certify_second_condition_strictly_below():
    # tx = 0.25, E = 2^-10: the bound is 3/4 - 2^-10 - 2.5e-7; its f32 neighbours differ by 6e-8 >> the
    # 1e-16 a double rounding could move it
    tx, E = f32(0.25), f32(2.0 ** -10)
    bound = F(3, 4) - F(1, 1024) - C2
    lo, c, hi1, hi2 = kx.f32_neighbours(float(bound))
    assert F(float(lo)) < F(float(c)) <= bound < F(float(hi1)) < F(float(hi2))
    assert bound - F(float(c)) > F(1, 10 ** 12) and F(float(hi1)) - bound > F(1, 10 ** 12)  # no near-tie
    assert F(float(tx)) < 1 - F(float(E)) - C3a - C3b
    assert kx.certify(tx, _kth(lo), E, 1.0) and kx.certify(tx, _kth(c), E, 1.0)
    assert not kx.certify(tx, _kth(hi1), E, 1.0) and not kx.certify(tx, _kth(hi2), E, 1.0)
    # equality is no certification.  With tx = -2^60 every other term is below half an ulp of 1 - tx, so
    # the bound is 2^60 exactly, an f32: a k-th "distance" of 2^60 is not below it, the f32 before it is
    big = f32(2.0 ** 60)
    assert float(((1.0 - float(-big)) - 0.0) - 2.5e-7) == 2.0 ** 60
    assert not kx.certify(-big, _kth(big), 0.0, 1.0) and kx.certify(-big, _kth(below(big)), 0.0, 1.0)


def test_certify_third_condition_identical_rows():
    # dk = 0 (a row identical to the query in the list), so only tx < 1 - E - 1e-4 - 6e-9 / |b| decides
    for nb, E in ((f32(1.0), f32(1e-3)), (f32(1e-6), f32(0.02)), (f32(1.0), f32(0.0))):
        bound = 1 - F(float(E)) - C3a - C3b / F(float(nb))
        lo, c, hi1, hi2 = kx.f32_neighbours(float(bound))
        assert F(float(c)) <= bound < F(float(hi1))
        assert min(bound - F(float(c)), F(float(hi1)) - bound) > F(1, 10 ** 12) or F(float(c)) == bound
        for tx, want in ((lo, True), (c, F(float(c)) < bound), (hi1, False), (hi2, False)):
            assert F(0) < 1 - F(float(tx)) - F(float(E)) - C2  # the second condition holds throughout
            assert kx.certify(tx, _kth(0.0), E, nb) == want, (nb, E, tx)
            assert (kx.exclusion_bound(tx, E, nb) != kx.NEG_INF) == want


def test_exclusion_bound_rounds_down():
    assert kx.exclusion_bound(kx.NEG_INF, np.nan, 0.0) == kx.POS_INF
    for tx, E in ((kx.POS_INF, 0.0), (np.nan, 0.0), (0.0, 1.0), (0.0, np.nan), (0.001, 0.999), (0.99991, 0.0)):
        assert kx.exclusion_bound(tx, E, 1.0) == kx.NEG_INF, (tx, E)
    ups = 0
    for i in range(-60, 60):
        tx, E = f32(i / 64.0 + 1e-3), f32(0.02)
        x = 1 - F(float(tx)) - F(float(E)) - C2  # (the double expression is within 2e-16 of this)
        if not F(float(tx)) < 1 - F(float(E)) - C3a - C3b:
            continue
        b = kx.exclusion_bound(tx, E, 1.0)
        assert b.dtype == np.float32
        assert F(float(b)) <= x + F(1, 10 ** 15) and F(float(above(b))) > x - F(1, 10 ** 15), (tx, b)
        ups += F(float(f32(float(x)))) > x  # round-to-nearest would have gone above
        # certify() agrees: a k-th distance at the bound or below certifies, the next f32 does not
        assert kx.certify(tx, _kth(b), E, 1.0) == (F(float(b)) < x)
        assert not kx.certify(tx, _kth(above(b)), E, 1.0)
    assert ups >= 20


# ---- selections ---------------------------------------------------------------------------
def _sk(score, row):
    return int(kc.score_key(f32(score), np.uint64(row)))


def test_select_kp_by_hand():
    # a dozen keys, scores descending = keys ascending; the 0.5s tie across the 4th place (kp = 3)
    sc = [0.9, 0.1, 0.5, 0.5, 0.7, 0.5, -0.2, 0.0, 0.3, 0.5, -0.0, 0.8]
    keys = np.array([_sk(s, 100 + i) for i, s in enumerate(sc)], np.uint64)
    rows, tx = kx.select_kp(keys, 12, 16, 3, -1.0)
    assert rows.tolist() == [100, 104, 111] and tx == f32(0.5)   # 0.9, 0.7, 0.8; the 4th score is 0.5
    rows, tx = kx.select_kp(keys, 12, 16, 5, -1.0)               # two of the 0.5s: the lowest rows
    assert rows.tolist() == [100, 102, 103, 104, 111] and tx == f32(0.5)
    rows, tx = kx.select_kp(keys, 12, 16, 12, -1.0)
    assert rows.tolist() == list(range(100, 112)) and tx == f32(-1.0)
    rows, tx = kx.select_kp(keys, 5, 16, 3, -1.0)                # only the first cnt slots count
    assert rows.tolist() == [100, 102, 104] and tx == f32(0.5)
    rows, tx = kx.select_kp(keys, 17, 16, 3, -1.0)               # overflowed
    assert len(rows) == 0 and tx == kx.POS_INF
    rows, tx = kx.select_kp(keys, 0, 16, 3, -0.25)
    assert len(rows) == 0 and tx == f32(-0.25)
    # +0.0 scores above -0.0
    z = np.array([_sk(-0.0, 1), _sk(0.0, 2)], np.uint64)
    rows, tx = kx.select_kp(z, 2, 16, 1, -1.0)
    assert rows.tolist() == [2] and np.signbit(tx)


def test_top_select_by_hand():
    # three 4-lists (ascending keys = descending scores)
    L = [[_sk(0.9, 1), _sk(0.8, 2), _sk(0.7, 3), _sk(0.6, 4)],
         [_sk(0.95, 5), _sk(0.5, 6), _sk(0.4, 7), _sk(0.3, 8)],
         [_sk(0.65, 9), _sk(0.62, 10), int(KN), int(KN)]]
    lists = np.array(sum(L, []) + [0xDEAD] * 4, np.uint64)  # (a slot past the 4 * top_w: untouched)
    r = kx.top_select(lists, 3, 2)
    # X = the best 4th key: score 0.6 (row 4); every row outside the lists scores <= 0.6
    assert r["top_tau"] == f32(0.6)
    # the keys above X, in slot order, at the front
    front = [L[0][0], L[0][1], L[0][2], L[1][0], L[2][0], L[2][1]]
    assert r["top_cnt"] == 6 and r["list"][:6].tolist() == front
    assert r["list"][6:].tolist() == lists[6:].tolist()
    # kp = 2: candidates 0.95, 0.9; the third score 0.8 > 0.6
    assert sorted(r["rows"].tolist()) == [1, 5] and r["tx"] == f32(0.8)
    # kp = 7: candidates down to 0.6; the 8th score is 0.5 < top_tau -> tx = top_tau
    r = kx.top_select(lists, 3, 7)
    assert sorted(r["rows"].tolist()) == [1, 2, 3, 4, 5, 9, 10] and r["tx"] == f32(0.6)
    # kp = 10 = every valid key: tx = top_tau
    r = kx.top_select(lists, 3, 10)
    assert len(r["rows"]) == 10 and r["tx"] == f32(0.6)
    # no list has a 4th key: nothing was left out
    short = lists.copy()
    short[[3, 7]] = KN
    r = kx.top_select(short, 3, 2)
    assert r["top_tau"] == kx.NEG_INF and r["top_cnt"] == 8 and r["tx"] == f32(0.8)
    assert r["list"][:8].tolist() == [k for k in short[:12].tolist() if k != int(KN)]
    r = kx.top_select(short, 3, 8)
    assert len(r["rows"]) == 8 and r["tx"] == kx.NEG_INF
    # unserved
    r = kx.top_select(lists, 3, 2, served=False)
    assert len(r["rows"]) == 0 and r["tx"] == kx.POS_INF and r["top_tau"] == kx.POS_INF and r["top_cnt"] == 0
    assert r["list"].tolist() == lists.tolist()


def test_merge_certify_branches():
    inf = kx.POS_INF
    assert kx.merge_certify(3, 0.5, [above(0.5), inf], 3, 3)
    assert not kx.merge_certify(3, 0.5, [f32(0.5), inf], 3, 3)          # equal: not strictly below
    assert not kx.merge_certify(3, 0.5, [below(0.5), inf], 3, 3)
    assert not kx.merge_certify(3, 0.5, [inf, np.nan], 3, 3)            # NaN counts as -inf
    assert not kx.merge_certify(2, 0.5, [inf, inf], 3, 3)               # got < need
    assert kx.merge_certify(2, 0.5, [inf, inf], 2, 3)                   # a short list, every row a candidate
    assert not kx.merge_certify(2, 0.5, [inf, f32(1.9)], 2, 3)          # a short list with a finite bound
    assert not kx.merge_certify(3, kx.POS_INF, [inf], 3, 3)             # inf < inf is false
    assert kx.merge_certify(5, 0.5, [f32(0.6)], 3, 5)                   # need below k, a full list


def test_rescore_build_names():
    b = kx.rescore_build
    assert b(n_items=5, ld=768, k=10, kp=63, cap=1024, sel=1, keys=True) == "k_rescore_kp<1>"
    assert b(n_items=5, ld=1152, k=10, kp=63, cap=1024, sel=1, keys=True) == "k_rescore<1,1,2,4>/sel"
    assert b(n_items=40, ld=768, k=10, kp=63, cap=1024, sel=1, keys=True) == "k_rescore<1,1,2,4>/sel"
    assert b(n_items=5, ld=768, k=10, kp=63, cap=2048, sel=1, top_w=512, keys=True) == "k_rescore_kp<1>/top"
    assert b(n_items=40, ld=768, k=100, kp=383, cap=6144) == "k_rescore<2,1,2,4>/A"
    assert b(n_items=40, ld=768, k=100, kp=383, cap=6144, keys=True) == "k_rescore<2,1,2,4>/B"
    assert b(n_items=40, ld=768, k=100, kp=383, cap=6144, keys=True, dev=True, qlist=True) == "k_rescore<2,8,2>"
    assert b(n_items=40, ld=768, k=10, kp=63, cap=1024, keys=True, excl=True) == "k_rescore_flat<1,12>"
    assert b(n_items=40, ld=64, k=256, kp=831, cap=13312, keys=True, excl=True) == "k_rescore_flat<4,0>"
    assert b(n_items=40, ld=1152, k=10, kp=63, cap=1024, keys=True, excl=True) == "k_rescore<1,1,2,4>/excl"
