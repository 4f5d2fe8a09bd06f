"""The numpy models of tests/kcheck.py, pinned by hand-derived cases (no GPU): the kernel-level GPU
tests compare the kernels with these models, so a model must be right on its own, not merely
consistent with itself."""
from fractions import Fraction

import numpy as np
import pytest

import kcheck as kc


def f32(x):
    return np.float32(x)


# ---- quantisation ------------------------------------------------------------------------
def test_quantize_four_element_row_by_hand():
    # a = (3, -4, 0, 12): |a| = 13, x = (3, -4, 0, 12) / 13, max|x| = 12/13.
    # s = the smallest f32 >= (12/13)/127 = 12/1651.
    # x/s = (3, -4, 0, 12) * 127/12 / (1 + d), d = s's relative rounding (0 <= d < 1.2e-7)
    #     = (31.75, -42.33.., 0, 127) / (1 + d)  ->  q = (32, -42, 0, 127)
    # x - s q = s * (-0.25, -1/3, 0, ~0)  ->  e_row = s * sqrt(1/16 + 1/9) = s * 5/12 = 5/1651,
    # up to d: each x/s moves by at most 127 d = 1.5e-5 steps against 5/12, well within 1e-4 relative.
    a = np.array([[3, -4, 0, 12]], np.float32)
    q, sc, e = kc.quantize(a, 32)
    assert q.tolist() == [[32, -42, 0, 127]]
    assert sc.dtype == np.float32 and sc.shape == (1,)
    assert float(sc[0]) >= 12 / 1651 and float(np.nextafter(sc[0], f32(0))) < 12 / 1651
    assert abs(e[0] - 5 / 1651) <= 1e-4 * 5 / 1651
    # a second, flat row in the same block takes the first row's scale:
    # x = (1/2, 1/2, 1/2, 1/2), x/s = 1651/24 = 68.79 -> 69, e_row = 2 s (69 - 68.79..) = s * 5/12
    a2 = np.array([[3, -4, 0, 12], [1, 1, 1, 1]], np.float32)
    q2, sc2, e2 = kc.quantize(a2, 32)
    assert q2.tolist() == [[32, -42, 0, 127], [69, 69, 69, 69]] and sc2[0] == sc[0]
    assert abs(e2[1] - 5 / 1651) <= 1e-4 * 5 / 1651
    # with a scale of its own (group = 1: the query side) it is exact: s >= 1/254, q = 127
    q3, sc3, e3 = kc.quantize(a2, 1)
    assert q3[1].tolist() == [127] * 4 and float(sc3[1]) >= 0.5 / 127 and e3[1] < 1e-6


def test_quantize_zero_row_and_scale_of_empty_group():
    a = np.zeros((33, 4), np.float32)
    a[32] = (0, 0, 2, 0)
    q, sc, e = kc.quantize(a, 32)
    assert not q[:32].any() and sc[0] == 1.0 and not e[:32].any()  # zero rows: q = 0, e = 0, scale 1.0
    assert q[32].tolist() == [0, 0, 127, 0] and float(sc[1]) >= 1 / 127


def test_quantize_clamps_to_127_and_ignores_row_magnitude():
    a = np.array([[1e-19, -1e-19, 5e-20, 0], [1e17, -1e17, 5e16, 0]], np.float32)
    q, sc, _ = kc.quantize(a, 1)
    assert q[0].tolist() == q[1].tolist() and abs(q).max() == 127
    assert q[0, 2] in (63, 64)  # 63.5 / (1 + d): the f32 inputs decide the side


def test_f32_round_up():
    assert kc.f32_round_up(np.float64(1.0)) == f32(1.0)
    assert kc.f32_round_up(np.float64(1.0) + 2.0 ** -30) == f32(1.0 + 2.0 ** -23)
    assert kc.f32_round_up(np.float64(0.1)) == f32(0.1)  # f32(0.1) = 0.100000001 >= 0.1
    assert float(kc.f32_round_up(np.float64(0.7))) >= 0.7 > float(f32(0.7))  # f32(0.7) = 0.699999988


def test_sequential_norm_is_sequential():
    # squares 2^24, 1, 1, 1, 1 in index order: 2^24 + 1 rounds back to 2^24 every time; a wider
    # accumulator reaches 2^24 + 4, whose root rounds to the next f32 above 4096
    q = np.array([[4096, 1, 1, 1, 1], [3, 4, 0, 0, 0], [0, 0, 0, 0, 0]], np.float32)
    nb = kc.seq_norm_f32(q)
    assert nb[0] == f32(4096.0) and nb[1] == f32(5.0)
    assert nb[2] == 0.0 and not np.signbit(nb[2])  # -0.0 + 0.0 = +0.0
    assert np.sqrt(np.float32(np.sum(q[0].astype(np.float64) ** 2))) != nb[0]


def test_query_flags():
    q = np.array([[1, 0], [0, 0], [1e-20, 0], [1e19, 1e19], [np.nan, 1], [np.inf, 1]], np.float32)
    nb = kc.seq_norm_f32(q)
    assert kc.query_flags(q, nb).tolist() == [0, 2, 2, 2, 3, 3]


# ---- keys --------------------------------------------------------------------------------
def test_key_order_by_hand():
    den = np.float32(1e-45)  # the smallest denormal
    vals = np.array([0.0, -0.0, 1.0, -1.0, den, -den], np.float32)
    o = kc.ord_f32(vals)
    assert [hex(int(x)) for x in o] == ["0x80000000", "0x7fffffff", "0xbf800000", "0x407fffff", "0x80000001",
                                        "0x7ffffffe"]
    keys = kc.score_key(vals, np.zeros(6, np.uint64))
    order = np.argsort(keys)  # ascending key = best score first
    assert vals[order].tolist() == [1.0, float(den), 0.0, -0.0, -float(den), -1.0]
    assert np.signbit(vals[order]).tolist() == [False, False, False, True, True, True]
    assert int(kc.score_key(f32(1.0), 5)) == 0x407FFFFF00000005
    # the row breaks ties: the smaller row first; a better score beats any row
    assert kc.score_key(f32(2.5), 3) < kc.score_key(f32(2.5), 4) < kc.score_key(f32(2.0), 0)
    assert kc.score_key(f32(np.inf), 0) < kc.score_key(f32(3e38), 0) and kc.score_key(f32(-np.inf), 0xFFFFFFFF) < kc.KEY_NONE
    # round trip, bit for bit (the sign of zero included)
    back = kc.score_key_score(keys)
    assert back.view(np.uint32).tolist() == vals.view(np.uint32).tolist()
    assert kc.key_row(kc.score_key(f32(-7.0), 0xFFFFFFFE)) == 0xFFFFFFFE


def test_kth_largest_with_ties():
    S = np.array([[3, 1, 3, 2, 2, 2, -0.0, 0.0]], np.float32)
    want = {1: 3.0, 2: 3.0, 3: 2.0, 5: 2.0, 6: 1.0, 7: 0.0, 8: -0.0}
    for ks, v in want.items():
        tau, best = kc.kth_largest(S, ks)
        assert tau[0] == v and np.signbit(tau[0]) == np.signbit(f32(v)), ks
        assert best.shape == (1, ks)
    _, best = kc.kth_largest(S, 8)
    assert kc.key_row(best[0]).tolist() == [0, 2, 3, 4, 5, 1, 7, 6]


# ---- scores ------------------------------------------------------------------------------
def test_integer_dot_is_exact_and_score_rounds_twice():
    A = np.full((3, 1152), 127, np.int8)
    A[1] = -127
    A[2, ::2] = 0
    B = np.full((2, 1152), 127, np.int8)
    B[1] = -127
    assert kc.idot(A, B).tolist() == [[18580608, -18580608], [-18580608, 18580608], [9290304, -9290304]]
    # the widest rows of the f32 matmul path (127^2 * 1024 < 2^24) against plain integer arithmetic
    rng = np.random.default_rng(5)
    A2 = np.where(rng.integers(0, 2, (40, 1024)) == 1, 127, -127).astype(np.int8)
    A2[0], A2[1] = 127, -127
    B2 = rng.integers(-127, 128, (9, 1024), dtype=np.int8)
    B2[0] = 127
    assert np.array_equal(kc.idot(A2, B2), A2.astype(np.int64) @ B2.astype(np.int64).T)
    assert kc.idot(A2, B2)[0, 0] == 127 * 127 * 1024
    # (float)I rounds to nearest even: 2^24 + 1 -> 2^24, 2^24 + 3 -> 2^24 + 4
    I = np.array([[2 ** 24 + 1], [2 ** 24 + 3], [-(2 ** 24 + 1)]], np.int64)
    assert kc.score(I, np.ones(3, np.float32), np.ones(1, np.float32))[:, 0].tolist() == [2.0 ** 24, 2.0 ** 24 + 4, -2.0 ** 24]
    # two roundings, in this order.  I = 5 and two scales given by their bit patterns:
    # rounding each product (exact rational arithmetic below, not numpy's f32) gives a value that
    # differs both from the other order of the multiplies and from one rounding of the product.
    s1, s2 = np.array([1031510449], np.uint32).view(np.float32)[0], np.array([1027654030], np.uint32).view(np.float32)[0]
    F1, F2 = Fraction(float(s1)), Fraction(float(s2))
    want = _rn32(Fraction(float(_rn32(5 * F1))) * F2)
    v = kc.score(np.array([[5]], np.int64), np.array([s1]), np.array([s2]))[0, 0]
    assert v.dtype == np.float32 and v == want
    assert _rn32(Fraction(float(_rn32(5 * F2))) * F1) != want and _rn32(5 * F1 * F2) != want


def _rn32(x: Fraction):
    """Round an exact rational to the nearest f32 (ties to even), without f32 arithmetic."""
    f = np.float32(float(x))
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(c.view(np.uint32)) & 1))
    return best


def test_emit_keys_include_ties_at_tau():
    Sq = np.array([0.5, 0.25, 0.5, -1.0, 0.25], np.float32)
    assert kc.key_row(kc.emit_keys(Sq, 0.5)).tolist() == [0, 2]
    assert kc.key_row(kc.emit_keys(Sq, 0.25)).tolist() == [0, 2, 1, 4]
    assert kc.emit_keys(Sq, np.inf).size == 0 and kc.emit_keys(Sq, -np.inf).size == 5
    assert kc.key_row(kc.emit_keys(np.array([0.0, -0.0], np.float32), 0.0)).tolist() == [0, 1]  # -0.0 >= +0.0


def test_top_workgroup_rows_partition():
    # n = 70: 5 units of 16, rows 0 .. 79 laid out as eight strided pairs per unit, 2 * 5 apart
    wg = kc.top_workgroup_rows(70, 2)
    # unit 0 holds rows 0, 1, 10, 11, 20, 21, ...; unit 1 rows 2, 3, 12, 13, ...: workgroup = unit % 2
    assert wg[[0, 1, 10, 11, 60, 61]].tolist() == [0] * 6
    assert wg[[2, 3, 12, 13, 62, 63]].tolist() == [1] * 6
    assert wg[[4, 5, 8, 9]].tolist() == [0, 0, 0, 0] and wg[[6, 7]].tolist() == [1, 1]


# ---- the committed data sets sit on no rounding tie ------------------------------------------
def _same_in_longdouble(rows, group, what):
    q64, s64, _ = kc.quantize(rows, group)
    q80, s80, _ = kc.quantize(rows, group, np.longdouble)
    assert np.array_equal(q64, q80) and np.array_equal(s64.view(np.uint32), s80.view(np.uint32)), what


@pytest.mark.parametrize("dim", kc.PREP_DIMS)
def test_committed_row_cases_have_no_excused_element(dim):
    """The model in np.longdouble gives the operand and the scales the float64 model gives, for
    every corpus tests/test_gpu_kernels_prep.py compares with the model -- every n with every plant
    position, the sample operands, data (b) and (c): nothing there lies within a double's rounding
    of a tie, so the GPU tests' excuse count is expected to be 0.  (Where np.longdouble is no wider
    than float64 the comparison is trivially true.)"""
    for n in kc.PREP_NS:
        for plant in kc.plant_positions(n):
            _same_in_longdouble(kc.prep_rows(n, dim, plant), 32, (n, plant))
    for n in kc.PREP_SAMPLE_NS:
        _same_in_longdouble(kc.prep_rows(n, dim, kc.plant_positions(n)[-1])[::32], 128, ("sample", n))
    for kind in ("b", "c"):
        for d, n in kc.PREP_KIND_CASES:
            if d == dim:
                _same_in_longdouble(kc.prep_rows(n, d, None, kind), 32, (kind, n))


@pytest.mark.parametrize("dim", kc.QUERY_DIMS + tuple(d for d in kc.QUERY_KIND_DIMS if d not in kc.QUERY_DIMS))
def test_committed_query_cases_have_no_excused_element(dim):
    batches = []
    if dim in kc.QUERY_DIMS:
        batches += [kc.prep_queries(nq, dim, variant=variant) for nq, variant in kc.QUERY_BATCHES]
    if dim in kc.QUERY_KIND_DIMS:
        batches += [kc.prep_queries(40, dim, kind) for kind in ("b", "c")]
    for q in batches:
        ok = kc.query_flags(q, kc.seq_norm_f32(q)) == 0
        _same_in_longdouble(q[ok], 1, (dim, q.shape))


def test_planted_row_is_the_worst_row():
    for dim in kc.PREP_DIMS:
        for n in (33, 257):
            for plant in kc.plant_positions(n):
                _, _, e = kc.quantize(kc.prep_rows(n, dim, plant), 32)
                assert int(np.argmax(e)) == plant, (dim, n, plant)


# ---- the mask bitsets ----------------------------------------------------------------------
def _bit(words, i):
    return (int(words[i >> 6]) >> (i & 63)) & 1


def _rows_by_loop(allow, dead, n):
    return [i for i in range(n)
            if (allow is None or _bit(allow, i)) and not (dead is not None and _bit(dead, i))]


@pytest.mark.parametrize("n", [n for n in kc.MASK_NS if n <= 2 * 16384 + 100])
def test_mask_list_model_against_a_loop(n):
    """mask_rows / mask_list_model (np.unpackbits) against a bit-by-bit loop: every mask kind and
    dead kind of the GPU test, the block prefixes included."""
    rows_per_block = 64 * kc.MASK_BLOCK_WORDS
    for kind in kc.MASK_KINDS:
        allow = kc.mask_case(n, kind)
        if kind == "garbage" and n % 64:
            assert int(allow[-1]) >> (n % 64) == (1 << (64 - n % 64)) - 1  # test data: the tail is set
        for dkind in kc.DEAD_KINDS:
            dead = kc.dead_case(n, dkind, allow)
            want = _rows_by_loop(allow, dead, n)
            blk, ids = kc.mask_list_model(allow, dead, n)
            assert ids.dtype == np.uint32 and ids.tolist() == want, (kind, dkind)
            assert len(blk) == kc.mask_blocks(n) + 1 and blk[-1] == len(want)
            for b in range(kc.mask_blocks(n)):
                assert blk[b] == sum(1 for i in want if i < b * rows_per_block), (kind, dkind, b)
            if dkind == "superset":
                assert not want
            if kind == "last" and dkind == "none":
                assert want == [n - 1]
            if kind in ("full", "none") and dkind == "none":
                assert want == list(range(n))


def test_mask_blocks_and_pack_bits_by_hand():
    assert [kc.mask_blocks(n) for n in (0, 1, 16384, 16385, 257 * 16384 + 5)] == [1, 1, 1, 2, 258]
    w = kc.pack_bits(np.array([1, 0, 1] + [0] * 61 + [1], bool))
    assert w.tolist() == [5, 1]


def test_mask_cut_model_against_a_loop():
    n = 100
    allow = kc.mask_case(n, "garbage", seed=4)
    dead = kc.dead_case(n, "random", None, seed=5)
    rows = [0, 99, 100, 127, 128, 5000, 0xFFFFFFFE, 17, 17, 64, 63]
    keys = np.array([((i + 1) << 32) | r for i, r in enumerate(rows)] + [int(kc.KEY_NONE)], np.uint64)
    for d in (None, dead):
        want = [int(k) for k in keys
                if int(k) != int(kc.KEY_NONE) and (int(k) & 0xFFFFFFFF) < n
                and _bit(allow, int(k) & 0xFFFFFFFF) and not (d is not None and _bit(d, int(k) & 0xFFFFFFFF))]
        assert kc.mask_cut_model(keys, allow, d, n).tolist() == want
    assert kc.mask_cut_model(keys[:0], allow, None, n).tolist() == []
