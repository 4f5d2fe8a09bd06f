"""Kernel-level checks of the filter's scores (csrc/k_filter.hip, sample mode): every score the
sample kernels store equals ((float)I * s_block) * s_query of the exact integer dot product I, bit
for bit, for every build a batch can reach:

  k_filter_qs16<false, NK>      NK = 2, 4, 6, 8, 10, 12 (row_bytes 128 .. 768, even slice counts)
  k_filter<false>               row_bytes 64, 192 (odd slice counts), 1152 (more than 12 slices)
  k_filter_skinny2<Sample, NK>  NK = 4, 8, 12, 16 (batches of <= 16 queries, rows of <= 1024 bytes)
  k_filter_skinny<false>        row_bytes 1152

The launches follow sample_pass (index.cpp): the operand is the contiguous sample (every 32nd corpus
row), one scale per 128 sample rows, padded to a multiple of 128 rows; S is [qpad][s_ld] with
s_ld = ceil(n_s / 256) * 256 (every score) or * 8 (compact: the maximum of every 32 sample rows).
Padding queries have a zero operand and scale 0, as k_query_prep leaves them.
"""
import numpy as np
import pytest

import kcheck as kc

pytestmark = pytest.mark.gpu

BIG = 300 * 128 + 37  # 301 tiles of 128: two tiles for some of qs16's 256 row streams at n_qt = 1


def _sample(A, a_scale, n_s, B, b_scale, skinny, compact):
    qpad = B.shape[0]
    n_rt = (n_s + 255) // 256
    s_ld = n_rt * (8 if compact else 256)
    S = np.full((qpad, s_ld), np.nan, np.float32)
    kc.gemm(kc.SKINNY_SAMPLE if skinny else kc.SAMPLE, A=A, n_rows=n_s, a_scale_rows=128, B=B, a_scale=a_scale,
            b_scale=b_scale, n_qt=qpad // 256, S=S, s_ld=s_ld, s_compact=1 if compact else 0, n_rt=n_rt)
    return S


def _check_scores(A, a_scale, n_s, B, b_scale, skinny=False, compact_too=False):
    """Full mode: S[q][r] for every q < qpad, r < n_s; compact mode: the maxima of the model's scores
    over the same 32-row groups.  Compared in slabs of 1024 queries."""
    S = _sample(A, a_scale, n_s, B, b_scale, skinny, False)
    Sc = _sample(A, a_scale, n_s, B, b_scale, skinny, True) if compact_too else None
    s_rows = kc.row_scales(a_scale, 128, n_s)
    ng = (n_s + 31) // 32
    for q0 in range(0, B.shape[0], 1024):
        q1 = min(q0 + 1024, B.shape[0])
        M = kc.score(kc.idot(A[:n_s], B[q0:q1]), s_rows, b_scale[q0:q1])  # [row][query]
        got = S[q0:q1, :n_s].T
        if not np.array_equal(got.view(np.uint32), M.view(np.uint32)):
            r, q = np.argwhere(got.view(np.uint32) != M.view(np.uint32))[0]
            raise AssertionError(f"score[row {r}][query {q0 + q}]: gpu {got[r, q]!r} model {M[r, q]!r}; "
                                 f"{np.count_nonzero(got.view(np.uint32) != M.view(np.uint32))} differ")
        if Sc is not None:
            pad = np.full((ng * 32, q1 - q0), -np.inf, np.float32)
            pad[:n_s] = M
            want = pad.reshape(ng, 32, q1 - q0).max(axis=1)
            gotc = Sc[q0:q1, :ng].T
            assert np.array_equal(gotc.view(np.uint32), want.view(np.uint32)), "compact maxima differ"


def _synthetic(rng, n_s, row_bytes, nq, qpad):
    A, a_scale = kc.synth_operand(rng, n_s, row_bytes, 128, kc.round_up(n_s, 128))
    B, b_scale = kc.synth_queries(rng, nq, qpad, row_bytes)
    return A, a_scale, B, b_scale


@pytest.mark.parametrize("row_bytes", (64, 128, 192, 256, 384, 512, 640, 768, 1152))
def test_sample_scores_batched(gpu, row_bytes):
    """Data (d) through launch_filter_sample: n_s in {1, 127, 129, 300 * 128 + 37} at one query tile
    (compact too at the largest), and n_qt = 2, 3, 5 -- the grids at 3 and 5 leave workgroups
    inactive -- at 129 rows, and at 7000 rows (more tiles than row streams at n_qt = 5) and the
    301-tile shape for the narrowest and widest query-stationary builds and an odd slice count."""
    rng = np.random.default_rng(31000 + row_bytes)
    for n_s in (1, 127, 129, BIG):
        A, a_scale, B, b_scale = _synthetic(rng, n_s, row_bytes, 250, 256)
        _check_scores(A, a_scale, n_s, B, b_scale, compact_too=n_s in (129, BIG))
    for n_qt in (2, 3, 5):
        for n_s in ((129, 7000, BIG) if row_bytes in (128, 192, 768) else (129,)):
            A, a_scale, B, b_scale = _synthetic(rng, n_s, row_bytes, 256 * n_qt - 9, 256 * n_qt)
            _check_scores(A, a_scale, n_s, B, b_scale, compact_too=n_s == 7000)


def test_sample_scores_33_query_tiles(gpu):
    """The n_qt >= 32 grid (one workgroup per query tile and XCD): 33 query tiles, 3000 rows, NK = 12."""
    rng = np.random.default_rng(33)
    A, a_scale, B, b_scale = _synthetic(rng, 3000, 768, 33 * 256 - 100, 33 * 256)
    _check_scores(A, a_scale, 3000, B, b_scale)


@pytest.mark.parametrize("row_bytes", (192, 256, 512, 768, 1024, 1152))
def test_sample_scores_skinny(gpu, row_bytes):
    """Data (d) through launch_filter_skinny_sample: k_filter_skinny2<Sample, 4 | 8 | 12 | 16> (192
    bytes: three slices in the NK = 4 build) and k_filter_skinny (1152)."""
    rng = np.random.default_rng(32000 + row_bytes)
    for n_s in (1, 127, 129, BIG):
        for nq in (16, 3):
            A, a_scale, B, b_scale = _synthetic(rng, n_s, row_bytes, nq, 16)
            _check_scores(A, a_scale, n_s, B, b_scale, skinny=True, compact_too=True)


@pytest.mark.parametrize("kind", ("a", "b", "c"))
@pytest.mark.parametrize("dim", (130, 768, 1100))
def test_sample_scores_prepared_data(gpu, kind, dim):
    """Data (a), (b), (c) as the product prepares it: the sample operand of a 4097-row corpus (129
    sample rows, two scale groups) from k_rows_to_i8_sample and the queries from k_query_prep, through
    the batched (40 queries) and the skinny (7 queries) sample kernels; the model is applied to the
    operands the GPU produced."""
    rows = kc.prep_rows(4097, dim, None, kind)
    op, sc = kc.rows_to_i8_sample(rows)
    n_s = 129
    for nq in (40, 7):
        qp = kc.query_prep(kc.prep_queries(nq, dim, kind)[:nq], np.float32(0.004), True)
        assert (qp["qflags"][:nq] == 0).sum() >= nq - 4
        _check_scores(op, sc, n_s, qp["qop"], qp["qscale"], skinny=nq <= 16, compact_too=True)
