"""Kernel-level checks of the emission (csrc/k_filter.hip): launch_filter_emit,
launch_filter_skinny_emit and launch_sample_fixup against the exact model
    emitted(q) = { score_key(v, row) : v = ((float)I * s_block) * s_query >= tau[q], row < n_rows }
(ties at tau included), every key once.  Certification assumes exactly this set: a row dropped at
some (tile position, query lane, n mod 128) would go unnoticed by the end-to-end tests unless it
happened to be one of a query's top k.

The launches follow emit_pass (index.cpp): the operand padded to 256 rows with zero rows (scale 1.0),
one scale per 32 rows, cnt zeroed as k_select_tau leaves it, tail = cnt + qpad (or nullptr), padding
queries with a zero operand, scale 0 and tau = +inf.

Builds reached: k_filter_qs16<true, NK> for NK = 2 .. 10, the small-shard NK = 12 build (the one
launch_filter picks when no row-stream gang is possible), k_filter<true>, k_filter_skinny2<Emit,
4 | 8 | 12 | 16>, k_filter_skinny_glds<Emit, 12> and k_filter_skinny<true>.  NOT reached: the gang
build of k_filter_qs16<true, 12> -- it needs kGangMinTiles = 600 static tiles per row stream, about
9.8M rows, which no test of a few seconds can hold; tests/test_gpu_full_size.py covers it end to end.
"""
import numpy as np
import pytest

import kcheck as kc

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
BIG = 300 * 128 + 37       # 301 tiles: more tiles than row streams at one query tile
TAIL12 = 100 * 128 - 77    # 100 tiles: 12 tail tiles, pools of 2, two of the 8 pools empty
NOTAIL = 7 * 128 - 5       # 7 tiles: fewer than 8, the dynamic tail is empty


def _emit(kind, A, a_scale, n, B, b_scale, nq, tau, cap, tail=True, cand=None, cnt=None, **kw):
    qpad = B.shape[0]
    if cand is None:
        cand = np.full((qpad, cap), 0xEEEEEEEEEEEEEEEE, np.uint64)
        cnt = np.zeros(kc.cnt_words(qpad), np.uint32)
    kc.gemm(kind, A=A, n_rows=n, a_scale_rows=32, B=B, a_scale=a_scale, b_scale=b_scale, n_qt=qpad // 256,
            tau=tau, cand=cand, cnt=cnt, cap=cap, tail=tail, n_q=nq, n_rt=(n + 255) // 256, **kw)
    return cand, cnt


def _thresholds(M, nq, qpad, dense_q=5):
    """tau per query: the model's own m-th largest score, m in {1, 17, 64} (ties exactly at tau
    exist); queries 3 and 4: +inf; query `dense_q`: -inf; padding: +inf."""
    n = M.shape[0]
    tau = np.full(qpad, INF, np.float32)
    for q in range(nq):
        m = min((1, 17, 64)[q % 3], n)
        tau[q] = kc.kth_largest(M[:, q][None, :], m)[0][0]
    tau[3] = tau[4] = INF
    if dense_q is not None and dense_q < nq:
        tau[dense_q] = -INF
    return tau


def _check_lists(cand, cnt, M, tau, cap, rows_mask=None, what=""):
    """Every query's list against the model (rows_mask: the rows the launch is responsible for)."""
    qpad = cand.shape[0]
    rows = None if rows_mask is None else np.flatnonzero(rows_mask)
    for q in range(qpad):
        Sq = M[:, q] if rows is None else M[rows, q]
        want = kc.emit_keys(Sq, tau[q], rows)
        c = int(cnt[q])
        assert c == want.size, f"{what} query {q}: cnt {c}, model {want.size} (tau {tau[q]!r})"
        if c <= cap:
            got = np.sort(cand[q, :c])
            if not np.array_equal(got, want):
                miss = np.setdiff1d(want, got)
                extra = np.setdiff1d(got, want)
                raise AssertionError(f"{what} query {q}: {miss.size} keys missing (rows {kc.key_row(miss)[:8]}), "
                                     f"{extra.size} not in the model (rows {kc.key_row(extra)[:8]})")
        else:  # overflowed: the cap stored keys are distinct members of the model set
            got = cand[q]
            assert np.unique(got).size == cap, f"{what} query {q}: a key twice in an overflowed list"
            assert np.isin(got, want).all(), f"{what} query {q}: an overflowed list holds a key outside the model set"


def _model(A, a_scale, n, B, b_scale):
    return kc.score(kc.idot(A[:n], B), kc.row_scales(a_scale, 32, n), b_scale)  # [row][query]


def _synthetic(rng, n, row_bytes, nq, qpad):
    A, a_scale = kc.synth_operand(rng, n, row_bytes, 32, kc.round_up(n, 256))
    B, b_scale = kc.synth_queries(rng, nq, qpad, row_bytes)
    return A, a_scale, B, b_scale


def _run_shape(kind, rng, n, row_bytes, nq, qpad, tail=True, dense=True, overflow=True, what=""):
    A, a_scale, B, b_scale = _synthetic(rng, n, row_bytes, nq, qpad)
    M = _model(A, a_scale, n, B, b_scale)
    tau = _thresholds(M, nq, qpad, dense_q=5 if dense else None)
    cap = max(n, 64) if dense else 1024  # dense: cap >= n_rows, past a lane's ring and the staged lists
    cand, cnt = _emit(kind, A, a_scale, n, B, b_scale, nq, tau, cap, tail)
    _check_lists(cand, cnt, M, tau, cap, what=f"{what} n={n} cap={cap}")
    if overflow and n > 64:
        tau2 = tau.copy()
        tau2[min(5, nq - 1)] = -INF
        cand, cnt = _emit(kind, A, a_scale, n, B, b_scale, nq, tau2, 64, tail)
        assert cnt[min(5, nq - 1)] == n
        _check_lists(cand, cnt, M, tau2, 64, what=f"{what} n={n} cap=64")


@pytest.mark.parametrize("row_bytes", (128, 256, 384, 512, 640, 768))
def test_emit_query_stationary(gpu, row_bytes):
    """k_filter_qs16<true, NK>, data (d): 1, 127, 129 rows (fewer tiles than row streams), 7 tiles
    (empty tail), 100 tiles (12 tail tiles: pools of 2, two pools empty) and the 301-tile shape at
    one query tile; 129 rows, 100 tiles and 301 tiles at n_qt = 2 and 3; tail = nullptr at 129 rows,
    7, 100 and 301 tiles."""
    rng = np.random.default_rng(41000 + row_bytes)
    for n in (1, 127, 129, NOTAIL, TAIL12):
        _run_shape(kc.EMIT, rng, n, row_bytes, 250, 256, what=f"rb={row_bytes}")
    _run_shape(kc.EMIT, rng, BIG, row_bytes, 250, 256, dense=row_bytes == 768, overflow=False, what=f"rb={row_bytes}")
    for n in (129, NOTAIL, TAIL12, BIG):
        _run_shape(kc.EMIT, rng, n, row_bytes, 250, 256, tail=False, dense=n == 129, overflow=False,
                   what=f"rb={row_bytes} no tail")
    for n_qt in (2, 3):
        for n in (129, TAIL12, BIG):
            _run_shape(kc.EMIT, rng, n, row_bytes, 256 * n_qt - 9, 256 * n_qt, dense=n == 129, overflow=n == 129,
                       what=f"rb={row_bytes} n_qt={n_qt}")


@pytest.mark.parametrize("row_bytes", (64, 192, 1152))
def test_emit_general_filter(gpu, row_bytes):
    """k_filter<true> (odd slice counts, and more than 12 slices): 256-row tiles."""
    rng = np.random.default_rng(42000 + row_bytes)
    for n in (1, 127, 129, 257, TAIL12):
        _run_shape(kc.EMIT, rng, n, row_bytes, 250, 256, what=f"rb={row_bytes}")
    _run_shape(kc.EMIT, rng, BIG, row_bytes, 250, 256, dense=False, overflow=False, what=f"rb={row_bytes}")
    for n_qt in (2, 3):
        _run_shape(kc.EMIT, rng, 2500, row_bytes, 256 * n_qt - 9, 256 * n_qt, what=f"rb={row_bytes} n_qt={n_qt}")


@pytest.mark.parametrize("row_bytes,glds", ((256, None), (512, None), (768, None), (768, "0"), (1024, None), (1152, None)))
def test_emit_skinny(gpu, monkeypatch, row_bytes, glds):
    """launch_filter_skinny_emit: k_filter_skinny2<Emit, NK>, k_filter_skinny_glds<Emit, 12> (768-byte
    rows; BSR_SKINNY_GLDS=0 takes k_filter_skinny2 instead) and k_filter_skinny (1152)."""
    if glds is None:
        monkeypatch.delenv("BSR_SKINNY_GLDS", raising=False)
    else:
        monkeypatch.setenv("BSR_SKINNY_GLDS", glds)
    assert kc.lib().kc_skinny_glds_on() == (0 if glds == "0" else 1)
    rng = np.random.default_rng(43000 + row_bytes + (1 if glds else 0))
    for n in (1, 127, 129, TAIL12, BIG):
        for nq in (16, 7):
            _run_shape(kc.SKINNY_EMIT, rng, n, row_bytes, nq, 16, overflow=nq == 16, what=f"rb={row_bytes} nq={nq}")


# ---- prepared data: operands from k_rows_to_i8 and k_query_prep -----------------------------------
def _prepared(kind, n, dim, nq):
    """Data (a), (b) or (c) as the product prepares it: (op, scales, qop, qscale, nq, live queries).
    (c) is all-positive rows against all-negative queries with no zero row and no special query, so
    every integer dot product, every score and every threshold is negative: k_filter_qs16's integer
    pre-test then scores a lane's maximum with the tile's SMALLEST block scale, and a whole tile's
    maxima stay below zero."""
    rng = np.random.default_rng(46000 + 7 * dim + n + nq)
    if kind == "c":
        rows, q = kc.data_positive(rng, n, dim), -kc.data_positive(rng, nq, dim)
    else:
        rows, q = kc.prep_rows(n, dim, None, kind), kc.prep_queries(nq, dim, kind)
    op, sc, ea = kc.rows_to_i8(rows)
    qp = kc.query_prep(q, ea, True)
    live = np.flatnonzero(qp["qflags"][:nq] == 0)
    assert live.size >= nq - 4 and (kind != "c" or live.size == nq)
    return op, sc, qp["qop"], qp["qscale"], nq, live


def _thresholds_live(M, live, qpad, kind, dense_q=None):
    """tau of the i-th live query: the model's m-th largest score, m = (1, 17, 64)[i % 3]; every other
    query (flagged, padding) +inf, as k_select_tau leaves it.  Data (c): every tau is negative."""
    tau = np.full(qpad, INF, np.float32)
    for i, q in enumerate(live):
        tau[q] = kc.kth_largest(M[:, q][None, :], min((1, 17, 64)[i % 3], M.shape[0]))[0][0]
    if kind == "c":
        assert (M[:, live] < 0).all() and (tau[live] < 0).all(), "data (c): every score and threshold negative"
    if dense_q is not None:
        tau[dense_q] = -INF
    return tau


@pytest.mark.parametrize("kind", ("a", "b", "c"))
@pytest.mark.parametrize("launch,dim,nq,glds", (
    (kc.EMIT, 768, 250, None),         # k_filter_qs16, the small-shard NK = 12 build
    (kc.EMIT, 768, 500, None),         # ... two query tiles
    (kc.EMIT, 384, 250, None),         # k_filter_qs16<true, 6>
    (kc.EMIT, 100, 250, None),         # k_filter_qs16<true, 2>
    (kc.EMIT, 130, 250, None),         # k_filter<true>, 192-byte rows
    (kc.EMIT, 1100, 250, None),        # k_filter<true>, 1152-byte rows
    (kc.SKINNY_EMIT, 768, 16, None),   # k_filter_skinny_glds<Emit, 12>
    (kc.SKINNY_EMIT, 768, 16, "0"),    # k_filter_skinny2<Emit, 12>
    (kc.SKINNY_EMIT, 200, 11, None),   # k_filter_skinny2<Emit, 4>
    (kc.SKINNY_EMIT, 1000, 16, None),  # k_filter_skinny2<Emit, 16>
    (kc.SKINNY_EMIT, 1100, 16, None),  # k_filter_skinny<true>
))
def test_emit_prepared_data(gpu, monkeypatch, kind, launch, dim, nq, glds):
    """Emission on data (a), (b), (c) prepared by k_rows_to_i8 and k_query_prep (the inputs of the score
    tests), thresholds the model's own m-th largest score, m in {1, 17, 64}: 1000 rows and the
    100-tile shape, and once more with a dense query (tau = -inf, cap >= n_rows) among them."""
    if glds is None:
        monkeypatch.delenv("BSR_SKINNY_GLDS", raising=False)
    else:
        monkeypatch.setenv("BSR_SKINNY_GLDS", glds)
    for n in (1000, TAIL12):
        op, sc, qop, qscale, nq, live = _prepared(kind, n, dim, nq)
        M = _model(op, sc, n, qop, qscale)
        tau = _thresholds_live(M, live, qop.shape[0], kind)
        cand, cnt = _emit(launch, op, sc, n, qop, qscale, nq, tau, 1024)
        _check_lists(cand, cnt, M, tau, 1024, what=f"data ({kind}) dim {dim} n={n}")
        if n == 1000:
            tau = _thresholds_live(M, live, qop.shape[0], kind, dense_q=int(live[2]))
            cand, cnt = _emit(launch, op, sc, n, qop, qscale, nq, tau, 1024)
            _check_lists(cand, cnt, M, tau, 1024, what=f"data ({kind}) dim {dim} n={n} dense")


# ---- prepared data and the bound itself -----------------------------------------------------------
@pytest.mark.parametrize("kind", ("a", "b", "c"))
@pytest.mark.parametrize("dim", (768, 130))
def test_bound_holds_for_every_pair(gpu, kind, dim):
    """Data (a), (b), (c) prepared by k_rows_to_i8 and k_query_prep; dense emission (tau = -inf, cap >=
    n_rows) returns the filter's score of EVERY (query, row) pair, which must be the model's, and
        |score - cos64(q, r)| <= ebound[q]
    with cos64 the float64 cosine of the original f32 vectors -- the statement certification rests on.
    Prints the largest ratio found.  dim 768: the small-shard NK = 12 build; dim 130: k_filter."""
    n, nq = 1000, 40
    rows = kc.prep_rows(n, dim, 500, kind)
    op, sc, ea = kc.rows_to_i8(rows)
    q = kc.prep_queries(nq, dim, kind)
    qp = kc.query_prep(q, ea, True)
    qpad = qp["qpad"]
    live = np.flatnonzero(qp["qflags"][:nq] == 0)
    assert live.size >= nq - 4
    tau = np.full(qpad, INF, np.float32)
    tau[live] = -INF
    cap = 1024
    cand, cnt = _emit(kc.EMIT, op, sc, n, qp["qop"], qp["qscale"], nq, tau, cap)
    M = _model(op, sc, n, qp["qop"], qp["qscale"])
    _check_lists(cand, cnt, M, tau, cap, what=f"data ({kind}) dim {dim}")
    S = np.full((n, qpad), np.nan, np.float32)
    for qi in live:
        keys = cand[qi, :n]
        S[kc.key_row(keys), qi] = kc.score_key_score(keys)
    C = kc.cos64(rows, q)
    err = np.abs(S[:, live].astype(np.float64) - C[:, live])
    ratio = err / qp["ebound"][live].astype(np.float64)[None, :]
    print(f"bound data ({kind}) dim {dim}: max |score - cos| / ebound = {ratio.max():.4f} "
          f"(max error {err.max():.3e}, ebound {qp['ebound'][live].min():.3e} .. {qp['ebound'][live].max():.3e}, ea {ea:.3e})")
    assert np.all(err <= qp["ebound"][live].astype(np.float64)[None, :])


# ---- sample tiles -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(32 * 2 + 31) * 128 + r for r in (1, 33, 127)] + [9 * 32 * 128 + 5])
@pytest.mark.parametrize("row_bytes,n_qt", ((768, 1), (768, 2), (128, 1), (384, 1)))
def test_sample_tiles(gpu, n, row_bytes, n_qt):
    """s_tiles != 0 (sample_pass / emit_pass with sample tiles): one 128-row tile in 32 is scored by
    the sample pass alone -- S[q][4 L + g] = the exact maximum emit score of block g of tile
    32 L + 31 -- the emit pass walks the other tiles, and launch_sample_fixup emits the sample
    tiles' rows.  The first three n leave the last sample tile partial."""
    rng = np.random.default_rng(44000 + n + row_bytes + n_qt)
    qpad = 256 * n_qt
    nq = qpad - 9
    A, a_scale, B, b_scale = _synthetic(rng, n, row_bytes, nq, qpad)
    M = _model(A, a_scale, n, B, b_scale)
    _check_sample_tiles(A, a_scale, n, B, b_scale, nq, M, _thresholds(M, nq, qpad, dense_q=None))


def _check_sample_tiles(A, a_scale, n, B, b_scale, nq, M, tau):
    qpad = B.shape[0]
    n_qt = qpad // 256
    tiles = kc.lib().kc_sample_tiles_for(n)
    assert tiles == ((n + 127) // 128) // 32 and tiles >= 3
    in_sample = kc.sample_tile_rows(n, tiles)
    last0 = ((tiles - 1) * 32 + 31) * 128
    s_vals = 4 * (tiles - 1) + (min(128, n - last0) + 31) // 32
    s_ld = 4 * tiles
    # the sample pass
    S = np.full((qpad, s_ld), np.nan, np.float32)
    kc.gemm(kc.SAMPLE, A=A, n_rows=n, a_scale_rows=32, B=B, a_scale=a_scale, b_scale=b_scale, n_qt=n_qt, S=S,
            s_ld=s_ld, s_compact=1, n_rt=tiles, s_tiles=tiles, s_vals=s_vals)
    for j in range(s_vals):
        r0 = ((j >> 2) * 32 + 31) * 128 + (j & 3) * 32
        want = M[r0:min(r0 + 32, n)].max(axis=0)
        assert np.array_equal(S[:, j].view(np.uint32), want.view(np.uint32)), f"sample value {j} (rows {r0} ..)"
    # the emit pass alone: the passing rows outside the sample tiles, no row of a sample tile
    cap = 2048
    cand, cnt = _emit(kc.EMIT, A, a_scale, n, B, b_scale, nq, tau, cap, S=S, s_ld=s_ld, s_tiles=tiles, s_vals=s_vals)
    _check_lists(cand, cnt, M, tau, cap, rows_mask=~in_sample, what="emit alone")
    # emit + fix-up: the full model set, each key once; a query with tau = +inf gets nothing
    cand, cnt = _emit(kc.FIXUP, A, a_scale, n, B, b_scale, nq, tau, cap, cand=cand, cnt=cnt, S=S, s_ld=s_ld,
                      s_tiles=tiles, s_vals=s_vals)
    assert not cnt[:qpad][np.isposinf(tau)].any()
    _check_lists(cand, cnt, M, tau, cap, what="emit + fix-up")


@pytest.mark.parametrize("kind", ("a", "b", "c"))
@pytest.mark.parametrize("dim", (768, 384))
def test_sample_tiles_prepared_data(gpu, kind, dim):
    """The same three steps on data (a), (b), (c) prepared by k_rows_to_i8 and k_query_prep, 96 tiles
    with a partial last sample tile; (c): every threshold negative."""
    n = (32 * 2 + 31) * 128 + 33
    op, sc, qop, qscale, nq, live = _prepared(kind, n, dim, 250)
    M = _model(op, sc, n, qop, qscale)
    tau = _thresholds_live(M, live, qop.shape[0], kind)
    _check_sample_tiles(op, sc, n, qop, qscale, nq, M, tau)
