"""Kernel-level checks of the 768-byte gang build of the emit filter, k_filter_qs16<true, 12, true>
(csrc/k_filter.hip), whose level 2 queues raw records and scores them at the flush.

launch_filter_emit takes this build only from about 5.6M rows (kGangMinTiles static tiles per row
stream); launch_filter_emit_gang (tests/kcheck/kcheck_gang.cpp -> lib/libbsr_kcheck_gang.so)
launches it whatever the shard size.  Below kGangMinTiles no workgroup runs in a gang, so the
throttle is idle and everything else -- the schedule, the dynamic tail, the sample-tile map, level 1,
the queue and its flush -- runs as at 10M rows.

Every case compares, per query, the emitted keys with the exact model
    emitted(q) = { score_key(v, row) : v = ((float)I * s_block) * s_query >= tau[q], row < n_rows }
(kcheck.emit_keys over kcheck.score(kcheck.idot(...))): the same keys, each once, cnt[q] the model's
count also where the list overflows, and no word of the list written past the count.  The model is
exact: no tolerance.

Sample tiles.  The kernel's map from logical to physical tiles skips tile 32 L + 31 for every L; it
is correct exactly when s_tiles = floor(ceil(n / 128) / 32), the value emit_pass passes
(sample_tiles_for).  At 20,037 rows that is 4; s_tiles = 1 or 2 there would send the last logical
tiles past the operand.  So s_tiles = 1 and 2 run at 5,157 and 8,997 rows (41 and 71 tiles), and
20,037 rows runs with its own 4.
"""
import ctypes
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import kcheck as kc

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
PATTERN = np.uint64(0xEEEEEEEEEEEEEEEE)
ROW_BYTES = 768
SMALL = 128 * 3 + 5     # 4 tiles, the last partial: fewer tiles than row streams, workgroups with no tile
BIG = 20000 + 37        # 157 tiles, the last partial: static streams and a 19-tile pooled tail
NQS = (17, 257, 769, 1000)  # 1, 2, 4 and 4 query tiles, the last with padding queries
GANG_LIB = os.path.join(kc.ROOT, "better-search-rag-rust_amd", "lib", "libbsr_kcheck_gang.so")

_gang = None


def _gang_lib():
    """libbsr_kcheck_gang.so (raises if it has not been built: there is no other path)."""
    global _gang
    if _gang is None:
        if not os.path.exists(GANG_LIB):
            raise RuntimeError(f"{GANG_LIB} not built (run __graft_entry__.build())")
        _gang = ctypes.CDLL(GANG_LIB)
    return _gang


def _qpad(nq):
    return kc.round_up(nq, 256)


@functools.lru_cache(maxsize=None)
def _case(n, nq, kind="d"):
    """One operand pair and its model scores M [row][query], computed once and shared (read-only).
    kind "d": kcheck's synthetic int8 data; "neg": positive rows against negated positive queries,
    so every dot product, score and threshold is negative."""
    rng = np.random.default_rng(51000 + 7 * n + nq + (1 if kind == "neg" else 0))
    qpad = _qpad(nq)
    A, a_scale = kc.synth_operand(rng, n, ROW_BYTES, 32, kc.round_up(n, 256))
    B, b_scale = kc.synth_queries(rng, nq, qpad, ROW_BYTES)
    if kind == "neg":
        A[:n] = rng.integers(1, 128, (n, ROW_BYTES), dtype=np.int8)
        B[:nq] = -rng.integers(1, 128, (nq, ROW_BYTES), dtype=np.int8)
    M = kc.score(kc.idot(A[:n], B), kc.row_scales(a_scale, 32, n), b_scale)
    for a in (A, a_scale, B, b_scale, M):
        a.setflags(write=False)
    return SimpleNamespace(n=n, nq=nq, qpad=qpad, A=A, a_scale=a_scale, B=B, b_scale=b_scale, M=M)


def _tau_rate(c, rows_mask=None):
    """Per-query tau at the bench's emission rate: the query's m-th largest score, m = ceil(n / 1000)
    (about its 99.9th percentile; the m-th row sits exactly at tau).  Padding queries: +inf."""
    M = c.M if rows_mask is None else c.M[rows_mask]
    m = max(1, -(-M.shape[0] // 1000))
    tau = np.full(c.qpad, INF, np.float32)
    tau[:c.nq] = -np.partition(-M[:, :c.nq], m - 1, axis=0)[m - 1]
    return tau


def _launch(which, c, tau, cap, tail=True, s_tiles=0, A=None, a_scale=None):
    """One emit launch as emit_pass makes it: cnt zeroed, tail = cnt + qpad or nullptr."""
    A = c.A if A is None else A
    a_scale = c.a_scale if a_scale is None else a_scale
    cand = np.full((c.qpad, cap), PATTERN, np.uint64)
    cnt = np.zeros(kc.cnt_words(c.qpad), np.uint32)
    tau = np.ascontiguousarray(tau, np.float32)
    if which == "small":
        kc.gemm(kc.EMIT, A=A, n_rows=c.n, a_scale_rows=32, B=c.B, a_scale=a_scale, b_scale=c.b_scale,
                n_qt=c.qpad // 256, tau=tau, cand=cand, cnt=cnt, cap=cap, tail=tail, n_q=c.nq,
                n_rt=(c.n + 255) // 256, s_tiles=s_tiles)
        return cand, cnt
    g = kc._Gemm()
    for name, arr in (("A", A), ("B", c.B), ("a_scale", a_scale), ("b_scale", c.b_scale), ("tau", tau),
                      ("cand", cand), ("cnt", cnt)):
        assert arr.flags.c_contiguous
        setattr(g, name, arr.ctypes.data)
    g.a_bytes, g.b_bytes = A.nbytes, c.B.nbytes
    g.a_scale_bytes, g.b_scale_bytes = a_scale.nbytes, c.b_scale.nbytes
    g.tau_bytes, g.cand_bytes, g.cnt_bytes = tau.nbytes, cand.nbytes, cnt.nbytes
    g.a_stride, g.n_rows, g.a_scale_rows, g.row_bytes = ROW_BYTES, c.n, 32, ROW_BYTES
    g.n_rt, g.n_qt, g.cap = (c.n + 255) // 256, c.qpad // 256, cap
    g.tail_off = c.qpad if tail else -1
    g.n_q, g.s_tiles = c.nq, s_tiles
    rc = _gang_lib().kc_gemm_gang(ctypes.byref(g))
    assert rc == 0, f"kc_gemm_gang: hipError_t {rc}"
    return cand, cnt


def _check(cand, cnt, M, tau, cap, rows_mask=None, what=""):
    """Every query's list against the model (rows_mask: the rows the launch is responsible for)."""
    rows = None if rows_mask is None else np.flatnonzero(rows_mask)
    Mr = M if rows is None else M[rows]
    for q in range(cand.shape[0]):
        want = kc.emit_keys(Mr[:, q], tau[q], rows)
        c = int(cnt[q])
        assert c == want.size, f"{what} query {q}: cnt {c}, model {want.size} (tau {tau[q]!r})"
        if c <= cap:
            got = np.sort(cand[q, :c])
            if not np.array_equal(got, want):
                miss, extra = np.setdiff1d(want, got), np.setdiff1d(got, want)
                raise AssertionError(f"{what} query {q}: {miss.size} keys missing (rows {kc.key_row(miss)[:8]}), "
                                     f"{extra.size} not in the model (rows {kc.key_row(extra)[:8]})")
            assert (cand[q, c:] == PATTERN).all(), f"{what} query {q}: a word written past the count"
        else:  # overflowed: the cap stored keys are distinct members of the model set
            assert np.unique(cand[q]).size == cap, f"{what} query {q}: a key twice in an overflowed list"
            assert np.isin(cand[q], want).all(), f"{what} query {q}: an overflowed list holds a key outside the model set"


@pytest.mark.parametrize("tail", (True, False), ids=("tail", "notail"))
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("n", (SMALL, BIG))
def test_bench_rate(gpu, n, nq, tail):
    """tau at the bench's rate, every shape, pooled tail and static-only."""
    c = _case(n, nq)
    tau = _tau_rate(c)
    cand, cnt = _launch("gang", c, tau, 1024, tail)
    _check(cand, cnt, c.M, tau, 1024, what=f"n={n} nq={nq} tail={tail}")
    emitted = int(cnt[:c.nq].sum())
    assert emitted >= c.nq * max(1, -(-n // 1000)), "the m-th row itself reaches tau"


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("n", (SMALL, BIG))
def test_tau_inf_emits_nothing(gpu, n, nq):
    """tau = +inf: no lane passes level 1, the queue is never touched, nothing is written."""
    c = _case(n, nq)
    cand, cnt = _launch("gang", c, np.full(c.qpad, INF, np.float32), 64)
    assert not cnt[:c.qpad].any()
    assert (cand == PATTERN).all()


@pytest.mark.parametrize("tail", (True, False), ids=("tail", "notail"))
@pytest.mark.parametrize("cap", (512, 256, 64))
def test_dense_overfills_the_queue(gpu, cap, tail):
    """tau = -inf at 389 rows, 17 queries: every lane of every tile passes, 128 records per wave and
    tile against a queue of kEmitQueueDepth -- the enqueue / flush / continue loop -- and, with
    cap < n_rows, the overflow of the lists at cap."""
    assert _gang_lib().kc_gang_queue_depth() < 128
    c = _case(SMALL, 17)
    tau = np.full(c.qpad, INF, np.float32)
    tau[:c.nq] = -INF
    cand, cnt = _launch("gang", c, tau, cap, tail)
    assert (cnt[:c.nq] == SMALL).all()
    _check(cand, cnt, c.M, tau, cap, what=f"dense cap={cap} tail={tail}")


@pytest.mark.parametrize("n,nq", ((SMALL, 17), (BIG, 257), (BIG, 1000)))
def test_ties_at_tau_are_emitted(gpu, n, nq):
    """A row planted twice in one 32-row block (the copy of a query's operand: the query's best
    dot product) at the first and last rows of a tile, across a 16-row block's edge and at the
    shard's last rows, their block's scale set to the data's largest so that nothing else of the shard
    reaches them; tau of that query = the planted rows' exact score.  Both copies sit at tau."""
    c = _case(n, nq)
    A, a_scale = c.A.copy(), c.a_scale.copy()
    spots = {0: 0, 1: 126, 2: 15, nq - 1: n - 2}  # query -> first row of its pair
    if n > 128 * 78:
        spots[5] = 128 * 77 + 30  # a tile of the middle of a static stream
    for q, r in spots.items():
        A[r] = A[r + 1] = c.B[q]
        a_scale[r // 32] = 0.1  # the largest scale of the data: the pair is near the query's top
    rows = np.array(sorted({32 * (r // 32) + i for r in spots.values() for i in range(32) if 32 * (r // 32) + i < n}))
    M = c.M.copy()
    M[rows] = kc.score(kc.idot(A[rows], c.B), kc.row_scales(a_scale, 32, n)[rows], c.b_scale)
    tau = _tau_rate(c)
    for q, r in spots.items():
        tau[q] = M[r, q]
        assert M[r + 1, q] == tau[q]
    cand, cnt = _launch("gang", c, tau, 1024, A=A, a_scale=a_scale)
    _check(cand, cnt, M, tau, 1024, what=f"ties n={n} nq={nq}")
    for q, r in spots.items():
        assert 2 <= cnt[q] <= 1024, f"query {q}: {cnt[q]} rows at or above the planted pair's score"
        got = kc.key_row(cand[q, :int(cnt[q])])
        assert r in got and r + 1 in got, f"query {q}: a planted row at tau is missing"


@pytest.mark.parametrize("n,nq", ((SMALL, 257), (BIG, 257), (BIG, 1000)))
def test_all_negative_scores(gpu, n, nq):
    """Positive rows against negated queries: every score and every threshold is negative, so level 1
    must score a lane's (negative) integer maximum with the tile's SMALLEST block scale."""
    c = _case(n, nq, "neg")
    tau = _tau_rate(c)
    assert (c.M[:, :nq] < 0).all() and (tau[:nq] < 0).all()
    cand, cnt = _launch("gang", c, tau, 1024)
    _check(cand, cnt, c.M, tau, 1024, what=f"negative n={n} nq={nq}")


@pytest.mark.parametrize("tail", (True, False), ids=("tail", "notail"))
@pytest.mark.parametrize("n,s_tiles", ((40 * 128 + 37, 1), (70 * 128 + 37, 2), (BIG, 4)))
def test_sample_tiles_are_skipped(gpu, n, s_tiles, tail):
    """s_tiles set in GemmArgs: the emitted set is the model's over the non-sample tiles only (the
    rows of tiles 32 L + 31 are launch_sample_fixup's)."""
    assert kc.lib().kc_sample_tiles_for(n) == s_tiles
    c = _case(n, 257)
    mask = ~kc.sample_tile_rows(n, s_tiles)
    assert mask.sum() == n - 128 * s_tiles
    tau = _tau_rate(c, mask)
    cand, cnt = _launch("gang", c, tau, 1024, tail, s_tiles=s_tiles)
    _check(cand, cnt, c.M, tau, 1024, rows_mask=mask, what=f"n={n} s_tiles={s_tiles} tail={tail}")


@pytest.mark.parametrize("n,nq,s_tiles", ((SMALL, 17, 0), (BIG, 257, 0), (BIG, 1000, 0), (BIG, 769, 4)))
def test_both_builds_emit_the_same(gpu, n, nq, s_tiles):
    """The same operand and tau through launch_filter_emit (the small-shard build at these sizes) and
    the forced gang launcher: equal counts and equal key sets."""
    c = _case(n, nq)
    tau = _tau_rate(c)
    tau[min(5, nq - 1)] = -INF  # one dense query: its list overflows in both
    a_cand, a_cnt = _launch("small", c, tau, 1024, s_tiles=s_tiles)
    b_cand, b_cnt = _launch("gang", c, tau, 1024, s_tiles=s_tiles)
    assert np.array_equal(a_cnt[:c.qpad], b_cnt[:c.qpad])
    for q in range(c.qpad):
        k = int(a_cnt[q])
        if k <= 1024:
            assert np.array_equal(np.sort(a_cand[q, :k]), np.sort(b_cand[q, :k])), f"query {q}"
