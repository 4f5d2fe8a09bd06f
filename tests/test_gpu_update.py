"""In-place update (bsr_index_update): rows of a loaded shard replaced, their ids
kept.  The expected result everywhere is the reference's compute_local_top_k
(src/mpi_helpers/metrics.rs:16-53) over a numpy copy of the rows with the same replacements:
oracle.parallel_top_k(rows_modified[live_ids], queries, k) with the indices mapped through live_ids
(+ offset) -- counts, indices, order and f32 distance bits, with the (~0, +inf) tail.  The derived
state is checked against a second Index freshly loaded with the modified rows: equal operands and
samples emit equally, and the updated index's row error bound is never the smaller."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THREADS = 16
NONE_IDX = np.uint64(2 ** 64 - 1)
E_INVALID, E_NONFINITE, E_STATE = -1, -2, -7


def _same(got, want, ctx):
    gi, gd, gc = got
    wi, wd, wc = want
    assert np.array_equal(gc, wc), (ctx, gc, wc)
    for q in range(len(wc)):
        c = int(wc[q])
        assert np.array_equal(gi[q, :c], wi[q, :c]), (ctx, q, gi[q, :c], wi[q, :c])
        assert np.array_equal(gd[q, :c].view(np.uint32), wd[q, :c].view(np.uint32)), (ctx, q)
        assert np.all(gi[q, c:] == NONE_IDX) and np.all(np.isposinf(gd[q, c:])), (ctx, q, "tail")


def _want(oracle_mod, host, ids, qs, k, offset=0):
    """The reference's local top-k over the rows ids (ascending), global indices."""
    ids = np.asarray(ids, np.int64)
    nq = len(qs)
    if len(ids) == 0:
        return (np.full((nq, k), NONE_IDX), np.full((nq, k), np.inf, np.float32), np.zeros(nq, np.uint32))
    wi, wd, wc = oracle_mod.parallel_top_k(np.ascontiguousarray(host[ids]), np.ascontiguousarray(qs), k,
                                           size=THREADS, threads=THREADS)
    gi = np.full((nq, k), NONE_IDX)
    for q in range(nq):
        c = int(wc[q])
        gi[q, :c] = ids[wi[q, :c].astype(np.int64)].astype(np.uint64) + np.uint64(offset)
    return gi, wd, wc


def _bf16_bits(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _widen(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


class Model:
    """The numpy model of an index: the f32 rows as stored, the dead bits, the expected lists."""

    def __init__(self, oracle_mod, rows, offset=0):
        self.oracle, self.rows, self.offset = oracle_mod, np.array(rows, np.float32), offset
        self.dead = np.zeros(len(rows), bool)

    def update(self, local_ids, new_rows):
        self.rows[np.asarray(local_ids, np.int64)] = new_rows

    def want(self, qs, k, allow=None):
        keep = ~self.dead if allow is None else (~self.dead & allow)
        return _want(self.oracle, self.rows, np.flatnonzero(keep), qs, k, self.offset)


def _fresh_stats(bsr_mod, rows, qs, k, offset=0):
    """(n_emitted, n_fallback, row_ebound) of the search on an index freshly loaded with rows."""
    f = bsr_mod.Index(rows.shape[1], max_k=64, device=0)
    f.load(rows, global_offset=offset)
    f.local_top_k(qs, k)
    st = f.last_stats()
    f.close()
    return st.n_emitted, st.n_fallback, st.row_ebound


def _check_stage(bsr_mod, ix, m, qs, k, ctx, nqs=(5, 40)):
    """get_many, the searches against the oracle, emission and error bound against a fresh load."""
    assert np.array_equal(ix.get_many().view(np.uint32), m.rows.view(np.uint32)), (ctx, "get_many")
    assert ix.get_count() == len(m.rows) and ix.global_offset() == m.offset
    for nq in nqs:
        got = ix.local_top_k(qs[:nq], k)
        st = ix.last_stats()
        _same(got, m.want(qs[:nq], k), (ctx, nq))
        emitted, _, ebound = _fresh_stats(bsr_mod, m.rows, qs[:nq], k, m.offset)
        print(f"{ctx} nq={nq}: emitted={st.n_emitted} fresh={emitted} ebound={st.row_ebound:.6g} fresh={ebound:.6g} "
              f"fallback={st.n_fallback}")
        assert st.n_emitted == emitted, (ctx, nq, st.n_emitted, emitted)
        assert st.row_ebound >= ebound, (ctx, nq, st.row_ebound, ebound)


# ---- 1. the stages at the small odd shape ---------------------------------------------------------
N1, D1, OFF1, K = 3001, 100, 1000, 10


def test_small_stages(bsr_mod, oracle_mod, gpu):
    import torch
    rng = np.random.default_rng(131)
    n, dim, off, k = N1, D1, OFF1, K
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.update([off], rows[:1])
    assert e.value.status == E_STATE
    ix.load(rows, global_offset=off)
    m = Model(oracle_mod, rows, off)
    ix.update([], np.zeros((0, dim), np.float32))  # n_ids = 0: BSR_OK
    _check_stage(bsr_mod, ix, m, qs, k, "as loaded")

    def stage(local_ids, new_rows, ctx, ids_dev=False, rows_dev=False):
        local_ids = np.asarray(local_ids, np.int64)
        new_rows = np.ascontiguousarray(new_rows, np.float32)
        ids = (local_ids + off).astype(np.uint64)
        a = torch.from_numpy(ids.astype(np.int64)).to("cuda:0") if ids_dev else ids
        r = torch.from_numpy(new_rows).to("cuda:0") if rows_dev else new_rows
        ix.update(a, r)
        m.update(local_ids, new_rows)
        _check_stage(bsr_mod, ix, m, qs, k, ctx)

    def fresh(count):
        return rng.uniform(-1, 1, (count, dim)).astype(np.float32)

    stage([0, 31, 32, 63, 64, 3000], fresh(6), "word and block edges")
    # rows the fop_s sample reads (local 0 and 32 j): the group path; and one that it does not
    stage([0, 32 * 7, 32 * 93, 45], fresh(4), "sampled rows")
    # a far row becomes query 0's nearest neighbour: a stale operand would leave it unemitted
    cos = (m.rows @ qs[0]) / np.maximum(np.linalg.norm(m.rows, axis=1), 1e-30)
    far = int(np.argmin(cos))
    stage([far], 1.5 * qs[:1], "nearest neighbour")
    got = ix.local_top_k(qs[:5], k)
    assert got[0][0, 0] == far + off, (got[0][0], far + off)
    # a spike: one large component among small ones, in a block of ordinary rows -- a stale block
    # scale would clamp it
    spike = np.full(dim, 1e-3, np.float32)
    spike[7] = 1.0
    row_s = 32 * 31 + 8
    stage([row_s], spike[None, :], "spike")
    blk = np.arange(32 * 31, 32 * 32)
    qb = np.ascontiguousarray(m.rows[blk])  # the spike and the 31 other rows of its block, as queries
    got = ix.local_top_k(qb, k)
    _same(got, m.want(qb, k), "spike block self-queries")
    assert got[0][8, 0] == row_s + off and np.array_equal(got[0][:, 0], (blk + off).astype(np.uint64))
    got1 = ix.local_top_k(spike[None, :], k)
    _same(got1, m.want(spike[None, :], k), "spike query")
    assert got1[0][0, 0] == row_s + off
    # a zero row scores 1.0; a row replaced by its own values changes nothing
    before = ix.local_top_k(qs, k)
    stage([1234], m.rows[1234:1235].copy(), "own values")
    after = ix.local_top_k(qs, k)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    stage([500], np.zeros((1, dim), np.float32), "zero row")
    only = ix.local_top_k(qs[:3], 1, allow_ids=[500], mask_mode="list")
    assert np.all(only[0][:, 0] == 500 + off) and np.all(only[1][:, 0] == np.float32(1.0))
    # ids and rows as device tensors; host ids with device rows; device ids with host rows
    stage([3, 2999, 1500], fresh(3), "device ids, device rows", ids_dev=True, rows_dev=True)
    stage([4, 96, 2047, 2048], fresh(4), "host ids, device rows", rows_dev=True)
    stage([5, 1024], fresh(2), "device ids, host rows", ids_dev=True)
    # a larger update: more than one workgroup of every list kernel's input
    ids = rng.choice(n, 700, replace=False)
    stage(ids, fresh(700), "700 rows")
    ix.close()


def test_small_stages_bf16(bsr_mod, oracle_mod, gpu):
    """A bf16 index: the incoming rows are bf16 bits, widened exactly."""
    import torch
    rng = np.random.default_rng(132)
    n, dim, off, k = N1, D1, OFF1, K
    bits = _bf16_bits(rng.uniform(-1, 1, (n, dim)))
    qs = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
    ix = bsr_mod.Index(dim, max_k=64, device=0, dtype=bsr_mod.BSR_BF16)
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.update([off], bits[:1])
    assert e.value.status == E_STATE
    ix.load(bits, global_offset=off)
    m = Model(oracle_mod, _widen(bits), off)

    def stage(local_ids, ctx, rows_dev=False):
        local_ids = np.asarray(local_ids, np.int64)
        new = _bf16_bits(rng.uniform(-1, 1, (len(local_ids), dim)))
        r = torch.from_numpy(new.view(np.int16)).to("cuda:0") if rows_dev else new
        ix.update(local_ids + off, r)
        m.update(local_ids, _widen(new))
        _check_stage(bsr_mod, ix, m, qs, k, ctx)

    stage([0, 31, 32, 63, 64, 3000], "bf16 word and block edges")
    stage([0, 32 * 7, 32 * 93, 45], "bf16 sampled rows", rows_dev=True)
    bad = bits[:2].copy()
    bad[1, dim - 1] = 0x7FC0  # a bf16 NaN
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.update([off + 1, off + 2], bad)
    assert e.value.status == E_NONFINITE
    _check_stage(bsr_mod, ix, m, qs, k, "bf16 after a refused update", nqs=(5,))
    ix.close()


# ---- 2. all or nothing ----------------------------------------------------------------------------
def test_all_or_nothing(bsr_mod, oracle_mod, gpu):
    import torch
    rng = np.random.default_rng(133)
    n, dim, off, k = N1, D1, OFF1, K
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(rows, global_offset=off)
    m = Model(oracle_mod, rows, off)
    want5, want40 = m.want(qs[:5], k), m.want(qs, k)
    stored = ix.get_many()
    assert np.array_equal(stored.view(np.uint32), rows.view(np.uint32))
    new = rng.uniform(-1, 1, (50, dim)).astype(np.float32)
    good = rng.choice(n, 50, replace=False).astype(np.int64) + off

    def refused(ids, new_rows, status, ctx, dev=False):
        ids = np.asarray(ids, np.int64)
        a, r = ids, new_rows
        if dev:
            a, r = torch.from_numpy(ids).to("cuda:0"), torch.from_numpy(new_rows).to("cuda:0")
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.update(a, r)
        assert e.value.status == status, (ctx, e.value.status)
        assert np.array_equal(ix.get_many().view(np.uint32), stored.view(np.uint32)), (ctx, "get_many")
        _same(ix.local_top_k(qs[:5], k), want5, (ctx, 5))
        _same(ix.local_top_k(qs, k), want40, (ctx, 40))

    for bad_id in (off - 1, off + n, 7):
        for pos in (0, 49):
            ids = good.copy()
            ids[pos] = bad_id
            refused(ids, new, E_INVALID, ("out of range", bad_id, pos), dev=pos == 0)
    ids = good.copy()
    ids[49] = ids[3]
    refused(ids, new, E_INVALID, "duplicate")
    refused(ids, new, E_INVALID, "duplicate, device", dev=True)
    for bad_val in (np.nan, np.inf, -np.inf):
        x = new.copy()
        x[49, dim - 1] = bad_val
        refused(good, x, E_NONFINITE, ("non-finite", bad_val), dev=bad_val == np.inf)
    # null pointers with n_ids > 0
    L = bsr_mod.lib()
    assert L.bsr_index_update(ix._h, None, new.ctypes.data, 50) == E_INVALID
    assert L.bsr_index_update(ix._h, good.astype(np.uint64).ctypes.data, None, 50) == E_INVALID
    assert L.bsr_index_update(ix._h, None, None, 0) == 0
    # the same call, valid, goes through
    ix.update(good, new)
    m.update(good - off, new)
    _same(ix.local_top_k(qs, k), m.want(qs, k), "accepted")
    assert np.array_equal(ix.get_many().view(np.uint32), m.rows.view(np.uint32))
    ix.close()


# ---- 3. with tombstones ---------------------------------------------------------------------------
def _want_grouped(m, qs, k, masks, qmask):
    nq = len(qs)
    wi = np.full((nq, k), NONE_IDX)
    wd = np.full((nq, k), np.inf, np.float32)
    wc = np.zeros(nq, np.uint32)
    for g in range(len(masks)):
        sel = np.flatnonzero(qmask == g)
        if len(sel):
            gi, gd, gc = m.want(qs[sel], k, allow=masks[g])
            wi[sel], wd[sel], wc[sel] = gi, gd, gc
    return wi, wd, wc


def test_with_tombstones(bsr_mod, oracle_mod, gpu):
    rng = np.random.default_rng(134)
    n, extra, dim, off, k = N1, 100, D1, OFF1, K
    rows = rng.uniform(-1, 1, (n + extra, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(rows[:n], global_offset=off)
    m = Model(oracle_mod, rows[:n], off)
    gone = np.flatnonzero(rng.random(n) < 0.3)
    assert ix.delete(gone + off) == len(gone)
    m.dead[gone] = True
    ids = np.union1d(rng.choice(np.flatnonzero(~m.dead), 170, replace=False), rng.choice(gone, 30, replace=False))
    assert len(ids) == 200 and np.count_nonzero(m.dead[ids]) == 30
    new = rng.uniform(-1, 1, (len(ids), dim)).astype(np.float32)
    new[0] = 1.25 * qs[1]  # (a live or deleted row turned into query 1's best match)
    ix.update(ids + off, new)
    m.update(ids, new)

    def check(ctx):
        cnt = len(m.rows)
        assert ix.live_count() == int(np.count_nonzero(~m.dead)) and ix.get_count() == cnt
        assert np.array_equal(ix.deleted_mask(), m.dead), ctx
        assert np.array_equal(ix.get_many().view(np.uint32), m.rows.view(np.uint32)), (ctx, "get_many")
        for nq in (5, 40):
            _same(ix.local_top_k(qs[:nq], k), m.want(qs[:nq], k), (ctx, "plain", nq))
        allow = np.random.default_rng(4).random(cnt) < 0.5
        for mode in ("list", "filter"):
            got = ix.local_top_k(qs, k, allow_mask=allow, mask_mode=mode)
            _same(got, m.want(qs, k, allow=allow), (ctx, "masked", mode))
        masks = np.stack([allow, ~allow, np.random.default_rng(5).random(cnt) < 0.1])
        qmask = np.arange(len(qs)) % 3
        for mode in ("list", "filter"):
            got = ix.local_top_k_grouped(qs, k, masks, qmask, mask_mode=mode)
            _same(got, _want_grouped(m, qs, k, masks, qmask), (ctx, "grouped", mode))

    check("updated with tombstones")
    # append keeps both; the appended rows can be updated too
    ix.append_many(rows[n:])
    m.rows = np.concatenate([m.rows, rows[n:]])
    m.dead = np.concatenate([m.dead, np.zeros(extra, bool)])
    check("appended")
    ids2 = n + rng.choice(extra, 10, replace=False)
    new2 = rng.uniform(-1, 1, (10, dim)).astype(np.float32)
    ix.update(ids2 + off, new2)
    m.update(ids2, new2)
    check("appended rows updated")
    ix.close()


# ---- 4. the filter path at the workload's width ---------------------------------------------------
def test_filter_path_768(bsr_mod, oracle_mod, gpu):
    rng = np.random.default_rng(135)
    n, dim, nq, k = 40_000, 768, 40, 10
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(rows)
    m = Model(oracle_mod, rows)
    want = m.want(qs, k)
    for rep in range(3):
        _same(ix.local_top_k(qs, k), want, ("before", rep))
    assert ix.last_stats().graph_replay == 1
    ids = rng.choice(n, 1000, replace=False)
    new = rng.uniform(-1, 1, (1000, dim)).astype(np.float32)
    new[:nq] = 1.5 * qs  # every query's nearest neighbour changes: a pre-update result cannot pass
    ix.update(ids, new)
    m.update(ids, new)
    want = m.want(qs, k)
    assert np.array_equal(want[0][:, 0], ids[:nq].astype(np.uint64))
    for rep in range(3):
        got = ix.local_top_k(qs, k)
        st = ix.last_stats()
        _same(got, want, ("after", rep))
        print(f"after update, search {rep}: graph_replay={st.graph_replay} emitted={st.n_emitted} "
              f"fallback={st.n_fallback}")
    assert st.graph_replay == 1
    assert st.n_exact_direct == 0
    emitted, fallback, ebound = _fresh_stats(bsr_mod, m.rows, qs, k)
    assert st.n_emitted == emitted, (st.n_emitted, emitted)
    assert st.row_ebound >= ebound
    if fallback == 0:
        assert st.n_fallback == 0
    assert np.array_equal(ix.get_many().view(np.uint32), m.rows.view(np.uint32))
    # A second update of the same size grows no buffer: the captured graph bakes in nothing an
    # update changes, so the very next search replays -- and must see the new rows.  (The fresh
    # index above allocated, which drops every captured graph: three searches capture again.)
    for rep in range(3):
        _same(ix.local_top_k(qs, k), want, ("recapture", rep))
    assert ix.last_stats().graph_replay == 1
    ids2 = rng.choice(n, 1000, replace=False)
    new2 = rng.uniform(-1, 1, (1000, dim)).astype(np.float32)
    new2[:nq] = 1.75 * qs
    ix.update(ids2, new2)
    m.update(ids2, new2)
    got = ix.local_top_k(qs, k)
    assert ix.last_stats().graph_replay == 1
    _same(got, m.want(qs, k), "replayed after the second update")
    ix.close()


# ---- 5. sticky flags ------------------------------------------------------------------------------
def test_sticky_flags(bsr_mod, oracle_mod, gpu):
    rng = np.random.default_rng(136)
    n, dim, off, k = N1, D1, OFF1, K
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(rows, global_offset=off)
    m = Model(oracle_mod, rows, off)
    _same(ix.local_top_k(qs, k), m.want(qs, k), "as loaded")
    assert ix.last_stats().n_exact_direct == 0
    u = rng.uniform(-1, 1, dim)
    huge = (u / np.linalg.norm(u) * 1e19).astype(np.float32)[None, :]  # magnitude 1e19: kRowNormRange
    ix.update([off + 77], huge)
    m.update([77], huge)
    for nq in (5, 40):
        _same(ix.local_top_k(qs[:nq], k), m.want(qs[:nq], k), ("huge row", nq))
        assert ix.last_stats().n_exact_direct == nq
    back = rng.uniform(-1, 1, (1, dim)).astype(np.float32)
    ix.update([off + 77], back)
    m.update([77], back)
    for nq in (5, 40):
        _same(ix.local_top_k(qs[:nq], k), m.want(qs[:nq], k), ("ordinary again", nq))
    assert ix.last_stats().n_exact_direct == 40  # sticky, as documented: only a load clears the flag
    ix.load(m.rows, global_offset=off)
    _same(ix.local_top_k(qs, k), m.want(qs, k), "reloaded")
    assert ix.last_stats().n_exact_direct == 0
    ix.close()


# ---- 6. the parallel entry point ------------------------------------------------------------------
def test_parallel(bsr_mod, oracle_mod, gpu):
    rng = np.random.default_rng(137)
    n, dim, off, k = N1, D1, 0, K
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (40, dim)).astype(np.float32)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(rows, global_offset=off)
    m = Model(oracle_mod, rows, off)
    _same(bsr_mod.parallel_top_k_similarity_search_batch(None, ix, qs, k), m.want(qs, k), "before")
    ids = rng.choice(n, 300, replace=False)
    new = rng.uniform(-1, 1, (300, dim)).astype(np.float32)
    new[:5] = 2.0 * qs[:5]
    ix.update(ids, new)
    m.update(ids, new)
    got = bsr_mod.parallel_top_k_similarity_search_batch(None, ix, qs, k)
    _same(got, m.want(qs, k), "after")
    assert np.array_equal(got[0][:5, 0], ids[:5].astype(np.uint64))
    ix.close()
