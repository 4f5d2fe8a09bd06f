"""Tombstones (bsr_index_delete): rows of a loaded shard marked as deleted, honoured
by every search.  The expected result everywhere is the reference's compute_local_top_k
(src/mpi_helpers/metrics.rs:16-53) over a store that holds only the live rows, each keeping its
global index: oracle.parallel_top_k(rows[live_ids], queries, k) with the indices mapped through
live_ids (+ offset) -- counts, indices, order and f32 distance bits, with the (~0, +inf) tail."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THREADS = 16
NONE_IDX = np.uint64(2 ** 64 - 1)
E_INVALID, E_STATE = -1, -7


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


class Model:
    """The numpy model of an index with tombstones: the rows, the dead bits, the expected lists."""

    def __init__(self, oracle_mod, rows, offset=0):
        self.oracle, self.rows, self.offset = oracle_mod, rows, offset
        self.dead = np.zeros(len(rows), bool)

    def delete(self, local_ids):
        """-> the number of rows that go live -> deleted."""
        local_ids = np.unique(np.asarray(local_ids, np.int64))
        newly = int(np.count_nonzero(~self.dead[local_ids]))
        self.dead[local_ids] = True
        return newly

    def live(self):
        return np.flatnonzero(~self.dead)

    def want(self, qs, k, allow=None):
        keep = ~self.dead if allow is None else (~self.dead & allow)
        return _want(self.oracle, self.rows, np.flatnonzero(keep), qs, k, self.offset)

    def top(self, qs, k):
        """Local ids of every query's current top-k (the distinct ones)."""
        wi, _, wc = self.want(qs, k)
        ids = np.concatenate([wi[q, :int(wc[q])] for q in range(len(qs))]).astype(np.int64) - self.offset
        return np.unique(ids)


def _check_state(ix, m):
    assert ix.live_count() == int(np.count_nonzero(~m.dead))
    assert ix.get_count() == len(m.rows)
    assert np.array_equal(ix.deleted_mask(), m.dead)


# ---- 1. small, odd width: every stage down to an empty shard ---------------------------------
def test_small_stages(bsr_mod, oracle_mod, gpu):
    import torch
    rng = np.random.default_rng(31)
    n, dim, nq, k, off = 3001, 100, 5, 10, 1000
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.delete([off])
    assert e.value.status == E_STATE
    ix.load(rows, global_offset=off)
    m = Model(oracle_mod, rows, off)
    _check_state(ix, m)
    _same(ix.local_top_k(qs, k), m.want(qs, k), "no tombstone")
    assert ix.delete([]) == 0

    def stage(local_ids, ctx, as_tensor=False):
        ids = np.asarray(local_ids, np.int64) + off
        arg = torch.from_numpy(ids).to("cuda:0") if as_tensor else ids
        assert ix.delete(arg) == m.delete(local_ids), ctx
        _check_state(ix, m)
        got = ix.local_top_k(qs, k)
        want = m.want(qs, k)
        assert np.all(want[2] == min(k, ix.live_count()))
        _same(got, want, ctx)

    stage([0, 63, 64, 3000], "word edges")
    # duplicates and rows deleted before count once
    assert ix.delete(np.array([63, 63, 5, 5, 5, 0], np.uint64) + np.uint64(off)) == m.delete([5])
    _check_state(ix, m)
    # query 0's current top-3: its list must shift
    before = m.want(qs[:1], k)[0][0]
    stage(before[:3].astype(np.int64) - off, "top-3 of query 0", as_tensor=True)
    assert np.array_equal(ix.local_top_k(qs[:1], k)[0][0, :k - 3], before[3:])
    # an id outside [offset, offset + n): nothing changes
    for bad in ([off - 1, off + 7], [off + 8, off + n], [7]):
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.delete(np.asarray(bad, np.uint64))
        assert e.value.status == E_INVALID
        _check_state(ix, m)
    stage(np.flatnonzero(rng.random(n) < 0.3), "30%")
    # deleted rows keep their place and their stored values
    assert np.array_equal(ix.get_many(), rows)
    keep = rng.choice(m.live(), 7, replace=False)
    stage(np.setdiff1d(np.arange(n), keep), "all but 7", as_tensor=True)
    assert ix.live_count() == 7
    stage(np.arange(n), "all")
    assert ix.live_count() == 0 and np.all(ix.local_top_k(qs, k)[2] == 0)
    ix.close()


# ---- 2, 4, 7 (zero query), 9: one shard of 40,037 x 768 uniform rows ---------------------------
N, D = 40_037, 768


@pytest.fixture(scope="module")
def base(gpu):
    rng = np.random.default_rng(32)
    rows = rng.uniform(-1, 1, (N, D)).astype(np.float32)
    qs = rng.uniform(-1, 1, (40, D)).astype(np.float32)
    return rows, qs


def test_batched_replay_and_stale_graph(bsr_mod, oracle_mod, base):
    """The query-stationary path: exact with 30% + every query's top-5 deleted, replayed from the
    third search of a shape on; a delete after a capture must not be answered from the stale graph
    (its baked live count and bitset), and replay resumes two searches later."""
    rows, qs = base
    ix = bsr_mod.Index(D, max_k=64, device=0)
    ix.load(rows)
    m = Model(oracle_mod, rows)
    first = np.union1d(np.flatnonzero(np.random.default_rng(1).random(N) < 0.3), m.top(qs, 5))
    assert ix.delete(first) == m.delete(first)
    for k in (10, 50):
        want = m.want(qs, k)
        for rep in range(3):
            got = ix.local_top_k(qs, k)
            st = ix.last_stats()
            _same(got, want, ("replay", k, rep))
            assert st.n_exact_direct == 0 and not st.search_path & bsr_mod.BSR_PATH_MASK_LIST
        assert st.graph_replay == 1, k
        # the stale-graph case: each query's new top-2 goes
        top2 = m.top(qs, 2)
        assert ix.delete(top2) == m.delete(top2) == len(top2)
        want = m.want(qs, k)
        for rep in range(3):
            got = ix.local_top_k(qs, k)
            st = ix.last_stats()
            _same(got, want, ("after delete", k, rep))
            if rep == 0:
                assert st.graph_replay == 0
        assert st.graph_replay == 1, k
    _check_state(ix, m)
    ix.close()


@pytest.fixture(scope="module")
def shard30(bsr_mod, oracle_mod, base):
    """The shard with 30% of its rows deleted at random plus the top-5 of every query."""
    rows, qs = base
    ix = bsr_mod.Index(D, max_k=256, device=0)
    ix.load(rows)
    m = Model(oracle_mod, rows)
    ids = np.union1d(np.flatnonzero(np.random.default_rng(2).random(N) < 0.3), m.top(qs, 5))
    assert ix.delete(ids) == m.delete(ids)
    yield ix, m, qs
    ix.close()


@pytest.mark.parametrize("nq", [1, 7, 16])
@pytest.mark.parametrize("k", [1, 10])
def test_tiny_batches(bsr_mod, shard30, nq, k):
    """Batches of <= 16 queries: the skinny filter and k_rescore_kp on the thresholded path."""
    ix, m, qs = shard30
    want = m.want(qs[:nq], k)
    for rep in range(3):
        got = ix.local_top_k(qs[:nq], k)
        _same(got, want, ("tiny", nq, k, rep))
    st = ix.last_stats()
    assert st.graph_replay == 1 and st.n_exact_direct == 0
    assert not st.search_path & bsr_mod.BSR_PATH_SKINNY_TOP


def test_zero_query_fallback(bsr_mod, shard30):
    """A zero query is not served by the filter: the list scan over the live rows answers it."""
    ix, m, qs = shard30
    q = qs[:6].copy()
    q[3] = 0.0
    got = ix.local_top_k(q, 10)
    st = ix.last_stats()
    _same(got, m.want(q, 10), "zero query")
    assert st.n_exact_direct == 1


@pytest.mark.parametrize("k", [201, 256])
def test_large_k_fallback(bsr_mod, shard30, k):
    """k > 200: no filter, every query by the list scan over the live rows."""
    ix, m, qs = shard30
    got = ix.local_top_k(qs[:9], k)
    st = ix.last_stats()
    _same(got, m.want(qs[:9], k), ("large k", k))
    assert st.n_exact_direct == 9 and st.graph_replay == 0


def test_exact_only_fallback(bsr_mod, oracle_mod, base):
    rows, qs = base
    n = 9_001
    ix = bsr_mod.Index(D, max_k=64, device=0, flags=bsr_mod.BSR_FLAG_EXACT_ONLY)
    ix.load(rows[:n])
    m = Model(oracle_mod, rows[:n])
    ids = np.flatnonzero(np.random.default_rng(3).random(n) < 0.3)
    assert ix.delete(ids) == m.delete(ids)
    for nq in (3, 11):
        got = ix.local_top_k(qs[:nq], 10)
        _same(got, m.want(qs[:nq], 10), ("exact only", nq))
        assert ix.last_stats().n_exact_direct == nq
    ix.close()


@pytest.mark.parametrize("mode", ["list", "filter"])
def test_masked_and_tombstones(bsr_mod, shard30, mode):
    """A masked search on an index with tombstones answers over allow & ~dead."""
    ix, m, qs = shard30
    allow = np.random.default_rng(4).random(N) < 0.5
    want = m.want(qs, 10, allow=allow)
    got = ix.local_top_k(qs, 10, allow_mask=allow, mask_mode=mode)
    st = ix.last_stats()
    _same(got, want, ("masked", mode))
    bit = bsr_mod.BSR_PATH_MASK_LIST if mode == "list" else bsr_mod.BSR_PATH_MASK_FILTER
    assert st.search_path & bit, st.search_path
    if mode == "filter":
        # (the threshold lowered by live / A: the lists do not overflow into the list scan)
        assert st.n_fallback + st.n_exact_direct < len(qs), (st.n_fallback, st.n_exact_direct)
    # the plain search is untouched by the masked one
    _same(ix.local_top_k(qs, 10), m.want(qs, 10), "plain after masked")


# ---- 3. sample tiles ----------------------------------------------------------------------------
def test_sample_tiles(bsr_mod, oracle_mod, gpu):
    """n >= 65,505: batches of more than 16 queries sample whole tiles of the operand.  Three whole
    sample tiles (rows 128 (32 L + 31) ... + 127) are deleted with a 20% random set."""
    rng = np.random.default_rng(33)
    n, nq, k = 70_001, 40, 10
    rows = rng.uniform(-1, 1, (n, D)).astype(np.float32)
    qs = rng.uniform(-1, 1, (nq, D)).astype(np.float32)
    ix = bsr_mod.Index(D, max_k=64, device=0)
    ix.load(rows)
    m = Model(oracle_mod, rows)
    tiles = np.concatenate([128 * (32 * L + 31) + np.arange(128) for L in range(3)])
    ids = np.union1d(tiles, np.flatnonzero(rng.random(n) < 0.2))
    assert ix.delete(ids) == m.delete(ids)
    want = m.want(qs, k)
    for rep in range(3):
        _same(ix.local_top_k(qs, k), want, ("sample tiles", rep))
    st = ix.last_stats()
    assert st.n_exact_direct == 0 and st.graph_replay == 1
    ix.close()


# ---- 5. the self-thresholded path at its smallest shard ----------------------------------------
def test_self_thresholded_path(bsr_mod, oracle_mod, gpu):
    import torch
    n, dim, k = (1 << 21) + 1000, 64, 10
    dev = torch.empty((n, dim), dtype=torch.float32, device="cuda:0")
    bsr_mod.synth_uniform(dev.data_ptr(), 0, n, dim, 51)
    qd = torch.empty((13, dim), dtype=torch.float32, device="cuda:0")
    bsr_mod.synth_uniform(qd.data_ptr(), 0, 13, dim, 52)
    torch.cuda.synchronize()
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(dev)
    rows, qs = dev.cpu().numpy(), qd.cpu().numpy()
    del dev
    torch.cuda.empty_cache()
    m = Model(oracle_mod, rows)
    ids = np.union1d(np.flatnonzero(np.random.default_rng(5).random(n) < 0.1), m.top(qs, 5))
    assert ix.delete(torch.from_numpy(ids).to("cuda:0")) == m.delete(ids)
    for nq in (1, 13):
        want = m.want(qs[:nq], k)
        for rep in range(3):
            got = ix.local_top_k(qs[:nq], k)
            st = ix.last_stats()
            assert st.search_path & bsr_mod.BSR_PATH_SKINNY_TOP, st.search_path
            _same(got, want, ("top", nq, rep))
        assert st.graph_replay == 1
    ix.close()


# ---- 6. the operand is really zeroed ------------------------------------------------------------
def test_operand_zeroed(bsr_mod, oracle_mod, gpu):
    """Even rows: exact copies of the queries (500 each); odd rows: U(-1, 1).  With every even row
    deleted the index must answer as the odd rows alone do, without a fallback: were the deleted
    rows still in the operand, tau0 would sit at the copies, no live row would be emitted and every
    query would fall back.  (Every row the fop_s sample reads -- every 32nd -- is even: the sample
    must take live rows in their place.)"""
    rng = np.random.default_rng(34)
    n, nq, k = 40_000, 40, 10
    qs = rng.uniform(-1, 1, (nq, D)).astype(np.float32)
    rows = rng.uniform(-1, 1, (n, D)).astype(np.float32)
    even = np.arange(0, n, 2)
    rows[even] = qs[(even // 2) % nq]
    odd = np.ascontiguousarray(rows[1::2])
    ctl = bsr_mod.Index(D, max_k=64, device=0)
    ctl.load(odd)
    ctl.local_top_k(qs, k)
    assert ctl.last_stats().n_fallback == 0, "precondition: the odd rows alone need no fallback"
    ctl.close()
    ix = bsr_mod.Index(D, max_k=64, device=0)
    ix.load(rows)
    m = Model(oracle_mod, rows)
    assert ix.delete(even) == m.delete(even) == n // 2
    got = ix.local_top_k(qs, k)
    st = ix.last_stats()
    print(f"zeroed operand: fallback={st.n_fallback} rescued={st.n_rescued} emitted={st.n_emitted}")
    _same(got, m.want(qs, k), "operand zeroed")
    assert st.n_fallback == 0 and st.n_exact_direct == 0
    ix.close()


# ---- the dead bit in the rescore kernels: deleted rows that ARE candidates ------------------------
@pytest.fixture(scope="module")
def halfspace(bsr_mod, oracle_mod, gpu):
    """Corpus and queries in opposite half-spaces: rows >= 0 (a quarter of the entries U(0, 1), the
    rest 0), queries <= 0, so every cosine is negative and tau0 < 0.  A deleted row scores exactly 0
    >= tau0: it IS emitted, as the best candidate of every query, and rescored with its real
    distance -- for the deleted true neighbours a winning one.  Only the bit read in k_rescore /
    k_rescore_kp removes it.  Deleted: at most every query's top-2 and 20 more rows, about 100 --
    few enough that the emptied sample slots (one per 32 deleted rows, scoring 0) stay below
    ks = 8 and tau0 stays negative."""
    rng = np.random.default_rng(36)
    rows = (rng.uniform(0, 1, (N, D)) * (rng.random((N, D)) < 0.25)).astype(np.float32)
    qs = -(rng.uniform(0, 1, (40, D)) * (rng.random((40, D)) < 0.25)).astype(np.float32)
    assert (rows[:2000] @ qs.T).max() < 0
    out = {}
    # "many": more deleted rows than the first pass selects (k' = 63): it sees deleted rows alone
    # and the second chance answers.  "few": the top-2 of 17 queries only, which share the first
    # pass's selection with live rows.
    for name, nq_top, extra in (("many", 40, 20), ("few", 17, 0)):
        m = Model(oracle_mod, rows)
        ids = np.union1d(m.top(qs[:nq_top], 2), rng.choice(N, extra, replace=False)).astype(np.int64)
        m.delete(ids)
        ctl = bsr_mod.Index(D, max_k=64, device=0)
        ctl.load(np.ascontiguousarray(rows[m.live()]))
        ctl.local_top_k(qs, 10)
        assert ctl.last_stats().n_fallback == 0, "precondition: the live rows alone need no fallback"
        ctl.close()
        ix = bsr_mod.Index(D, max_k=64, device=0)
        ix.load(rows)
        assert ix.delete(ids) == len(ids)
        out[name] = (ix, m)
    yield out, qs
    for ix, _ in out.values():
        ix.close()


@pytest.mark.parametrize("which,nq,k", [("many", 40, 10), ("many", 16, 10), ("many", 7, 10), ("many", 1, 10),
                                        ("many", 7, 1), ("few", 17, 10), ("few", 7, 10)])
def test_deleted_candidates_dropped_by_the_bit(bsr_mod, halfspace, which, nq, k):
    """17 and 40 queries: k_rescore; 1, 7, 16: k_rescore_kp.  No fallback and no direct scan, so that
    the list scan (whose list holds no deleted row) cannot stand in for the rescore."""
    out, qs = halfspace
    ix, m = out[which]
    got = ix.local_top_k(qs[:nq], k)
    st = ix.last_stats()
    print(f"half-space {which} nq={nq} k={k}: deleted={int(m.dead.sum())} emitted={st.n_emitted} "
          f"rescued={st.n_rescued} fallback={st.n_fallback}")
    _same(got, m.want(qs[:nq], k), ("half-space", which, nq, k))
    assert st.n_fallback == 0 and st.n_exact_direct == 0
    assert not st.search_path & bsr_mod.BSR_PATH_SKINNY_TOP


# ---- 8. append after delete, load clears ----------------------------------------------------------
def test_append_keeps_load_clears(bsr_mod, oracle_mod, gpu):
    rng = np.random.default_rng(35)
    n, extra, dim, k = 3001, 500, 100, 10
    rows = rng.uniform(-1, 1, (n + extra, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (5, dim)).astype(np.float32)
    qs[4] = rows[n + 123]  # a self-query on an appended row
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(rows[:n])
    m = Model(oracle_mod, rows)
    m.dead[n:] = True  # (not there yet)
    ids = np.flatnonzero(rng.random(n) < 0.3)
    assert ix.delete(ids) == len(ids)
    m.dead[ids] = True
    _same(ix.local_top_k(qs, k), m.want(qs, k), "before append")
    ix.append_many(rows[n:])
    m.dead[n:] = False
    _check_state(ix, m)
    assert ix.live_count() == n + extra - len(ids)
    got = ix.local_top_k(qs, k)
    _same(got, m.want(qs, k), "after append")
    assert got[0][4, 0] == n + 123 and got[1][4, 0] == 0.0
    # the appended rows can be deleted too
    assert ix.delete([n + 123, 2]) == m.delete([n + 123, 2])
    _same(ix.local_top_k(qs, k), m.want(qs, k), "appended row deleted")
    ix.load(rows[:n])
    m = Model(oracle_mod, rows[:n])
    _check_state(ix, m)
    assert ix.live_count() == n
    _same(ix.local_top_k(qs, k), m.want(qs, k), "after load")
    ix.close()


# ---- 10. the parallel search ----------------------------------------------------------------------
@pytest.mark.parametrize("comm_kind", ["none", "loopback-8", "forced-one-rank"])
def test_parallel(bsr_mod, oracle_mod, base, monkeypatch, comm_kind):
    """With a deleted row the parallel search takes the standard path (each rank's certified top-k
    over its live rows, the all-gather, the merge); a load clears the tombstones and the
    global-threshold path is taken again."""
    rows, qs = base
    k = 10
    ix = bsr_mod.Index(D, max_k=64, device=0)
    ix.load(rows)
    m = Model(oracle_mod, rows)
    ids = np.union1d(np.flatnonzero(np.random.default_rng(6).random(N) < 0.3), m.top(qs, 5))
    assert ix.delete(ids) == m.delete(ids)
    comm = None
    if comm_kind == "loopback-8":
        comm = bsr_mod.Comm.loopback(0, 8, 0)  # (no script: every slot is this rank's own list)
    elif comm_kind == "forced-one-rank":
        monkeypatch.setenv("BSR_FORCE_COLLECTIVES", "1")
        comm = bsr_mod.Comm(bsr_mod.Comm.unique_id(), 0, 1, 0)
    want = m.want(qs, k)
    for rep in range(2):
        got = bsr_mod.parallel_top_k_similarity_search_batch(comm, ix, qs, k)
        st = ix.last_stats()
        _same(got, want, (comm_kind, rep))
        assert not st.search_path & bsr_mod.BSR_PATH_GLOBAL_TAU, st.search_path
        if comm is not None:
            assert st.search_path & bsr_mod.BSR_PATH_COLLECTIVE, st.search_path
    ix.load(rows)
    got = bsr_mod.parallel_top_k_similarity_search_batch(comm, ix, qs, k)
    st = ix.last_stats()
    _same(got, Model(oracle_mod, rows).want(qs, k), (comm_kind, "after load"))
    if comm is not None:
        assert st.search_path & bsr_mod.BSR_PATH_GLOBAL_TAU, st.search_path
    if comm is not None:
        comm.close()
    ix.close()
