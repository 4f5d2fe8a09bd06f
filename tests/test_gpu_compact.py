"""Compaction (bsr_index_compact): the deleted rows of a loaded shard dropped on the
device.  Afterwards the index must be what a fresh index is after a load of the live rows at the
new offset.  The expected result everywhere is the reference's compute_local_top_k
(src/mpi_helpers/metrics.rs:16-53) over rows[live] with the indices new_offset + j: counts,
indices, order, f32 distance bits and the (~0, +inf) tail.  No tolerances."""
import ctypes

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


def _want(oracle_mod, host, ids, qs, k, offset=0, packed=False):
    """The reference's local top-k over the rows host[ids] (ids ascending).  Global indices: offset
    + ids (rows that keep their place), or offset + the position in ids (packed: after a compaction)."""
    ids = np.asarray(ids, np.int64)
    nq = len(qs)
    if len(ids) == 0:
        return (np.full((nq, k), NONE_IDX), np.full((nq, k), np.inf, np.float32), np.zeros(nq, np.uint32))
    wi, wd, wc = oracle_mod.parallel_top_k(np.ascontiguousarray(host[ids]), np.ascontiguousarray(qs), k,
                                           size=THREADS, threads=THREADS)
    gi = np.full((nq, k), NONE_IDX)
    for q in range(nq):
        c = int(wc[q])
        pos = wi[q, :c].astype(np.int64)
        gi[q, :c] = (pos if packed else ids[pos]).astype(np.uint64) + np.uint64(offset)
    return gi, wd, wc


def _shifted(want, offset):
    wi, wd, wc = want
    gi = wi.copy()
    gi[gi != NONE_IDX] += np.uint64(offset)
    return gi, wd, wc


def _check_packed(ix, rows_live, offset):
    """The state a load of rows_live at `offset` leaves."""
    assert ix.get_count() == ix.live_count() == len(rows_live)
    assert ix.global_offset() == offset
    assert not ix.deleted_mask().any()
    got = ix.get_many()
    assert got.shape == rows_live.shape
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(rows_live).view(np.uint32))


# ---- 1. move patterns at a small, odd shape, about 12 chunks ---------------------------------------
SN, SD, SOFF, SNEW = 3001, 100, 1000, 77
CHUNK_BYTES = 256 * 128 * 4  # 256 rows of ld = 128 floats


@pytest.fixture(scope="module")
def small(gpu, oracle_mod):
    rng = np.random.default_rng(141)
    rows = rng.uniform(-1, 1, (SN, SD)).astype(np.float32)
    qs = rng.uniform(-1, 1, (5, SD)).astype(np.float32)
    top3 = _want(oracle_mod, rows, np.arange(SN), qs[:1], 3)[0][0].astype(np.int64)
    return rows, qs, top3


def _pattern(name, top3):
    n = SN
    if name == "row0":       # displacement 1: every destination is its neighbour's source
        return np.array([0])
    if name == "prefix":
        return np.arange(1500)
    if name == "even":
        return np.arange(0, n, 2)
    if name == "last":       # no move: tail zeroing only
        return np.array([3000])
    if name == "tail":
        return np.arange(2944, 3001)
    if name == "but3":
        return np.setdiff1d(np.arange(n), [7, 1500, 3000])
    if name == "all":
        return np.arange(n)
    assert name == "rand30"
    return np.union1d(np.flatnonzero(np.random.default_rng(142).random(n) < 0.3), top3)


@pytest.mark.parametrize("name", ["row0", "prefix", "even", "last", "tail", "but3", "all", "rand30"])
def test_move_patterns(bsr_mod, oracle_mod, small, monkeypatch, name):
    import torch
    rows, qs, top3 = small
    if name != "rand30":  # (rand30: the default staging size, one chunk)
        monkeypatch.setenv("BSR_COMPACT_STAGE_BYTES", str(CHUNK_BYTES))
    dead = _pattern(name, top3)
    live = np.setdiff1d(np.arange(SN), dead)
    ix = bsr_mod.Index(SD, max_k=64, device=0)
    ix.load(rows, global_offset=SOFF)
    assert ix.delete(dead + SOFF) == len(dead)
    if name == "even":  # the id map into device memory, through the C entry point
        out = torch.full((len(live),), -1, dtype=torch.int64, device="cuda:0")
        cnt = ctypes.c_uint64(0)
        st = bsr_mod.lib().bsr_index_compact(ix._h, SNEW, 0, out.data_ptr(), len(live), ctypes.byref(cnt))
        assert st == 0, bsr_mod.lib().bsr_last_error()
        assert cnt.value == len(live)
        ids = out.cpu().numpy().astype(np.uint64)
    else:
        ids = ix.compact(global_offset=SNEW)
    assert ids.dtype == np.uint64 and np.array_equal(ids, (live + SOFF).astype(np.uint64)), name
    _check_packed(ix, rows[live], SNEW)
    want = _want(oracle_mod, rows, live, qs, 10, SNEW, packed=True)
    for rep in range(2):
        _same(ix.local_top_k(qs, 10), want, (name, rep))
    if len(live) == 0:
        assert np.all(ix.local_top_k(qs, 10)[2] == 0)
    ix.close()


# ---- 2. capacity and state errors: all or nothing ---------------------------------------------------
def test_errors_change_nothing(bsr_mod, oracle_mod, small):
    rows, qs, top3 = small
    L = bsr_mod.lib()
    ix = bsr_mod.Index(SD, max_k=64, device=0)
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.compact()
    assert e.value.status == E_STATE
    assert L.bsr_index_compact(ix._h, 0, 0, None, 0, None) == E_STATE
    ix.load(rows, global_offset=SOFF)
    dead = _pattern("rand30", top3)
    live = np.setdiff1d(np.arange(SN), dead)
    assert ix.delete(dead + SOFF) == len(dead)
    want = _want(oracle_mod, rows, live, qs, 10, SOFF)
    mask = np.zeros(SN, bool)
    mask[dead] = True

    def unchanged(ctx):
        assert ix.get_count() == SN and ix.live_count() == len(live) and ix.global_offset() == SOFF, ctx
        assert np.array_equal(ix.deleted_mask(), mask), ctx
        assert np.array_equal(ix.get_many(), rows), ctx
        _same(ix.local_top_k(qs, 10), want, ctx)

    unchanged("before")
    out = np.full(len(live), 12345, np.uint64)
    cnt = ctypes.c_uint64(99)
    assert L.bsr_index_compact(ix._h, SNEW, 0, out.ctypes.data, len(live) - 1, ctypes.byref(cnt)) == E_INVALID
    assert b"out_capacity" in L.bsr_last_error()
    assert cnt.value == 99 and np.all(out == 12345)
    unchanged("capacity")
    for flags in (2, 0x80000000, 3):
        assert L.bsr_index_compact(ix._h, SNEW, flags, None, 0, None) == E_INVALID, flags
    unchanged("flags")
    for bad in (2 ** 64 - len(live), 2 ** 64 - 1):  # (offset + live = 2^64: the last id would be ~0)
        assert L.bsr_index_compact(ix._h, bad, 0, None, 0, None) == E_INVALID
    unchanged("overflow")
    # (the largest offset whose sum fits is legal; NULL ids: the capacity is ignored)
    assert L.bsr_index_compact(ix._h, 2 ** 64 - 1 - len(live), 0, None, 0, ctypes.byref(cnt)) == 0
    assert cnt.value == len(live) and ix.global_offset() == 2 ** 64 - 1 - len(live)
    assert ix.get_count() == ix.live_count() == len(live)
    ix.close()


# ---- 3, 4, 8: one shard of 40,037 x 768 uniform rows, 30% + every query's top-5 deleted --------------
N, D = 40_037, 768


@pytest.fixture(scope="module")
def base(gpu, oracle_mod):
    rng = np.random.default_rng(143)
    rows = rng.uniform(-1, 1, (N, D)).astype(np.float32)
    qs = rng.uniform(-1, 1, (40, D)).astype(np.float32)
    wi, _, wc = _want(oracle_mod, rows, np.arange(N), qs, 5)
    top5 = np.unique(np.concatenate([wi[q, :int(wc[q])] for q in range(len(qs))]).astype(np.int64))
    dead = np.union1d(np.flatnonzero(np.random.default_rng(144).random(N) < 0.3), top5)
    live = np.setdiff1d(np.arange(N), dead)
    live_rows = np.ascontiguousarray(rows[live])
    want = {k: _want(oracle_mod, live_rows, np.arange(len(live)), qs, k) for k in (10, 50)}  # (offset 0)
    return dict(rows=rows, qs=qs, dead=dead, live=live, live_rows=live_rows, want=want)


def test_same_as_fresh_load_on_the_filter_path(bsr_mod, base):
    qs, live = base["qs"], base["live"]
    off = 4242
    ix = bsr_mod.Index(D, max_k=64, device=0)
    ix.load(base["rows"])
    assert ix.delete(base["dead"]) == len(base["dead"])
    ix.local_top_k(qs, 10)  # (graphs of the tombstoned shard exist before the compaction)
    ix.local_top_k(qs, 10)
    ids = ix.compact(global_offset=off)
    assert np.array_equal(ids, live.astype(np.uint64))
    _check_packed(ix, base["live_rows"], off)
    fresh = bsr_mod.Index(D, max_k=64, device=0)
    fresh.load(base["live_rows"], global_offset=off)
    for k in (10, 50):
        want = _shifted(base["want"][k], off)
        ref = fresh.local_top_k(qs, k)
        fst = fresh.last_stats()
        _same(ref, want, ("fresh", k))
        for rep in range(3):
            got = ix.local_top_k(qs, k)
            st = ix.last_stats()
            _same(got, want, ("compacted", k, rep))
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
            assert np.float32(st.row_ebound).view(np.uint32) == np.float32(fst.row_ebound).view(np.uint32)
            assert st.n_exact_direct == 0
        assert st.graph_replay == 1, k
    fresh.close()
    ix.close()


def test_stale_graph_on_an_offset_only_compact(bsr_mod, base):
    """The offset is a kernel argument a captured graph bakes in: a compaction that changes only the
    offset must not be answered from the old graph."""
    rows, qs, k = base["rows"][:20_011], base["qs"], 10
    old = 300
    ix = bsr_mod.Index(D, max_k=64, device=0)
    ix.load(rows, global_offset=old)
    for rep in range(3):
        before = ix.local_top_k(qs, k)
    assert ix.last_stats().graph_replay == 1
    ids = ix.compact(global_offset=old + 5000)
    assert np.array_equal(ids, np.arange(len(rows), dtype=np.uint64) + np.uint64(old))
    assert ix.global_offset() == old + 5000 and ix.get_count() == len(rows)
    want = _shifted(before, 5000)
    for rep in range(3):
        got = ix.local_top_k(qs, k)
        st = ix.last_stats()
        _same(got, want, ("offset only", rep))
        if rep == 0:
            assert st.graph_replay == 0
    assert st.graph_replay == 1
    # no tombstones, the same offset: a no-op, the graphs replay on
    for off in (None, old + 5000):
        ids = ix.compact(global_offset=off)
        assert np.array_equal(ids, np.arange(len(rows), dtype=np.uint64) + np.uint64(old + 5000))
        got = ix.local_top_k(qs, k)
        assert ix.last_stats().graph_replay == 1, off
        _same(got, want, ("no-op", off))
    ix.close()


@pytest.mark.parametrize("comm_kind", ["none", "loopback-8", "forced-one-rank"])
def test_parallel(bsr_mod, base, monkeypatch, comm_kind):
    """With tombstones the parallel search takes the standard path; a compaction makes the shard
    eligible for the global-threshold path again."""
    qs, k, off = base["qs"], 10, 123
    ix = bsr_mod.Index(D, max_k=64, device=0)
    ix.load(base["rows"])
    assert ix.delete(base["dead"]) == len(base["dead"])
    comm = None
    if comm_kind == "loopback-8":
        comm = bsr_mod.Comm.loopback(0, 8, 0)
    elif comm_kind == "forced-one-rank":
        monkeypatch.setenv("BSR_FORCE_COLLECTIVES", "1")
        comm = bsr_mod.Comm(bsr_mod.Comm.unique_id(), 0, 1, 0)
    bsr_mod.parallel_top_k_similarity_search_batch(comm, ix, qs, k)
    assert not ix.last_stats().search_path & bsr_mod.BSR_PATH_GLOBAL_TAU
    ids = ix.compact(global_offset=off)
    assert np.array_equal(ids, base["live"].astype(np.uint64))
    want = _shifted(base["want"][k], off)
    for rep in range(2):
        got = bsr_mod.parallel_top_k_similarity_search_batch(comm, ix, qs, k)
        st = ix.last_stats()
        _same(got, want, (comm_kind, rep))
        if comm is not None:
            assert st.search_path & bsr_mod.BSR_PATH_GLOBAL_TAU, st.search_path
            assert st.search_path & bsr_mod.BSR_PATH_COLLECTIVE, st.search_path
    if comm is not None:
        comm.close()
    ix.close()


# ---- 5. the lifecycle after a compaction -------------------------------------------------------------
class Model:
    """The numpy model of an index: its rows, the dead bits, the offset."""

    def __init__(self, oracle_mod, rows, offset):
        self.oracle, self.rows, self.offset = oracle_mod, rows.copy(), offset
        self.dead = np.zeros(len(rows), bool)

    def live(self):
        return np.flatnonzero(~self.dead)

    def want(self, qs, k, allow=None):
        keep = ~self.dead if allow is None else (~self.dead & allow)
        return _want(self.oracle, self.rows, np.flatnonzero(keep), qs, k, self.offset)

    def compact(self, offset):
        """-> the old global ids."""
        live = self.live()
        ids = (live + self.offset).astype(np.uint64)
        self.rows, self.offset, self.dead = np.ascontiguousarray(self.rows[live]), offset, np.zeros(len(live), bool)
        return ids


@pytest.mark.parametrize("shrink", [False, True])
def test_lifecycle_after_compact(bsr_mod, oracle_mod, small, monkeypatch, shrink):
    monkeypatch.setenv("BSR_COMPACT_STAGE_BYTES", str(CHUNK_BYTES))
    rows, qs, top3 = small
    rng = np.random.default_rng(145)
    k = 10
    ix = bsr_mod.Index(SD, max_k=64, device=0)
    ix.load(rows, global_offset=SOFF)
    m = Model(oracle_mod, rows, SOFF)
    dead = _pattern("rand30", top3)
    assert ix.delete(dead + SOFF) == len(dead)
    m.dead[dead] = True
    assert np.array_equal(ix.compact(global_offset=SNEW, shrink=shrink), m.compact(SNEW))
    _check_packed(ix, m.rows, SNEW)
    _same(ix.local_top_k(qs, k), m.want(qs, k), "compacted")

    def check(ctx):
        assert ix.get_count() == len(m.rows) and ix.live_count() == len(m.live()), ctx
        assert np.array_equal(ix.deleted_mask(), m.dead), ctx
        assert np.array_equal(ix.get_many(), m.rows), ctx
        _same(ix.local_top_k(qs, k), m.want(qs, k), ctx)

    # delete, by the new ids: query 1's top-2 and 10% at random
    top2 = m.want(qs[1:2], 2)[0][0].astype(np.int64) - SNEW
    gone = np.union1d(top2, np.flatnonzero(rng.random(len(m.rows)) < 0.1))
    assert ix.delete(gone + SNEW) == len(gone)
    m.dead[gone] = True
    check("delete after compact")
    # update of two rows (one of them a self-query's target)
    upd = np.array([3, len(m.rows) - 1])
    new = rng.uniform(-1, 1, (2, SD)).astype(np.float32)
    new[0] = qs[2]
    ix.update(upd + SNEW, new)
    m.rows[upd] = new
    check("update after compact")
    # append: without shrink the slab is not regrown, so the rows land on the pad rows the
    # compaction left
    n0 = len(m.rows)
    extra = rng.uniform(-1, 1, (300, SD)).astype(np.float32)
    extra[17] = qs[3]
    ix.append_many(extra)
    m.rows = np.concatenate([m.rows, extra])
    m.dead = np.concatenate([m.dead, np.zeros(300, bool)])
    check("append after compact")
    got = ix.local_top_k(qs, k)
    assert got[0][3, 0] == SNEW + n0 + 17 and got[1][3, 0] == 0.0
    fresh = bsr_mod.Index(SD, max_k=64, device=0)
    fresh.load(m.rows, global_offset=SNEW)
    fresh.delete(np.flatnonzero(m.dead) + SNEW)
    ref = fresh.local_top_k(qs, k)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
    assert np.array_equal(got[2], ref[2])
    fresh.close()
    # masked and grouped searches
    allow_ids = np.flatnonzero(rng.random(len(m.rows)) < 0.5)
    allow = np.zeros(len(m.rows), bool)
    allow[allow_ids] = True
    _same(ix.local_top_k(qs, k, allow_ids=allow_ids), m.want(qs, k, allow=allow), "masked after compact")
    masks = rng.random((3, len(m.rows))) < np.array([0.7, 0.2, 0.01])[:, None]
    qm = np.array([0, 1, 2, 1, 0])
    got = ix.local_top_k_grouped(qs, k, masks, qm)
    for g in range(3):
        sel = np.flatnonzero(qm == g)
        _same(tuple(a[sel] for a in got), m.want(qs[sel], k, allow=masks[g]), ("grouped after compact", g))
    # a second compaction, rebased
    assert np.array_equal(ix.compact(global_offset=5, shrink=shrink), m.compact(5))
    _check_packed(ix, m.rows, 5)
    check("second compact")
    ix.close()


# ---- 6. a bf16 index and an exact-only index ---------------------------------------------------------
def test_bf16_index(bsr_mod, oracle_mod, gpu, monkeypatch):
    monkeypatch.setenv("BSR_COMPACT_STAGE_BYTES", str(CHUNK_BYTES))
    rng = np.random.default_rng(146)
    n, dim, k = 5003, 128, 10
    bits = (rng.uniform(-1, 1, (n, dim)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    wide = (bits.astype(np.uint32) << 16).view(np.float32)
    qs = rng.uniform(-1, 1, (7, dim)).astype(np.float32)
    ix = bsr_mod.Index(dim, max_k=64, device=0, dtype=bsr_mod.BSR_BF16)
    ix.load(bits, global_offset=9)
    dead = np.flatnonzero(rng.random(n) < 0.4)
    live = np.setdiff1d(np.arange(n), dead)
    assert ix.delete(dead + 9) == len(dead)
    assert np.array_equal(ix.compact(), (live + 9).astype(np.uint64))
    _check_packed(ix, wide[live], 9)
    want = _want(oracle_mod, wide, live, qs, k, 9, packed=True)
    for rep in range(3):
        _same(ix.local_top_k(qs, k), want, ("bf16", rep))
    fresh = bsr_mod.Index(dim, max_k=64, device=0, dtype=bsr_mod.BSR_BF16)
    fresh.load(np.ascontiguousarray(bits[live]), global_offset=9)
    _same(fresh.local_top_k(qs, k), want, "bf16 fresh")
    assert (np.float32(fresh.last_stats().row_ebound).view(np.uint32)
            == np.float32(ix.last_stats().row_ebound).view(np.uint32))
    fresh.close()
    ix.close()


def test_exact_only_index(bsr_mod, oracle_mod, base, monkeypatch):
    monkeypatch.setenv("BSR_COMPACT_STAGE_BYTES", str(1 << 20))
    n, k = 9_001, 10
    rows, qs = base["rows"][:n], base["qs"]
    ix = bsr_mod.Index(D, max_k=64, device=0, flags=bsr_mod.BSR_FLAG_EXACT_ONLY)
    ix.load(rows)
    dead = np.flatnonzero(np.random.default_rng(147).random(n) < 0.4)
    live = np.setdiff1d(np.arange(n), dead)
    assert ix.delete(dead) == len(dead)
    assert np.array_equal(ix.compact(global_offset=31), (live).astype(np.uint64))
    _check_packed(ix, rows[live], 31)
    for nq in (3, 11):
        got = ix.local_top_k(qs[:nq], k)
        _same(got, _want(oracle_mod, rows, live, qs[:nq], k, 31, packed=True), ("exact only", nq))
        assert ix.last_stats().n_exact_direct == nq
    ix.close()


# ---- 7. the self-thresholded path at its smallest shard ----------------------------------------------
def test_top_path(bsr_mod, gpu):
    """live >= 2^21 rows after the compaction: batches of <= 16 queries take the self-thresholded
    path; the compacted index answers as a fresh index of the live rows does."""
    import torch
    n, dim, k, off = (1 << 21) + 3000, 64, 10, 17
    dev = torch.empty((n, dim), dtype=torch.float32, device="cuda:0")
    bsr_mod.synth_uniform(dev.data_ptr(), 0, n, dim, 151)
    qd = torch.empty((16, dim), dtype=torch.float32, device="cuda:0")
    bsr_mod.synth_uniform(qd.data_ptr(), 0, 16, dim, 152)
    torch.cuda.synchronize()
    qs = qd.cpu().numpy()
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(dev)
    # deleted: every query's current top-3, rows 0 and n - 1, and 1 row in 1024 at random
    top = np.unique(ix.local_top_k(qs, 3)[0].astype(np.int64))
    dead = np.union1d(np.union1d(top, [0, n - 1]), np.flatnonzero(np.random.default_rng(153).random(n) < 1 / 1024))
    live = np.setdiff1d(np.arange(n), dead)
    assert len(live) >= 1 << 21
    assert ix.delete(torch.from_numpy(dead).to("cuda:0")) == len(dead)
    ids = ix.compact(global_offset=off)
    assert np.array_equal(ids, live.astype(np.uint64))
    live_dev = dev.index_select(0, torch.from_numpy(live).to("cuda:0"))
    del dev
    torch.cuda.synchronize()
    fresh = bsr_mod.Index(dim, max_k=64, device=0)
    fresh.load(live_dev, global_offset=off)
    assert ix.get_count() == ix.live_count() == fresh.get_count() == len(live)
    for nq in (1, 16):
        ref = fresh.local_top_k(qs[:nq], k)
        assert fresh.last_stats().search_path & bsr_mod.BSR_PATH_SKINNY_TOP
        assert np.all(ref[2] == k)
        for rep in range(3):
            got = ix.local_top_k(qs[:nq], k)
            st = ix.last_stats()
            assert st.search_path & bsr_mod.BSR_PATH_SKINNY_TOP, st.search_path
            _same(got, ref, ("top", nq, rep))
        assert st.graph_replay == 1
        assert not np.isin(ids[got[0].astype(np.int64) - off].astype(np.int64), dead).any()
    fresh.close()
    ix.close()
    del live_dev
    torch.cuda.empty_cache()


# ---- 9. byte offsets beyond 4 GiB ---------------------------------------------------------------------
def test_offsets_beyond_4_gib(bsr_mod, gpu):
    """2^24 + 300 rows of 256 bytes: the slab is 4.3 GB, the last rows lie beyond byte 2^32."""
    import torch
    n, dim, off = (1 << 24) + 300, 16, 5
    free, _ = torch.cuda.mem_get_info(0)
    if free < 12 << 30:
        pytest.skip(f"needs 12 GB of free HBM (about 7 GB are allocated), {free >> 20} MB are free")
    src = torch.empty((n, dim), dtype=torch.float32, device="cuda:0")
    bsr_mod.synth_uniform(src.data_ptr(), 0, n, dim, 161)
    torch.cuda.synchronize()
    ix = bsr_mod.Index(dim, max_k=16, device=0)
    ix.load(src, global_offset=off)
    assert ix.delete(np.array([0, 1, n - 2]) + off) == 3
    ids = ix.compact()
    m = n - 3
    assert len(ids) == m and ix.get_count() == ix.live_count() == m
    assert np.array_equal(ids[:2], np.array([2, 3], np.uint64) + np.uint64(off))
    assert np.array_equal(ids[-3:], np.array([n - 4, n - 3, n - 1], np.uint64) + np.uint64(off))
    head = ix.get_many(bsr_mod.SliceArgs(0, 4))
    assert np.array_equal(head.view(np.uint32), src[2:6].cpu().numpy().view(np.uint32))
    tail = ix.get_many(bsr_mod.SliceArgs(m - 64, 64))
    want = torch.cat([src[n - 66:n - 2], src[n - 1:]])[-64:].cpu().numpy()
    assert np.array_equal(tail.view(np.uint32), want.view(np.uint32))
    ix.close()
    del src
    torch.cuda.empty_cache()
