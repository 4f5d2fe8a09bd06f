"""Range search (bsr_local_range_search) through the C ABI: every live row within
radius[q] of query q, exact.  The expected result everywhere is the reference's own list --
oracle.local_top_k(live rows, 0, 1, top_k = all of them, query) -- cut at distance <= radius:
counts, global indices, order and f32 distance bits, with the (~0, +inf) tail; a count above the
capacity leaves only the tail.  No tolerance anywhere."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
NONE_IDX = np.uint64(2 ** 64 - 1)
E_INVALID, E_NONFINITE, E_STATE = -1, -2, -7
POS_INF, NEG_INF = F(np.inf), F(-np.inf)


# ---- the model ---------------------------------------------------------------------------------
def sorted_lists(oracle_mod, rows, qs):
    """Per query the reference's whole list over `rows`: (local ids, distances), distance ascending
    then id ascending."""
    rows = np.ascontiguousarray(rows, F)
    if len(rows) == 0:
        return [(np.zeros(0, np.uint64), np.zeros(0, F)) for _ in qs]
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda q: oracle_mod.local_top_k(rows, 0, 1, len(rows), q), qs))


def cut(lists, ids, radius, capacity, offset=0):
    """The lists cut at distance <= radius[q]: (idx [nq][capacity], dist, count), global indices
    offset + ids[local]."""
    nq = len(lists)
    idx = np.full((nq, capacity), NONE_IDX)
    dist = np.full((nq, capacity), np.inf, F)
    cnt = np.zeros(nq, np.uint32)
    ids = np.asarray(ids, np.uint64)
    for q, (oi, od) in enumerate(lists):
        r = F(radius[q])
        c = 0 if np.isnan(r) else int(np.searchsorted(od, r, side="right"))
        assert c == int(np.count_nonzero(od <= r))
        cnt[q] = c
        if c <= capacity:
            idx[q, :c] = ids[oi[:c].astype(np.int64)] + np.uint64(offset)
            dist[q, :c] = od[:c]
    return idx, dist, cnt


def same(got, want, ctx):
    gi, gd, gc = got
    wi, wd, wc = want
    assert gi.dtype == np.uint64 and gd.dtype == F and gc.dtype == np.uint32
    assert np.array_equal(gc, wc), (ctx, gc, wc)
    for q in range(len(wc)):
        assert np.array_equal(gi[q], wi[q]), (ctx, q, int(wc[q]))
        assert np.array_equal(gd[q].view(np.uint32), wd[q].view(np.uint32)), (ctx, q)
        c = int(wc[q]) if wc[q] <= gi.shape[1] else 0
        assert len(set(gi[q, :c].tolist())) == c, (ctx, q, "a global index appears twice")
        assert (gi[q, c:] == NONE_IDX).all() and np.isposinf(gd[q, c:]).all(), (ctx, q, "tail")


def kth_radius(lists, ms, below=False):
    """radius[q] = the exact distance of query q's ms[q]-th nearest row (below: one f32 under it)."""
    r = np.array([od[m - 1] for (_, od), m in zip(lists, ms)], F)
    return np.nextafter(r, NEG_INF) if below else r


class Model:
    """The rows of an index on the host, its tombstones and its offset."""

    def __init__(self, oracle_mod, rows, offset=0):
        self.oracle, self.rows, self.offset = oracle_mod, rows.copy(), offset
        self.dead = np.zeros(len(rows), bool)

    def live(self):
        return np.flatnonzero(~self.dead)

    def lists(self, qs):
        return sorted_lists(self.oracle, self.rows[self.live()], qs)

    def want(self, qs, radius, capacity, lists=None):
        return cut(lists or self.lists(qs), self.live(), radius, capacity, self.offset)


# ---- the data ----------------------------------------------------------------------------------
def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def cluster_rows(rng, q, per, lo=0.01, hi=0.12):
    """normalise(q + sigma * noise) with sigma drawn so that the distances spread over about
    [lo, hi]: for q ~ U(-1, 1)^dim, d ~ 1 - 1 / sqrt(1 + 3 sigma^2) ~ 1.5 sigma^2."""
    sigma = np.sqrt(rng.uniform(lo, hi, per) / 1.5)
    v = q.astype(np.float64)[None, :] + sigma[:, None] * rng.standard_normal((per, q.size))
    return unit(v).astype(F)


def rows_at_distance(rng, q, d):
    """Unit rows at cosine distance d[i] of q (to f32 rounding): cos * q^ + sin * u^, u^ orthogonal to q."""
    qh = unit(q.astype(np.float64))
    u = rng.standard_normal((len(d), q.size))
    u = unit(u - (u @ qh)[:, None] * qh[None, :])
    c = 1.0 - np.asarray(d, np.float64)
    return (c[:, None] * qh[None, :] + np.sqrt(1.0 - c * c)[:, None] * u).astype(F)


def make_shard(n, dim, nq, per, seed):
    """Uniform background rows with a planted cluster of `per` rows per query, at random places."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-1, 1, (n, dim)).astype(F)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(F)
    pos = rng.permutation(n)[:nq * per].reshape(nq, per)
    for q in range(nq):
        rows[pos[q]] = cluster_rows(rng, qs[q], per)
    return rows, qs, pos


# ---- 1. the filter path on planted clusters -------------------------------------------------------
SHAPES = {"768": (20011, 768, 40), "130": (8000, 130, 20)}  # n (a partial last tile), dim, cluster rows per query
_shards = {}


def shard(bsr_mod, oracle_mod, name):
    if name not in _shards:
        n, dim, per = SHAPES[name]
        rows, qs, _ = make_shard(n, dim, 300, per, 5 + dim)
        ix = bsr_mod.Index(dim, max_k=64, device=0).load(rows, global_offset=7_000_000_000)
        lists = sorted_lists(oracle_mod, rows, qs)
        ms = [1 + (7 * q) % per for q in range(300)]
        _shards[name] = (ix, rows, qs, lists, ms)
    return _shards[name]


@pytest.mark.parametrize("capacity", [64, 512])
@pytest.mark.parametrize("nq", [3, 16, 17, 300])
@pytest.mark.parametrize("name", list(SHAPES))
def test_filter_path(bsr_mod, oracle_mod, gpu, name, nq, capacity):
    ix, rows, qs, lists, ms = shard(bsr_mod, oracle_mod, name)
    for below in (False, True):
        radius = kth_radius(lists[:nq], ms[:nq], below)
        assert 0 < radius.min() and radius.max() < 0.2
        want = cut(lists[:nq], np.arange(len(rows)), radius, capacity, 7_000_000_000)
        got = ix.range_search(qs[:nq], radius, max_results=capacity)
        st = ix.last_stats()
        print(f"{name} nq={nq} cap={capacity} below={below}: emitted={st.n_emitted} fallback={st.n_fallback} "
              f"direct={st.n_exact_direct} path={st.search_path} E_row={st.row_ebound:.5f} counts<={want[2].max()}")
        same(got, want, (name, nq, capacity, below))
        # the planted data is served by the filter alone: conditions, not measurements
        assert st.search_path & bsr_mod.BSR_PATH_RANGE
        assert not (st.search_path & bsr_mod.BSR_PATH_RANGE_SCAN)
        assert st.n_fallback == 0 and st.n_exact_direct == 0
        assert st.n_queries == nq and st.graph_replay == 0
        assert st.n_emitted >= int(want[2].sum())
        if below:  # the row at the boundary went out: the radius is inclusive to the bit
            assert (want[2] < np.array(ms[:nq])).all()
        else:
            assert (want[2] >= np.array(ms[:nq])).all()


# ---- 2. the overflow ladder: filter -> scan -> count only ------------------------------------------
def test_ladder(bsr_mod, oracle_mod, gpu):
    rng = np.random.default_rng(77)
    n, dim, capacity = 9000, 768, 512
    rows = rng.uniform(-1, 1, (n, dim)).astype(F)
    qs = rng.uniform(-1, 1, (3, dim)).astype(F)
    pos = rng.permutation(n)
    dup, inside, outside, ordinary = pos[:3000], pos[3000:3400], pos[3400:4500], pos[4500:4530]
    rows[dup] = rows_at_distance(rng, qs[0], rng.uniform(0.001, 0.03, 3000))     # 3000 near-duplicates of query 0
    rows[inside] = rows_at_distance(rng, qs[1], rng.uniform(0.02, 0.0999, 400))  # query 1: 400 rows in range ...
    rows[ordinary] = cluster_rows(rng, qs[2], 30)
    ix = bsr_mod.Index(dim, max_k=64, device=0).load(rows)
    ix.range_search(qs[:1], 0.01, max_results=capacity)
    e_row = float(ix.last_stats().row_ebound)
    # ... and 1100 just outside its radius, by a delta the filter cannot resolve: below the int8
    # operand's own error bound, read from the loaded index
    d_hi = min(1e-3, e_row / 2)
    assert d_hi > 1e-4, f"row_ebound {e_row}: no room for a delta of 1e-4"
    rows[outside] = rows_at_distance(rng, qs[1], 0.1 + rng.uniform(1e-4, d_hi, 1100))
    ix.update(outside, rows[outside])
    m = Model(oracle_mod, rows)
    lists = m.lists(qs)
    radius = np.array([0.05, 0.1, lists[2][1][9]], F)
    want = m.want(qs, radius, capacity, lists)
    assert want[2][0] == 3000 and want[2][1] == 400 and want[2][2] >= 10
    got = ix.range_search(qs, radius, max_results=capacity)
    st = ix.last_stats()
    print(f"ladder: E_row={st.row_ebound:.5f} delta<={d_hi:.5f} emitted={st.n_emitted} fallback={st.n_fallback} "
          f"direct={st.n_exact_direct} path={st.search_path}")
    assert d_hi < st.row_ebound
    same(got, want, "ladder")
    assert (got[0][0] == NONE_IDX).all() and got[2][0] == 3000, "count only: exact, with every slot padding"
    assert (got[0][1, :400] != NONE_IDX).all()
    assert st.n_fallback >= 2 and st.n_exact_direct == 0
    assert st.search_path & bsr_mod.BSR_PATH_RANGE and st.search_path & bsr_mod.BSR_PATH_RANGE_SCAN
    # more capacity: the same call returns query 0's rows too
    big = ix.range_search(qs, radius, max_results=4096)
    same(big, m.want(qs, radius, 4096, lists), "ladder, 4096 slots")
    assert (big[0][0, :3000] != NONE_IDX).all()


# ---- 3. the row lifecycle, the pointers, the edge radii -----------------------------------------------
@pytest.fixture(scope="module")
def small(bsr_mod, oracle_mod, gpu):
    n, dim, nq, per = 6000, 130, 6, 40
    rows, qs, pos = make_shard(n, dim, nq, per, 1234)
    rows[17] = qs[1]  # a row identical to query 1
    ix = bsr_mod.Index(dim, max_k=64, device=0).load(rows, global_offset=1000)
    return ix, Model(oracle_mod, rows, 1000), qs, pos


def test_state_isolation(bsr_mod, small):
    """A range search between plain searches: their results and their graph replay are untouched."""
    ix, m, qs, pos = small
    first = None
    for rep in range(3):
        got = ix.local_top_k(qs, 10)
        first = first or got
    assert ix.last_stats().graph_replay == 1
    lists = m.lists(qs)
    radius = kth_radius(lists, [10] * len(qs))
    same(ix.range_search(qs, radius, max_results=64), m.want(qs, radius, 64, lists), "between")
    assert ix.last_stats().graph_replay == 0
    for rep in range(3):
        got = ix.local_top_k(qs, 10)
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[2], first[2]), rep
        assert np.array_equal(got[1].view(np.uint32), first[1].view(np.uint32)), rep
    assert ix.last_stats().graph_replay == 1


def test_edge_radii_on_the_filter_path(bsr_mod, small):
    ix, m, qs, pos = small
    lists = m.lists(qs)
    r5 = lists[5][1][4]
    radius = np.array([-1.0, 0.0, 2.0, np.inf, -0.0, r5], F)
    want = m.want(qs, radius, 64, lists)
    live = len(m.live())
    assert list(want[2][:4]) == [0, 1, live, live] and want[1][1, 0] == 0.0 and want[0][1, 0] == 1017
    got = ix.range_search(qs, radius, max_results=64)
    st = ix.last_stats()
    same(got, want, "edge radii")
    # radii >= 1 - E_q leave no positive threshold: scanned by design, nothing overflowed
    assert st.n_exact_direct == 2 and st.n_fallback == 0
    assert st.search_path & bsr_mod.BSR_PATH_RANGE_SCAN


def test_device_pointers_match_the_host_form(bsr_mod, small):
    import torch
    ix, m, qs, pos = small
    lists = m.lists(qs)
    radius = kth_radius(lists, [3, 40, 1, 17, 25, 8])
    nq, cap = len(qs), 64
    host = ix.range_search(qs, radius, max_results=cap)
    same(host, m.want(qs, radius, cap, lists), "host")
    dq, dr = torch.from_numpy(qs).to("cuda:0"), torch.from_numpy(radius).to("cuda:0")
    oi = torch.full((nq, cap), 5, dtype=torch.int64, device="cuda:0")
    od = torch.full((nq, cap), 5.0, dtype=torch.float32, device="cuda:0")
    oc = torch.full((nq,), 5, dtype=torch.int32, device="cuda:0")
    ix.range_search_device(dq, nq, dr, cap, oi, od, oc)
    torch.cuda.synchronize()
    dev = (oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32))
    same(dev, host, "device")
    # mixed: device queries, host radius and counts, device rows
    hc = np.zeros(nq, np.uint32)
    oi.fill_(5)
    ix.range_search_device(dq, nq, radius, cap, oi, od, hc)
    torch.cuda.synchronize()
    same((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), hc), host, "mixed")


def test_nan_radius_is_invalid_and_writes_nothing(bsr_mod, small):
    import torch
    ix, m, qs, pos = small
    nq, cap = len(qs), 8
    radius = np.full(nq, 0.1, F)
    radius[4] = np.nan
    oi, od, oc = np.full((nq, cap), 9, np.uint64), np.full((nq, cap), 9, F), np.full(nq, 9, np.uint32)
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.range_search_device(qs, nq, radius, cap, oi, od, oc)
    assert e.value.status == E_INVALID
    assert (oi == 9).all() and (od == 9).all() and (oc == 9).all()
    di = torch.full((nq, cap), 9, dtype=torch.int64, device="cuda:0")
    dd = torch.full((nq, cap), 9.0, dtype=torch.float32, device="cuda:0")
    dc = torch.full((nq,), 9, dtype=torch.int32, device="cuda:0")
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.range_search_device(torch.from_numpy(qs).to("cuda:0"), nq, torch.from_numpy(radius).to("cuda:0"), cap,
                               di, dd, dc)
    assert e.value.status == E_INVALID
    torch.cuda.synchronize()
    assert bool((di == 9).all()) and bool((dd == 9).all()) and bool((dc == 9).all())


def test_statuses(bsr_mod, small):
    ix, m, qs, pos = small
    got = ix.range_search(qs[:0], np.zeros(0, F), max_results=4)
    assert got[0].shape == (0, 4) and got[2].shape == (0,)
    bad = qs.copy()
    bad[2, 5] = np.inf
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.range_search(bad, 0.1)
    assert e.value.status == E_NONFINITE
    fresh = bsr_mod.Index(130, max_k=64, device=0)
    with pytest.raises(bsr_mod.BsrError) as e:
        fresh.range_search(qs, 0.1)
    assert e.value.status == E_STATE
    fresh.close()


def test_tombstones_update_compact(bsr_mod, oracle_mod, small):
    """(last of the tests on the shared index: it changes its rows)"""
    ix, m, qs, pos = small
    rng = np.random.default_rng(8)
    cap = 64

    def check(ctx, ms=(30, 40, 12, 5, 33, 20)):
        lists = m.lists(qs)
        radius = kth_radius(lists, ms)
        got = ix.range_search(qs, radius, max_results=cap)
        same(got, m.want(qs, radius, cap, lists), ctx)
        st = ix.last_stats()
        assert st.n_fallback == 0 and st.n_exact_direct == 0, ctx
        return got

    before = check("before any delete")
    gone = np.concatenate([pos[0][::2], rng.choice(np.setdiff1d(np.arange(len(m.rows)), pos.ravel()), 100, False)])
    assert ix.delete(gone + m.offset) == len(gone)
    m.dead[gone] = True
    after = check("half of cluster 0 deleted", ms=(15, 40, 12, 5, 33, 20))
    assert not np.isin(after[0], gone.astype(np.uint64) + np.uint64(m.offset)).any()
    assert np.isin(before[0][0], gone.astype(np.uint64) + np.uint64(m.offset)).any()
    # update: cluster 1 loses ten rows to the background, cluster 2 gains ten from it
    ids = np.concatenate([pos[1][:10], rng.choice(np.setdiff1d(m.live(), pos.ravel()), 10, False)])
    new = np.concatenate([rng.uniform(-1, 1, (10, qs.shape[1])).astype(F), cluster_rows(rng, qs[2], 10)])
    ix.update(ids + m.offset, new)
    m.rows[ids] = new
    check("after an update", ms=(15, 25, 45, 5, 33, 20))
    # compaction: the live rows packed, a new offset
    old = ix.compact(global_offset=50_000)
    assert np.array_equal(old, m.live().astype(np.uint64) + np.uint64(m.offset))
    m2 = Model(oracle_mod, m.rows[m.live()], 50_000)
    m.rows, m.dead, m.offset = m2.rows, m2.dead, m2.offset
    check("after a compaction", ms=(15, 25, 45, 5, 33, 20))
    # every row deleted: every count is 0
    assert ix.delete(np.arange(len(m.rows)) + m.offset) == len(m.rows)
    m.dead[:] = True
    got = ix.range_search(qs, 2.0, max_results=cap)
    assert not got[2].any() and (got[0] == NONE_IDX).all() and np.isposinf(got[1]).all()


# ---- 4. indexes that cannot filter ---------------------------------------------------------------
def test_exact_only_index(bsr_mod, oracle_mod, gpu):
    rows, qs, pos = make_shard(3000, 130, 17, 30, 99)
    m = Model(oracle_mod, rows, 40)
    lists = m.lists(qs)
    radius = kth_radius(lists, [1 + q for q in range(17)])
    want = m.want(qs, radius, 64, lists)
    res = []
    for flags in (0, bsr_mod.BSR_FLAG_EXACT_ONLY):
        ix = bsr_mod.Index(130, max_k=64, device=0, flags=flags).load(rows, global_offset=40)
        got = ix.range_search(qs, radius, max_results=64)
        st = ix.last_stats()
        same(got, want, ("flags", flags))
        assert st.search_path & bsr_mod.BSR_PATH_RANGE
        assert bool(st.search_path & bsr_mod.BSR_PATH_RANGE_SCAN) == bool(flags)
        assert st.n_exact_direct == (17 if flags else 0) and st.n_fallback == 0 and st.n_emitted == (0 if flags else st.n_emitted)
        res.append(got)
        ix.close()
    same(res[1], res[0], "exact-only against the filter path")


def test_small_shard_is_scanned(bsr_mod, oracle_mod, gpu):
    """n <= range_cap(capacity): no filter pass; every radius kind with capacity >= n returns its rows."""
    rng = np.random.default_rng(3)
    n, dim, cap = 300, 100, 512
    rows = rng.uniform(-1, 1, (n, dim)).astype(F)
    qs = rng.uniform(-1, 1, (9, dim)).astype(F)
    rows[200] = qs[1]
    rows[5] = 0.0      # a zero row: distance 1
    rows[6] = -qs[2]   # distance 2
    ix = bsr_mod.Index(dim, max_k=64, device=0).load(rows)
    m = Model(oracle_mod, rows)
    lists = m.lists(qs)
    radius = np.array([-1.0, 0.0, 2.0, np.inf, 1.0, lists[5][1][99], np.nextafter(lists[6][1][99], NEG_INF), 1.9999,
                       1e-30], F)
    want = m.want(qs, radius, cap, lists)
    assert list(want[2][:4]) == [0, 1, n, n] and want[2][5] >= 100 and want[2][6] == 99
    got = ix.range_search(qs, radius, max_results=cap)
    st = ix.last_stats()
    same(got, want, "small shard")
    assert st.search_path & bsr_mod.BSR_PATH_RANGE_SCAN and st.n_exact_direct == 9 and st.n_emitted == 0
    same(ix.range_search(qs, radius, max_results=50), m.want(qs, radius, 50, lists), "small shard, 50 slots")
    ix.delete([5, 200])
    m.dead[[5, 200]] = True
    same(ix.range_search(qs, radius, max_results=cap), m.want(qs, radius, cap), "small shard, tombstones")
