"""Masked top-k search (bsr_local_top_k_masked): the k nearest rows among those an
allow mask names.  The expected result is the reference's compute_local_top_k
(src/mpi_helpers/metrics.rs:16-53) over a store that holds only the allowed rows, each keeping
its global index: oracle.parallel_top_k(host[ids], queries, k) with the indices mapped through
ids (+ offset) -- counts, indices, order and f32 distance bits.  Both paths (the exact scan of
the allowed-row list, the int8 filter with its emitted lists cut by the mask) must give it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THREADS = 16
NONE_IDX = np.uint64(2 ** 64 - 1)


def _same(got, want, ctx):
    gi, gd, gc = got
    wi, wd, wc = want
    assert np.array_equal(gc, wc), (ctx, gc, wc)
    for q in range(len(wc)):
        c = int(wc[q])
        assert np.array_equal(gi[q, :c], wi[q, :c]), (ctx, q, gi[q, :c], wi[q, :c])
        assert np.array_equal(gd[q, :c].view(np.uint32), wd[q, :c].view(np.uint32)), (ctx, q)


def _tail_is_empty(got, ctx):
    gi, gd, gc = got
    for q in range(len(gc)):
        c = int(gc[q])
        assert np.all(gi[q, c:] == NONE_IDX) and np.all(np.isposinf(gd[q, c:])), (ctx, q)


def _want(oracle_mod, host, ids, qs, k, offset=0):
    """The reference's local top-k over the allowed rows (ids ascending), global indices."""
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


def _rand_mask(n, rho, seed):
    return np.random.default_rng(seed).random(n) < rho


# ---- 1. small, odd widths: the list path ---------------------------------------------------
@pytest.fixture(scope="module")
def small(bsr_mod, gpu):
    rng = np.random.default_rng(11)
    n, dim, nq = 3001, 100, 5
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(rows)
    yield ix, rows, qs
    ix.close()


@pytest.mark.parametrize("which", ["rho0.3", "seven", "one", "none", "all"])
def test_small_list_path(bsr_mod, oracle_mod, small, which):
    ix, rows, qs = small
    n, k = len(rows), 10
    mask = np.zeros(n, bool)
    if which == "rho0.3":
        mask = _rand_mask(n, 0.3, 1)
    elif which == "seven":
        mask[[3, 64, 65, 1000, 2047, 2048, 3000]] = True
    elif which == "one":
        mask[1234] = True
    elif which == "all":
        mask[:] = True
    ids = np.flatnonzero(mask)
    want = _want(oracle_mod, rows, ids, qs, k)
    assert np.all(want[2] == min(k, len(ids)))
    for mode in ("auto", "list", "filter"):
        got = ix.local_top_k(qs, k, allow_mask=mask, mask_mode=mode)
        st = ix.last_stats()
        _same(got, want, (which, mode))
        _tail_is_empty(got, (which, mode))
        assert st.graph_replay == 0
        if mode == "list" or which in ("seven", "one", "none"):
            # (a few rows of 3,001 are below the filter's range whatever the mode)
            assert st.search_path & bsr_mod.BSR_PATH_MASK_LIST and not st.search_path & bsr_mod.BSR_PATH_MASK_FILTER
            assert st.n_exact_direct == len(qs)
    # the same mask given as row ids
    got = ix.local_top_k(qs, k, allow_ids=ids[::-1], mask_mode="list")
    _same(got, want, (which, "ids"))


def test_wide_rows_list_path(bsr_mod, oracle_mod, gpu):
    """ld > 1024 (dim 1,100), a partial last tile, k above one wave's list (k = 100)."""
    rng = np.random.default_rng(12)
    n, dim, nq = 700, 1100, 5
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    qs[2] = rows[77]
    ix = bsr_mod.Index(dim, max_k=128, device=0)
    ix.load(rows)
    mask = _rand_mask(n, 0.5, 2)
    mask[77] = True
    ids = np.flatnonzero(mask)
    for k in (10, 100):
        got = ix.local_top_k(qs, k, allow_mask=mask)
        _same(got, _want(oracle_mod, rows, ids, qs, k), ("wide", k))
        assert got[0][2, 0] == 77 and got[1][2, 0] == 0.0
    ix.close()


# ---- 2-5, 8, 9: one shard of 40,037 x 768 uniform rows ------------------------------------
N, D = 40_037, 768


@pytest.fixture(scope="module")
def shard(bsr_mod, gpu):
    rng = np.random.default_rng(21)
    rows = rng.uniform(-1, 1, (N, D)).astype(np.float32)
    qs = rng.uniform(-1, 1, (40, D)).astype(np.float32)
    ix = bsr_mod.Index(D, max_k=256, device=0)
    ix.load(rows)
    yield ix, rows, qs
    ix.close()


@pytest.fixture(scope="module")
def wants(oracle_mod, shard):
    """Expected lists, computed once per (rho, k, nq) and shared."""
    _, rows, qs = shard
    cache = {}

    def get(rho, k, nq):
        key = (rho, k, nq)
        if key not in cache:
            mask = _rand_mask(N, rho, int(1 / rho))
            cache[key] = (mask, _want(oracle_mod, rows, np.flatnonzero(mask), qs[:nq], k))
        return cache[key]
    return get


@pytest.mark.parametrize("rho,k,nq", [(1 / 2, 10, 40), (1 / 8, 10, 40), (1 / 2, 10, 3), (1 / 8, 10, 3),
                                      (1 / 2, 50, 40), (1 / 2, 50, 3)])
def test_filter_path(bsr_mod, shard, wants, rho, k, nq):
    ix, rows, qs = shard
    mask, want = wants(rho, k, nq)
    got = ix.local_top_k(qs[:nq], k, allow_mask=mask, mask_mode=bsr_mod.BSR_MASK_FILTER)
    st = ix.last_stats()
    print(f"filter rho={rho:.3f} k={k} nq={nq}: fallback={st.n_fallback} exact_direct={st.n_exact_direct} "
          f"emitted={st.n_emitted} path={st.search_path}")
    assert st.search_path & bsr_mod.BSR_PATH_MASK_FILTER, st.search_path
    _same(got, want, ("filter", rho, k, nq))
    _tail_is_empty(got, ("filter", rho, k, nq))
    # (a filter path that never certifies must not pass on its fallback alone)
    assert st.n_fallback + st.n_exact_direct < nq, (st.n_fallback, st.n_exact_direct)
    assert st.n_queries == nq and st.graph_replay == 0
    got_l = ix.local_top_k(qs[:nq], k, allow_mask=mask, mask_mode=bsr_mod.BSR_MASK_LIST)
    st = ix.last_stats()
    assert st.search_path & bsr_mod.BSR_PATH_MASK_LIST and not st.search_path & bsr_mod.BSR_PATH_MASK_FILTER
    for a, b in zip(got, got_l):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                              b.view(np.uint32) if b.dtype == np.float32 else b)


def test_below_the_filters_range(bsr_mod, oracle_mod, shard, wants):
    ix, rows, qs = shard
    mask, want = wants(1 / 100, 10, 40)
    got = ix.local_top_k(qs, 10, allow_mask=mask, mask_mode=bsr_mod.BSR_MASK_FILTER)
    st = ix.last_stats()
    assert st.search_path & bsr_mod.BSR_PATH_MASK_LIST and not st.search_path & bsr_mod.BSR_PATH_MASK_FILTER
    _same(got, want, "rho 1/100")
    # k above the filter's largest k: the list path
    mask, want = wants(1 / 2, 256, 3)
    got = ix.local_top_k(qs[:3], 256, allow_mask=mask, mask_mode=bsr_mod.BSR_MASK_FILTER)
    st = ix.last_stats()
    assert st.search_path & bsr_mod.BSR_PATH_MASK_LIST and not st.search_path & bsr_mod.BSR_PATH_MASK_FILTER
    _same(got, want, "k 256")


@pytest.mark.parametrize("nq", [40, 3])
def test_all_ones_mask_is_the_unmasked_search(bsr_mod, shard, nq):
    ix, rows, qs = shard
    words = np.full((N + 63) // 64, 2 ** 64 - 1, np.uint64)  # (the tail bits past n set too)
    base = ix.local_top_k(qs[:nq], 10)
    for mode in (bsr_mod.BSR_MASK_LIST, bsr_mod.BSR_MASK_FILTER, bsr_mod.BSR_MASK_AUTO):
        got = ix.local_top_k(qs[:nq], 10, allow_mask=words, mask_mode=mode)
        assert np.array_equal(got[2], base[2]) and np.array_equal(got[0], base[0]), mode
        assert np.array_equal(got[1].view(np.uint32), base[1].view(np.uint32)), mode


def test_state_isolation(bsr_mod, shard, wants):
    """A masked search between unmasked ones: their results and their graph replay are untouched."""
    ix, rows, qs = shard
    mask, want = wants(1 / 2, 10, 40)
    first = None
    for rep in range(3):
        got = ix.local_top_k(qs, 10)
        first = first or got
    assert ix.last_stats().graph_replay == 1
    for mode in ("filter", "list"):
        m = ix.local_top_k(qs, 10, allow_mask=mask, mask_mode=mode)
        assert ix.last_stats().graph_replay == 0
        _same(m, want, ("between", mode))
    for rep in range(3):
        got = ix.local_top_k(qs, 10)
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[2], first[2]), rep
        assert np.array_equal(got[1].view(np.uint32), first[1].view(np.uint32)), rep
    assert ix.last_stats().graph_replay == 1


def test_device_mask_and_queries(bsr_mod, shard, wants):
    import torch
    ix, rows, qs = shard
    mask, want = wants(1 / 2, 10, 40)
    words = bsr_mod.pack_allow_mask(N, mask=mask)
    dw = torch.from_numpy(words.view(np.int64)).to("cuda:0")
    dq = torch.from_numpy(qs).to("cuda:0")
    for mode in ("filter", "list", "auto"):
        oi = torch.zeros((40, 10), dtype=torch.int64, device="cuda:0")
        od = torch.zeros((40, 10), dtype=torch.float32, device="cuda:0")
        oc = torch.zeros(40, dtype=torch.int32, device="cuda:0")
        ix.local_top_k_device(dq, 40, 10, oi, od, oc, allow_words=dw, mask_mode=mode)
        got = (oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32))
        _same(got, want, ("device", mode))
    # the packed device words through local_top_k as well
    _same(ix.local_top_k(qs, 10, allow_mask=dw), want, "device words")


def test_errors(bsr_mod, shard):
    ix, rows, qs = shard
    words = bsr_mod.pack_allow_mask(N, mask=np.ones(N, bool))
    oi, od, oc = np.zeros((2, 10), np.uint64), np.zeros((2, 10), np.float32), np.zeros(2, np.uint32)
    q = np.ascontiguousarray(qs[:2])

    def status(**kw):
        a = dict(queries=q, nq=2, k=10, allow_words=words, mask_mode="auto")
        a.update(kw)
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.local_top_k_device(a["queries"], a["nq"], a["k"], oi, od, oc, allow_words=a["allow_words"],
                                  mask_mode=a["mask_mode"])
        return e.value.status

    assert status(allow_words=words[:-1]) == -1
    assert status(allow_words=np.concatenate([words, words[:1]])) == -1
    assert status(mask_mode=3) == -1
    assert status(k=0) == -1
    assert status(k=257) == -1
    bad = q.copy()
    bad[1, 5] = np.nan
    assert status(queries=bad) == -2
    assert status(queries=bad, mask_mode="list") == -2
    with pytest.raises(bsr_mod.BsrError):
        ix.local_top_k(q, 10, allow_mask=np.ones(N, bool), allow_ids=[1])
    # a null mask through the C ABI
    st = bsr_mod.lib().bsr_local_top_k_masked(ix._h, q.ctypes.data, 2, 10, None, len(words), 0, oi.ctypes.data,
                                              od.ctypes.data, oc.ctypes.data)
    assert st == -1
    # the index still searches
    got = ix.local_top_k(q, 10, allow_mask=np.ones(N, bool))
    assert np.all(got[2] == 10)
    empty = bsr_mod.Index(D, max_k=16, device=0)
    with pytest.raises(bsr_mod.BsrError) as e:
        empty.local_top_k_device(q, 2, 10, oi, od, oc, allow_words=words)
    assert e.value.status == -7
    empty.close()


# ---- 6. ties and shortcuts -------------------------------------------------------------------
def test_ties_and_shortcuts(bsr_mod, oracle_mod, gpu):
    rng = np.random.default_rng(31)
    n, dim, off = 12_011, 128, 1_000_000
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    r = 777
    rows[r + 5000] = rows[r]              # identical rows, the first disallowed
    rows[[40, 41, 9000]] = 0.0            # all-zero rows: distance 1.0
    qs = rng.uniform(-1, 1, (4, dim)).astype(np.float32)
    qs[0] = rows[2500]                    # equal to an allowed row
    qs[1] = rows[r]                       # equal to a disallowed row whose duplicate is allowed
    qs[2] = rows[r] * np.float32(0.5) + np.float32(0.01)
    mask = _rand_mask(n, 0.5, 3)
    mask[[2500, r + 5000, 40, 41, 9000]] = True
    mask[r] = False
    ids = np.flatnonzero(mask)
    ix = bsr_mod.Index(dim, max_k=256, device=0)
    ix.load(rows, off)
    for mode in ("list", "filter"):
        for k in (10, 200):
            want = _want(oracle_mod, rows, ids, qs, k, off)
            got = ix.local_top_k(qs, k, allow_mask=mask, mask_mode=mode)
            _same(got, want, ("ties", mode, k))
            assert not np.any(got[0] == off + r), (mode, k)
        assert got[0][0, 0] == off + 2500 and got[1][0, 0] == 0.0
        assert got[0][1, 0] == off + r + 5000 and got[1][1, 0] == 0.0
        assert np.any(got[0][2] == off + r + 5000)
    # only the zero rows and a few others allowed: 1.0 for the zero rows, in index order
    few = np.zeros(n, bool)
    few[[40, 41, 9000]] = True
    got = ix.local_top_k(qs, 5, allow_mask=few, mask_mode="list")
    assert np.all(got[2] == 3)
    assert np.array_equal(got[0][:, :3], np.tile(np.uint64(off) + np.array([40, 41, 9000], np.uint64), (4, 1)))
    assert np.all(got[1][:, :3] == 1.0)
    ix.close()


# ---- 7. clusters (the filter path) -----------------------------------------------------------
def test_clusters(bsr_mod, oracle_mod, gpu):
    """300 allowed near-duplicates of query 0: all emitted, the list certifies.  5,000 disallowed
    near-duplicates of query 1: its emitted list overflows the cap, the cut leaves it overflowed,
    and the query takes the list scan.  The clusters sit on rows the sample pass never reads."""
    rng = np.random.default_rng(41)
    n, dim, k = 40_037, 768, 10
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (6, dim)).astype(np.float32)
    free = np.array([i for i in range(n) if i % 32 != 0])
    pick = rng.permutation(free)
    near, far = pick[:300], pick[300:5300]
    rows[near] = qs[0] + 1e-3 * rng.standard_normal((300, dim)).astype(np.float32)
    rows[far] = qs[1] + 1e-3 * rng.standard_normal((5000, dim)).astype(np.float32)
    mask = _rand_mask(n, 0.5, 4)
    mask[near] = True
    mask[far] = False
    ids = np.flatnonzero(mask)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(rows)
    # the allowed cluster alone
    sel = [0, 2, 3]
    got = ix.local_top_k(qs[sel], k, allow_mask=mask, mask_mode="filter")
    st = ix.last_stats()
    _same(got, _want(oracle_mod, rows, ids, qs[sel], k), "allowed cluster")
    assert st.search_path & bsr_mod.BSR_PATH_MASK_FILTER
    assert set(got[0][0].tolist()) <= set(near.tolist())
    # the disallowed cluster: an overflowed list
    got = ix.local_top_k(qs, k, allow_mask=mask, mask_mode="filter")
    st = ix.last_stats()
    _same(got, _want(oracle_mod, rows, ids, qs, k), "disallowed cluster")
    assert st.search_path & bsr_mod.BSR_PATH_MASK_FILTER and st.search_path & bsr_mod.BSR_PATH_MASK_LIST
    assert 1 <= st.n_fallback < len(qs), st.n_fallback
    assert not set(got[0][1].tolist()) & set(far.tolist())
    assert st.n_emitted >= 5000
    ix.close()


# ---- 10. seeded sweep ------------------------------------------------------------------------
SWEEP_DIMS = [64, 100, 768, 1024]
SWEEP_KS = [1, 10, 50, 200, 256]
SWEEP_KINDS = ["uniform", "clusters", "integers"]
SWEEP_OPS_CAP = 1.5e9  # allowed rows x queries x dim per case (the oracle's work)


def _sweep_case(i):
    rng = np.random.default_rng(20261019 + i)
    dim = int(rng.choice(SWEEP_DIMS))
    nq = int(rng.integers(1, 301))
    k = int(rng.choice(SWEEP_KS))
    n = int(rng.integers(1, 50_001))
    n = max(1, min(n, int(SWEEP_OPS_CAP / (nq * dim))))
    rho = [0.0, 1.0 / n, 1 / 1000, 1 / 16, 1 / 2, 1.0][int(rng.integers(0, 6))]
    mode = int(rng.integers(0, 3))
    kind = SWEEP_KINDS[i % len(SWEEP_KINDS)]
    return rng, dim, nq, k, n, rho, mode, kind


def _sweep_data(rng, kind, n, dim, nq):
    if kind == "uniform":
        rows = rng.uniform(-1, 1, (n, dim))
    elif kind == "clusters":
        c = rng.uniform(-1, 1, (int(rng.integers(4, 33)), dim))
        rows = c[rng.integers(0, len(c), n)] + 0.05 * rng.standard_normal((n, dim))
    else:
        rows = rng.integers(-2, 3, (n, dim)).astype(np.float64)
    rows = rows.astype(np.float32)
    if n > 8:
        rows[n - 1] = rows[1]
        rows[4] = 0
    qs = (rng.integers(-2, 3, (nq, dim)) if kind == "integers" else rng.uniform(-1, 1, (nq, dim))).astype(np.float32)
    for j in range(nq):
        if j % 5 == 1:
            qs[j] = rows[int(rng.integers(0, n))]
        elif j % 15 == 3 and j > 0:
            qs[j] = 0
    return rows, qs


SWEEP = list(range(12))


def test_sweep_case_list():
    """The sweep's cases, printed so that a failure names its seed and shape."""
    for i in SWEEP:
        _, dim, nq, k, n, rho, mode, kind = _sweep_case(i)
        print(f"sweep case {i}: seed={20261019 + i} n={n} dim={dim} nq={nq} k={k} rho={rho:.5f} mode={mode} {kind}")


@pytest.mark.parametrize("i", SWEEP)
def test_sweep_vs_oracle(bsr_mod, oracle_mod, gpu, i):
    rng, dim, nq, k, n, rho, mode, kind = _sweep_case(i)
    ctx = f"sweep case {i}: seed={20261019 + i} n={n} dim={dim} nq={nq} k={k} rho={rho:.5f} mode={mode} {kind}"
    print(ctx)
    rows, qs = _sweep_data(rng, kind, n, dim, nq)
    if rho == 0.0:
        mask = np.zeros(n, bool)
    elif rho == 1.0:
        mask = np.ones(n, bool)
    elif rho == 1.0 / n:
        mask = np.zeros(n, bool)
        mask[int(rng.integers(0, n))] = True
    else:
        mask = rng.random(n) < rho
    ids = np.flatnonzero(mask)
    off = int(rng.integers(0, 1 << 33))
    ix = bsr_mod.Index(dim, max_k=256, device=0)
    ix.load(rows, off)
    got = ix.local_top_k(qs, k, allow_mask=mask, mask_mode=mode)
    st = ix.last_stats()
    ix.close()
    want = _want(oracle_mod, rows, ids, qs, k, off)
    assert np.all(want[2] == min(k, len(ids))), ctx
    _same(got, want, ctx)
    _tail_is_empty(got, ctx)
    assert st.search_path & (bsr_mod.BSR_PATH_MASK_LIST | bsr_mod.BSR_PATH_MASK_FILTER), ctx
