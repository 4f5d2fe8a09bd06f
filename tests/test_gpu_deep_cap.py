"""Deep capped search (bsr_local_top_k_deep_capped) through the C ABI.  Every expected
row is kcheck_cap's pure-numpy model of the capped contract over the oracle's distances of every
stored row to every query (computed once per shard); indices, order, distance bits, groups, counts
and padding must be equal -- no tolerance anywhere."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import kcheck_cap as kp
from test_gpu_deep import plant_ladder

pytestmark = pytest.mark.gpu

F = np.float32
OFFSET = 7000
E_INVALID, E_NONFINITE = -1, -2
SHAPES = [(64, 40_000), (768, 40_000), (130, 50_001)]
# the seed of row_group per (dim, n // G): one at which, by the model, the cap drops a row of the first
# three queries' top 257 at three rows a group (1000 groups: one seed in two or three does)
SEEDS = {(64, 40): 6, (768, 40): 1, (130, 40): 8}
_made = {}


def shard(bsr_mod, oracle_mod, dim, n, flags=0, nq=40, plant=None, dtype=None, tag=None):
    """(index, stored rows, queries, distances [nq][n]) of a U(-1, 1) shard, made once per key (tag: an
    index of the test's own, which it may modify)."""
    key = (dim, n, flags, nq, plant is not None, dtype, tag)
    if key not in _made:
        rng = np.random.default_rng(dim * 1000 + n)
        rows = rng.uniform(-1, 1, (n, dim)).astype(F)
        qs = rng.uniform(-1, 1, (nq, dim)).astype(F)
        if plant:
            plant(rng, rows, qs)
        ix = bsr_mod.Index(dim, max_k=256, device=0, flags=flags, dtype=bsr_mod.BSR_F32 if dtype is None else dtype)
        if dtype == bsr_mod.BSR_BF16:
            bits = (rows.view(np.uint32) >> 16).astype(np.uint16)
            rows = (bits.astype(np.uint32) << 16).view(F)  # (the widened values the index keeps)
            ix.load(bits, global_offset=OFFSET)
        else:
            ix.load(rows, global_offset=OFFSET)
        with ThreadPoolExecutor(8) as ex:
            dists = np.stack(list(ex.map(lambda q: oracle_mod.np_cosine_distances(rows, q), qs)))
        _made[key] = (ix, rows, qs, dists)
    return _made[key]


def groups(n, G, seed=0):
    return np.random.default_rng(seed).integers(0, G, n).astype(np.uint32)


def same(got, want, ctx=""):
    """got / want: (idx, dist, count, group)."""
    assert np.array_equal(got[2], want[2]), (ctx, "counts", got[2], want[2])
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1))
    assert bad.size == 0, (ctx, "indices", bad[:8])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (ctx, "distance bits")
    assert np.array_equal(got[3], want[3]), (ctx, "groups")


@pytest.mark.parametrize("k", [1, 257, 1000, 1024])
@pytest.mark.parametrize("nq", [3, 40])
@pytest.mark.parametrize("gdiv,m", [(10, 1), (40, 3)])
@pytest.mark.parametrize("dim,n", SHAPES)
def test_filter_rung(bsr_mod, oracle_mod, gpu, dim, n, gdiv, m, nq, k):
    ix, rows, qs, dists = shard(bsr_mod, oracle_mod, dim, n)
    G = n // gdiv
    rg = groups(n, G, SEEDS.get((dim, gdiv), 0))
    want = kp.cap_batch(dists[:nq], rg, k, m, offset=OFFSET)
    # the inputs do what the case is about, by the model alone: the cap drops a row, and the k-th
    # kept row lies within the first 1.5 k rows of the plain order
    plain = kp.cap_batch(dists[:nq], np.arange(n), k, 1, offset=OFFSET)
    if k >= 257:
        assert not np.array_equal(want[0], plain[0])
    for q in range(nq):
        d, i = want[1][q, k - 1], int(want[0][q, k - 1]) - OFFSET
        assert np.count_nonzero((dists[q] < d) | ((dists[q] == d) & (np.arange(n) <= i))) <= 1.5 * k
    same(ix.deep_capped_search(qs[:nq], k, rg, m, n_groups=G, return_groups=True), want)
    st = ix.last_stats()
    print(f"emitted/query={st.n_emitted / nq:.0f} fallback={st.n_fallback} direct={st.n_exact_direct}")
    assert st.search_path == bsr_mod.BSR_PATH_DEEP | bsr_mod.BSR_PATH_CAP and st.n_queries == nq
    assert st.n_fallback + st.n_exact_direct <= nq / 10  # (the scan must not hide a rung that never certifies)


@pytest.mark.parametrize("case", ["few_groups_m1", "few_groups_m3", "budget", "long_document", "exact_only",
                                  "small_shard"])
def test_scan_rung(bsr_mod, oracle_mod, gpu, monkeypatch, case):
    n, k, m, G, nq, flags, plant = 40_000, 1000, 3, 300, 5, 0, None
    if case == "few_groups_m1":
        m = 1
    elif case == "budget":
        monkeypatch.setenv("BSR_COLLAPSE_TABLE_BUDGET", "1")  # (rounds of one query)
    elif case == "long_document":
        n, k, G, nq, plant = 45_000, 257, 45_000 // 40, 8, plant_ladder
    elif case == "exact_only":
        flags = bsr_mod.BSR_FLAG_EXACT_ONLY
    elif case == "small_shard":
        n, G = 3000, 3000 // 10  # (live <= cap: no filter rung)
    ix, rows, qs, dists = shard(bsr_mod, oracle_mod, 64, n, flags=flags, nq=nq, plant=plant)
    rg = groups(n, G)
    if plant:
        rg[1000:4000] = 0  # the 3000 near-duplicates of query 0: one long document
    want = kp.cap_batch(dists, rg, k, m, offset=OFFSET)
    same(ix.deep_capped_search(qs, k, rg, m, n_groups=G, return_groups=True), want, case)
    st = ix.last_stats()
    assert st.search_path == bsr_mod.BSR_PATH_DEEP | bsr_mod.BSR_PATH_CAP | bsr_mod.BSR_PATH_CAP_SCAN
    if case in ("exact_only", "small_shard"):
        assert st.n_exact_direct == nq and st.n_fallback == 0 and st.n_emitted == 0
    elif case == "long_document":
        assert st.n_fallback >= 1 and st.n_exact_direct >= 1  # (query 0; the zero query 2)
    else:
        assert np.all(want[2] == m * G) and st.n_fallback == nq and st.n_exact_direct == 0


def test_identities(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, dists = shard(bsr_mod, oracle_mod, 768, 40_000)
    n = len(rows)
    got = ix.deep_capped_search(qs, 1000, np.arange(n), 7, n_groups=n)
    for a, b in zip(got, ix.deep_search(qs, 1000)):
        assert a.tobytes() == b.tobytes()
    rg = groups(n, n // 40)
    for m, other in ((3, lambda: ix.capped_search(qs, 200, rg, 3, n_groups=n // 40, fetch_k=256, return_groups=True)),
                     (1, lambda: ix.collapsed_search(qs, 200, rg, n_groups=n // 40, fetch_k=256, return_groups=True))):
        for a, b in zip(ix.deep_capped_search(qs, 200, rg, m, n_groups=n // 40, return_groups=True), other()):
            assert a.tobytes() == b.tobytes()
    deep = ix.deep_capped_search(qs, 1000, rg, 3, n_groups=n // 40, return_groups=True)
    shallow = ix.deep_capped_search(qs, 257, rg, 3, n_groups=n // 40, return_groups=True)
    assert all(np.array_equal(deep[j][:, :257], shallow[j]) for j in (0, 1, 3))


@pytest.mark.parametrize("on_dev", [False, True])
@pytest.mark.parametrize("dtype", ["BSR_F32", "BSR_BF16"])
def test_deleted_rows(bsr_mod, oracle_mod, gpu, dtype, on_dev):
    import torch
    n, nq, k, m, G = 40_000, 6, 1000, 3, 1000
    ix, rows, qs, dists = shard(bsr_mod, oracle_mod, 64, n, nq=nq, dtype=getattr(bsr_mod, dtype), tag="deleted")
    rg = groups(n, G)
    rng = np.random.default_rng(5)
    heads = kp.cap_batch(dists[:1], rg, 40, 1)[0][0].astype(np.int64)  # the head rows of query 0's 40 best groups
    gone = np.union1d(heads[::2], np.flatnonzero(rng.random(n) < 0.05))
    ix.delete(gone + OFFSET)  # (the second run of the pair deletes nothing new)
    live = np.ones(n, bool)
    live[gone] = False
    want = kp.cap_batch(dists, rg, k, m, live=live, offset=OFFSET)
    if not on_dev:
        return same(ix.deep_capped_search(qs, k, rg, m, n_groups=G, return_groups=True), want)
    dev = torch.device("cuda:0")
    oi, od, og = (torch.zeros((nq, k), dtype=t, device=dev) for t in (torch.int64, torch.float32, torch.int32))
    oc = torch.zeros(nq, dtype=torch.int32, device=dev)
    ix.deep_capped_search_device(torch.from_numpy(qs).to(dev), nq, k, m, torch.from_numpy(rg.view(np.int32)).to(dev), G,
                                 oi, od, oc, out_group=og)
    same((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32),
          og.cpu().numpy().view(np.uint32)), want)


def test_two_ranks_compose(bsr_mod, oracle_mod, gpu):
    import torch
    ix, rows, qs, dists = shard(bsr_mod, oracle_mod, 64, 40_000)
    n, nq, k, m, G, half = len(rows), 8, 1000, 3, 1000, 20_000
    rg = groups(n, G)
    dev = torch.device("cuda:0")
    li, ld, lg = (torch.zeros((2, nq, k), dtype=t, device=dev) for t in (torch.int64, torch.float32, torch.int32))
    lc = torch.zeros((2, nq), dtype=torch.int32, device=dev)
    q = torch.from_numpy(qs[:nq]).to(dev)
    for r, (lo, hi) in enumerate(((0, half), (half, n))):
        part = bsr_mod.Index(64, max_k=256, device=0)
        part.load(rows[lo:hi], global_offset=OFFSET + lo)
        part.deep_capped_search_device(q, nq, k, m, np.ascontiguousarray(rg[lo:hi]), G, li[r], ld[r], lc[r],
                                       out_group=lg[r])
    oi, od, og = (torch.zeros((nq, k), dtype=t, device=dev) for t in (torch.int64, torch.float32, torch.int32))
    oc = torch.zeros(nq, dtype=torch.int32, device=dev)
    bsr_mod.merge_top_k_lists_capped_device(li, ld, lg, lc, k, m, oi, od, og, oc)
    torch.cuda.synchronize()
    one = ix.deep_capped_search(qs[:nq], k, rg, m, n_groups=G, return_groups=True)
    same((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32),
          og.cpu().numpy().view(np.uint32)), one)


@pytest.mark.parametrize("case", ["bad_group", "nan_query", "short_row_group", "null_row_group", "no_queries"])
def test_errors_leave_outputs_untouched(bsr_mod, oracle_mod, gpu, case):
    import torch
    ix, rows, qs, dists = shard(bsr_mod, oracle_mod, 64, 40_000)
    n, nq, k, G = len(rows), 4, 300, 1000
    rg, q, want = groups(n, G), qs[:nq].copy(), E_INVALID
    if case == "bad_group":
        rg[n - 1] = G
    elif case == "nan_query":
        q[2, 7], want = np.nan, E_NONFINITE
    elif case == "short_row_group":
        rg = rg[:-1].copy()
    for dev in (None, torch.device("cuda:0")):
        outs = [torch.full((nq, k), 7, dtype=t, device=dev) for t in (torch.int64, torch.float32, torch.int32)]
        outs.insert(2, torch.full((nq,), 7, dtype=torch.int32, device=dev))
        args = (q, 0 if case == "no_queries" else nq, k, 3, None if case == "null_row_group" else rg, G)
        if case == "null_row_group":  # (the wrapper reads the length off the array: the C call itself)
            rc = bsr_mod.lib().bsr_local_top_k_deep_capped(ix._h, q.ctypes.data, nq, k, 3, None, n, G,
                                                           *(o.data_ptr() for o in (outs[0], outs[1], outs[3], outs[2])))
            assert rc == E_INVALID
        elif case == "no_queries":
            ix.deep_capped_search_device(*args, outs[0], outs[1], outs[2], out_group=outs[3])  # (BSR_OK)
        else:
            with pytest.raises(bsr_mod.BsrError) as e:
                ix.deep_capped_search_device(*args, outs[0], outs[1], outs[2], out_group=outs[3])
            assert e.value.status == want
        torch.cuda.synchronize()
        assert all(bool((o == 7).all()) for o in outs)
