"""Masked deep search (bsr_local_top_k_deep_masked) through the Python entry point.
The model: the oracle's order of ALL rows of a shard per query (oracle.parallel_top_k with k = n, one
rank: (distance asc, index asc)), computed once per shard; a query's expected row is that order cut
to the rows its mask allows and that are not deleted, the first k.  Indices, order and distance bits
must be equal -- no tolerance anywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
PAD = np.uint64(2 ** 64 - 1)
OFFSET, NQ = 7000, 7
E_INVALID = -1
TIES = slice(100, 160)  # a block of identical rows
_made = {}


def shard(bsr_mod, oracle_mod, dim, n):
    """(index, queries, the oracle's order of every row and its distances, live[n]) of a U(-1, 1) shard
    with the tie block and 5% tombstones, made once per key."""
    if (dim, n) not in _made:
        rng = np.random.default_rng(dim * 1000 + n)
        rows = rng.uniform(-1, 1, (n, dim)).astype(F)
        rows[TIES] = rows[TIES.start]
        qs = rng.uniform(-1, 1, (NQ, dim)).astype(F)
        qs[0] = rows[TIES.start] + rng.uniform(-0.01, 0.01, dim).astype(F)  # the tie block leads its answer
        ix = bsr_mod.Index(dim, max_k=64, device=0)
        ix.load(rows, global_offset=OFFSET)
        gone = np.setdiff1d(np.flatnonzero(rng.random(n) < 0.05), np.arange(TIES.start, TIES.stop))
        assert ix.delete(gone.astype(np.uint64) + np.uint64(OFFSET)) == len(gone)
        live = np.ones(n, bool)
        live[gone] = False
        wi, wd, _ = oracle_mod.parallel_top_k(rows, qs, n, size=1, threads=8)
        _made[(dim, n)] = (ix, qs, wi.astype(np.int64), wd, live)
    return _made[(dim, n)]


def mask_of(rng, live, a):
    """A mask that allows a live rows -- the tie block first -- and every deleted row."""
    n = len(live)
    ids = np.flatnonzero(live)
    first = ids[(ids >= TIES.start) & (ids < TIES.stop)][:a]
    rest = rng.permutation(np.setdiff1d(ids, first))[:a - len(first)]
    m = ~live
    m[first] = m[rest] = True
    return m if a < n else np.ones(n, bool)


def check(got, order, dist, ok, k, q, gq=None):
    gi, gd, gc = got
    gq = q if gq is None else gq
    keep = ok[order[q]]
    wi, wd = order[q][keep][:k], dist[q][keep][:k]
    c = len(wi)
    assert gc[gq] == c == min(k, int(ok.sum())), (q, int(gc[gq]), c)
    assert np.array_equal(gi[gq, :c], wi.astype(np.uint64) + np.uint64(OFFSET)), f"query {q}: indices / order"
    assert np.array_equal(gd[gq, :c].view(np.uint32), wd.view(np.uint32)), f"query {q}: distance bits"
    assert np.all(gi[gq, c:] == PAD) and np.all(np.isposinf(gd[gq, c:]))


def path_ok(bsr_mod, st, groups):
    p = st.search_path
    assert p & bsr_mod.BSR_PATH_DEEP and not p & bsr_mod.BSR_PATH_DEEP_SCAN
    assert bool(p & bsr_mod.BSR_PATH_MASK_GROUPS) == groups
    return p


@pytest.mark.parametrize("k", [1, 257, 1024])
@pytest.mark.parametrize("dim", [64, 100, 768])
def test_one_mask_list(bsr_mod, oracle_mod, gpu, dim, k):
    n = 3000
    ix, qs, order, dist, live = shard(bsr_mod, oracle_mod, dim, n)
    rng = np.random.default_rng(k)
    for a in sorted({0, 1, k - 1, k, k + 1, n} | ({2400} if k == 1024 else set())):  # (2400 > kDeepScanBuf)
        m = mask_of(rng, live, a)
        got = ix.deep_search(qs[:5], k, allow_mask=m, mask_mode="list")  # (5 queries: a group of 4 and a padded one)
        for q in range(5):
            check(got, order, dist, m & live, k, q)
        st = ix.last_stats()
        assert path_ok(bsr_mod, st, False) & bsr_mod.BSR_PATH_MASK_LIST and st.n_exact_direct == 5 and st.n_fallback == 0


@pytest.mark.parametrize("budget", [None, 4 * 900])
def test_three_masks_and_chunks(bsr_mod, oracle_mod, gpu, monkeypatch, budget):
    """Masks of 2500, 40 and 700 rows, the second named by no query; with the budget, the first list
    is split over three chunks and the third shares a chunk with its tail: the carry."""
    if budget:
        monkeypatch.setenv("BSR_MASK_LIST_BUDGET", str(budget))
    ix, qs, order, dist, live = shard(bsr_mod, oracle_mod, 64, 3000)
    rng = np.random.default_rng(3)
    masks = np.stack([mask_of(rng, live, a) for a in (2500, 40, 700)])
    qmask = np.array([0, 2, 0, 0, 2, 0, 0], np.uint32)
    got = ix.deep_search(qs, 1024, allow_masks=masks, query_mask=qmask, mask_mode="list")
    for q in range(NQ):
        check(got, order, dist, masks[qmask[q]] & live, 1024, q)
    assert path_ok(bsr_mod, ix.last_stats(), True) & bsr_mod.BSR_PATH_MASK_LIST


def test_modes_agree_where_the_filter_runs(bsr_mod, oracle_mod, gpu):
    """n = 20 000, k = 257, rho = 1/2: ks_m = ceil(33 * 19 000 / 10 000) = 63 <= 128, lists of 8064 keys."""
    ix, qs, order, dist, live = shard(bsr_mod, oracle_mod, 64, 20_000)
    m = mask_of(np.random.default_rng(4), live, 10_000)
    by_list = ix.deep_search(qs, 257, allow_mask=m, mask_mode="list")
    by_filter = ix.deep_search(qs, 257, allow_mask=m, mask_mode="filter")
    st = ix.last_stats()
    print(f"emitted/query={st.n_emitted / NQ:.0f} fallback={st.n_fallback} direct={st.n_exact_direct} cap={st.n_candidates}")
    assert path_ok(bsr_mod, st, False) & bsr_mod.BSR_PATH_MASK_FILTER and st.n_emitted > 0
    assert st.n_fallback + st.n_exact_direct < NQ  # (the list scan must not hide a rung that never certifies)
    for a, b in zip(by_list, by_filter):
        assert a.tobytes() == b.tobytes()
    for q in range(NQ):
        check(by_filter, order, dist, m & live, 257, q)


def test_device_pointers(bsr_mod, oracle_mod, gpu):
    import torch
    ix, qs, order, dist, live = shard(bsr_mod, oracle_mod, 64, 3000)
    rng = np.random.default_rng(5)
    masks = np.stack([mask_of(rng, live, a) for a in (1500, 300)])
    qmask = np.array([1, 0, 0, 1, 0, 0, 0], np.int32)
    dev = torch.device("cuda:0")
    words = torch.from_numpy(bsr_mod.pack_allow_masks(3000, masks=masks).view(np.int64)).to(dev)
    oi = torch.zeros((NQ, 1000), dtype=torch.int64, device=dev)
    od = torch.zeros((NQ, 1000), dtype=torch.float32, device=dev)
    oc = torch.zeros(NQ, dtype=torch.int32, device=dev)
    ix.deep_search_device(torch.from_numpy(qs).to(dev), NQ, 1000, oi, od, oc, allow_words=words,
                          query_mask=torch.from_numpy(qmask).to(dev))
    torch.cuda.synchronize()
    got = (oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32))
    for q in range(NQ):
        check(got, order, dist, masks[qmask[q]] & live, 1000, q)


@pytest.mark.parametrize("case", ["k0", "k1025", "allow_words", "query_mask"])
def test_errors_leave_the_outputs_untouched(bsr_mod, oracle_mod, gpu, case):
    ix, qs, _, _, live = shard(bsr_mod, oracle_mod, 64, 3000)
    words = bsr_mod.pack_allow_masks(3000, masks=np.stack([live, ~live]))
    if case == "allow_words":
        words = np.ascontiguousarray(words[:, :-1])
    qmask = np.array([0, 1, 2 if case == "query_mask" else 1, 0], np.uint32)
    k = {"k0": 0, "k1025": 1025}.get(case, 300)
    oi, od, oc = np.full((4, 1025), 0x1234, np.uint64), np.full((4, 1025), -3.0, F), np.full(4, 0x5A5A, np.uint32)
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.deep_search_device(qs[:4].copy(), 4, k, oi, od, oc, allow_words=words, query_mask=qmask)
    assert e.value.status == E_INVALID
    assert np.all(oi == 0x1234) and np.all(od == -3.0) and np.all(oc == 0x5A5A)
