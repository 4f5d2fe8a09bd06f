"""Grouped masked search (bsr_local_top_k_masked_groups): one allow mask per group
of queries in one batch.  The expected result of every query is the reference's
compute_local_top_k over a store that holds only the live rows its own mask names, each keeping
its global index: per mask, oracle.parallel_top_k(host[ids_g], queries_of_g, k) with the indices
mapped through ids_g -- counts, indices, order and f32 distance bits, on every path."""
import ctypes

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


def _bitwise(a, b, ctx):
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                              y.view(np.uint32) if y.dtype == np.float32 else y), ctx


def _want(oracle_mod, host, masks, qmask, qs, k, offset=0, live=None):
    """The oracle per mask: every query over the (live) rows of its own mask, global indices."""
    nq = len(qs)
    qmask = np.asarray(qmask)
    gi = np.full((nq, k), NONE_IDX)
    gd = np.full((nq, k), np.inf, np.float32)
    gc = np.zeros(nq, np.uint32)
    for g in np.unique(qmask):
        sel = np.flatnonzero(qmask == g)
        ids = np.flatnonzero(masks[g] if live is None else masks[g] & live).astype(np.int64)
        if len(ids) == 0:
            continue
        wi, wd, wc = oracle_mod.parallel_top_k(np.ascontiguousarray(host[ids]), np.ascontiguousarray(qs[sel]), k,
                                               size=THREADS, threads=THREADS)
        for j, q in enumerate(sel):
            c = int(wc[j])
            gi[q, :c] = ids[wi[j, :c].astype(np.int64)].astype(np.uint64) + np.uint64(offset)
            gd[q, :c] = wd[j, :c]
            gc[q] = c
    return gi, gd, gc


def _rand_mask(n, rho, seed):
    return np.random.default_rng(seed).random(n) < rho


def _path(bsr_mod, st):
    assert st.search_path & bsr_mod.BSR_PATH_MASK_GROUPS, st.search_path
    assert st.graph_replay == 0
    return bool(st.search_path & bsr_mod.BSR_PATH_MASK_FILTER), bool(st.search_path & bsr_mod.BSR_PATH_MASK_LIST)


# ---- 1. small, odd widths: the list path ---------------------------------------------------
@pytest.fixture(scope="module")
def small(bsr_mod, gpu):
    rng = np.random.default_rng(11)
    n, dim, nq = 3001, 100, 20
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(rows)
    yield ix, rows, qs
    ix.close()


def test_small_list_path(bsr_mod, oracle_mod, small):
    """Four masks (rho = 0.3, seven rows, one row, none) named by 1, 7, 9 and 3 queries -- no group
    size a multiple of the scan's 8 queries -- and a fifth mask no query names.  The small groups are
    below the filter's range in every mode; the rho = 0.3 group (one query) takes the list in the
    list mode and, by the AUTO rule for one query, in auto; in the filter mode §12's rule sends it
    to the filter (3,001 rows are more than one candidate list), so only MASK_LIST is asserted there."""
    ix, rows, qs = small
    n, k = len(rows), 10
    masks = np.zeros((5, n), bool)
    masks[0] = _rand_mask(n, 0.3, 1)
    masks[1, [3, 64, 65, 1000, 2047, 2048, 3000]] = True
    masks[2, 1234] = True
    masks[4] = _rand_mask(n, 0.5, 2)
    qmask = np.array([0] + [1] * 7 + [2] * 9 + [3] * 3, np.uint32)
    qmask = qmask[np.random.default_rng(3).permutation(20)]
    want = _want(oracle_mod, rows, masks, qmask, qs, k)
    assert sorted(set(want[2].tolist())) == [0, 1, 7, 10]
    for mode in ("auto", "list", "filter"):
        got = ix.local_top_k_grouped(qs, k, masks, qmask, mask_mode=mode)
        st = ix.last_stats()
        _same(got, want, mode)
        _tail_is_empty(got, mode)
        filt, lst = _path(bsr_mod, st)
        assert lst, mode
        if mode != "filter":
            assert not filt and st.n_exact_direct == 20 and st.n_fallback == 0, mode
        else:
            assert st.n_exact_direct >= 19, mode
    # the packed form of the same masks
    got = ix.local_top_k_grouped(qs, k, bsr_mod.pack_allow_masks(n, masks=masks), qmask, mask_mode="list")
    _same(got, want, "packed")


# ---- one shard of 40,037 x 768 uniform rows ------------------------------------------------
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
def mixed(oracle_mod, shard):
    """Masks rho = 1/2, 1/4, 1/8, 1/100 named round-robin by the 40 queries; the expected lists."""
    _, rows, qs = shard
    masks = np.stack([_rand_mask(N, rho, int(1 / rho)) for rho in (1 / 2, 1 / 4, 1 / 8, 1 / 100)])
    qmask = (np.arange(40) % 4).astype(np.uint32)
    return masks, qmask, _want(oracle_mod, rows, masks, qmask, qs, 10)


# ---- 2. mixed filter and list groups ---------------------------------------------------------
def test_mixed_filter_and_list(bsr_mod, shard, mixed):
    ix, rows, qs = shard
    masks, qmask, want = mixed
    got = ix.local_top_k_grouped(qs, 10, masks, qmask, mask_mode=bsr_mod.BSR_MASK_FILTER)
    st = ix.last_stats()
    print(f"mixed: fallback={st.n_fallback} exact_direct={st.n_exact_direct} emitted={st.n_emitted} "
          f"path={st.search_path}")
    _same(got, want, "mixed filter")
    _tail_is_empty(got, "mixed filter")
    assert _path(bsr_mod, st) == (True, True)
    assert st.n_exact_direct == int(np.sum(qmask == 3)) == 10
    # (a filter that never certifies must not pass on its fallback alone)
    assert st.n_fallback < 30, st.n_fallback
    assert st.n_queries == 40 and st.n_rescued == 0 and st.n_emitted > 0
    got_l = ix.local_top_k_grouped(qs, 10, masks, qmask, mask_mode=bsr_mod.BSR_MASK_LIST)
    st = ix.last_stats()
    assert _path(bsr_mod, st) == (False, True) and st.n_exact_direct == 40 and st.n_fallback == 0
    _bitwise(got, got_l, "filter vs list")


# ---- 3. one mask per query -------------------------------------------------------------------
def test_one_mask_per_query_filter(bsr_mod, oracle_mod, shard):
    ix, rows, qs = shard
    masks = np.stack([_rand_mask(N, 1 / 2, 100 + s) for s in range(40)])
    qmask = np.random.default_rng(5).permutation(40).astype(np.uint32)
    want = _want(oracle_mod, rows, masks, qmask, qs, 10)
    got = ix.local_top_k_grouped(qs, 10, masks, qmask, mask_mode="filter")
    st = ix.last_stats()
    _same(got, want, "G = nq, filter")
    _tail_is_empty(got, "G = nq, filter")
    filt, _ = _path(bsr_mod, st)
    assert filt and st.n_exact_direct == 0 and st.n_fallback < 40, (st.search_path, st.n_fallback)


LENGTHS = (0, 1, 255, 256, 257, 400, None)  # (None: rho = 1/2, about 20,000 rows)


@pytest.fixture(scope="module")
def lengths(oracle_mod, shard):
    """Forty masks, one per query: list lengths 0, 1, 255, 256, 257, ~400 and ~20,000 in turn."""
    _, rows, qs = shard
    rng = np.random.default_rng(6)
    masks = np.zeros((40, N), bool)
    for g in range(40):
        want_len = LENGTHS[g % len(LENGTHS)]
        if want_len is None:
            masks[g] = rng.random(N) < 0.5
        elif want_len == 400:
            masks[g] = rng.random(N) < 0.01
        else:
            masks[g, rng.choice(N, want_len, replace=False)] = True
    qmask = np.arange(40, dtype=np.uint32)
    return masks, qmask, _want(oracle_mod, rows, masks, qmask, qs, 10)


def test_one_mask_per_query_list_lengths(bsr_mod, shard, lengths):
    """Short and long lists in one launch: workgroups of the grid without a tile in a short list."""
    ix, rows, qs = shard
    masks, qmask, want = lengths
    assert {int(m.sum()) for m in masks} >= {0, 1, 255, 256, 257}
    got = ix.local_top_k_grouped(qs, 10, masks, qmask, mask_mode="list")
    st = ix.last_stats()
    _same(got, want, "lengths")
    _tail_is_empty(got, "lengths")
    assert _path(bsr_mod, st) == (False, True) and st.n_exact_direct == 40


# ---- 4. skinny batch -------------------------------------------------------------------------
def test_skinny_batch(bsr_mod, oracle_mod, shard):
    ix, rows, qs = shard
    masks = np.stack([_rand_mask(N, 1 / 2, 41), _rand_mask(N, 1 / 4, 42)])
    qmask = np.array([1, 0, 1], np.uint32)
    want = _want(oracle_mod, rows, masks, qmask, qs[:3], 10)
    for mode, filt in (("filter", True), ("list", False)):
        got = ix.local_top_k_grouped(qs[:3], 10, masks, qmask, mask_mode=mode)
        st = ix.last_stats()
        _same(got, want, ("skinny", mode))
        _tail_is_empty(got, ("skinny", mode))
        assert _path(bsr_mod, st)[0] == filt, mode
        if filt:
            assert st.n_fallback + st.n_exact_direct < 3


# ---- 5. larger k -----------------------------------------------------------------------------
def test_k50_and_k256(bsr_mod, oracle_mod, shard):
    ix, rows, qs = shard
    masks = np.stack([_rand_mask(N, 1 / 2, 51), _rand_mask(N, 1 / 8, 52)])
    qmask = (np.arange(40) % 2).astype(np.uint32)
    want = _want(oracle_mod, rows, masks, qmask, qs, 50)
    got = ix.local_top_k_grouped(qs, 50, masks, qmask, mask_mode="filter")
    st = ix.last_stats()
    _same(got, want, "k 50")
    # rho = 1/8 is below ks(50) / 128 = 0.19: that group takes the list
    assert _path(bsr_mod, st) == (True, True) and st.n_exact_direct == 20 and st.n_fallback < 20
    want = _want(oracle_mod, rows, masks, qmask[:4], qs[:4], 256)
    got = ix.local_top_k_grouped(qs[:4], 256, masks, qmask[:4], mask_mode="filter")
    st = ix.last_stats()
    _same(got, want, "k 256")
    assert _path(bsr_mod, st) == (False, True) and st.n_exact_direct == 4


# ---- 6. G = 1 is the single-mask search ------------------------------------------------------
def test_one_group_is_the_single_mask_search(bsr_mod, shard):
    ix, rows, qs = shard
    mask = _rand_mask(N, 1 / 2, 61)
    zero = np.zeros(40, np.uint32)
    for mode in ("auto", "list", "filter"):
        one = ix.local_top_k(qs, 10, allow_mask=mask, mask_mode=mode)
        path1 = ix.last_stats().search_path
        grp = ix.local_top_k_grouped(qs, 10, mask[None, :], zero, mask_mode=mode)
        st = ix.last_stats()
        _bitwise(one, grp, mode)
        assert st.search_path & ~bsr_mod.BSR_PATH_MASK_GROUPS == path1, (mode, st.search_path, path1)
    words = np.full((1, (N + 63) // 64), 2 ** 64 - 1, np.uint64)  # (the tail bits past n set too)
    base = ix.local_top_k(qs, 10)
    for mode in ("auto", "list", "filter"):
        _bitwise(base, ix.local_top_k_grouped(qs, 10, words, zero, mask_mode=mode), ("all ones", mode))


# ---- 7. chunked lists ------------------------------------------------------------------------
def test_list_budget_chunks(bsr_mod, shard, lengths, monkeypatch):
    """BSR_MASK_LIST_BUDGET: ~120,000 listed ids in chunks of at most 45,000 (two long lists each: at
    least three chunks), then a budget below the longest list (a chunk per long list)."""
    ix, rows, qs = shard
    masks, qmask, want = lengths
    total = int(masks.sum())
    assert total > 3 * 45_000 - 45_000 and int(masks.sum(1).max()) > 1000
    whole = ix.local_top_k_grouped(qs, 10, masks, qmask, mask_mode="list")
    for budget in (4 * 45_000, 4 * 1000):
        monkeypatch.setenv("BSR_MASK_LIST_BUDGET", str(budget))
        got = ix.local_top_k_grouped(qs, 10, masks, qmask, mask_mode="list")
        monkeypatch.delenv("BSR_MASK_LIST_BUDGET")
        _bitwise(whole, got, budget)
        _same(got, want, budget)


# ---- 8. tombstones ---------------------------------------------------------------------------
def test_tombstones(bsr_mod, oracle_mod, shard):
    import torch
    _, rows, qs = shard
    ix = bsr_mod.Index(D, max_k=64, device=0)
    ix.load(rows)
    rng = np.random.default_rng(8)
    dead = rng.random(N) < 0.3
    dead[64 * 100:64 * 101] = True  # every row of one mask word
    masks = np.stack([_rand_mask(N, rho, 80 + i) for i, rho in enumerate((1 / 2, 1 / 4, 1 / 100))])
    masks[0, 64 * 100:64 * 101] = True
    qmask = (np.arange(40) % 3).astype(np.uint32)
    dw = torch.from_numpy(bsr_mod.pack_allow_masks(N, masks=masks).view(np.int64)).to("cuda:0")
    dm = torch.from_numpy(qmask.view(np.int32)).to("cuda:0")
    dq = torch.from_numpy(qs).to("cuda:0")
    oi = torch.zeros((40, 10), dtype=torch.int64, device="cuda:0")
    od = torch.zeros((40, 10), dtype=torch.float32, device="cuda:0")
    oc = torch.zeros(40, dtype=torch.int32, device="cuda:0")

    def run(mode):
        ix.local_top_k_grouped_device(dq, 40, 10, oi, od, oc, dw, dm, mask_mode=mode)
        return oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32)

    for mode in ("filter", "list"):  # (every buffer of both paths sized before the delete)
        run(mode)
    assert ix.delete(np.flatnonzero(dead)) == int(dead.sum())
    want = _want(oracle_mod, rows, masks, qmask, qs, 10, live=~dead)
    free0 = torch.cuda.mem_get_info(0)[0]
    for mode in ("filter", "list"):
        got = run(mode)
        st = ix.last_stats()
        _same(got, want, ("tombstones", mode))
        _tail_is_empty(got, ("tombstones", mode))
        assert _path(bsr_mod, st)[0] == (mode == "filter")
        assert not np.any(dead[got[0][got[0] != NONE_IDX].astype(np.int64)])
    # the masks are read with the tombstones taken out on the fly: no [G][words] copy is allocated
    assert torch.cuda.mem_get_info(0)[0] >= free0
    ix.close()


# ---- 9. ties and shortcuts within a group ----------------------------------------------------
def test_ties_and_shortcuts(bsr_mod, oracle_mod, gpu):
    rng = np.random.default_rng(31)
    n, dim, off = 12_011, 128, 1_000_000
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    r = 777
    rows[r + 5000] = rows[r]              # duplicate rows, one per mask
    rows[[40, 9000]] = 0.0                # all-zero rows: distance 1.0
    masks = np.stack([_rand_mask(n, 0.5, 1), _rand_mask(n, 0.5, 2)])
    masks[0, [2500, r, 40]] = True
    masks[1, [2500, r, 40]] = False
    masks[0, r + 5000] = False
    masks[1, [r + 5000, 9000]] = True
    qs = rng.uniform(-1, 1, (6, dim)).astype(np.float32)
    qs[0] = rows[2500]                    # equal to a row of its own mask
    qs[1] = rows[2500]                    # equal to a row only the other group's mask allows
    qs[2] = rows[r]                       # its mask holds the row itself ...
    qs[3] = rows[r]                       # ... the other one its duplicate
    qs[4] = 0.0                           # the zero query (the filter cannot serve it)
    qmask = np.array([0, 1, 0, 1, 1, 0], np.uint32)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(rows, global_offset=off)
    want = _want(oracle_mod, rows, masks, qmask, qs, 10, offset=off)
    for mode in ("filter", "list", "auto"):
        got = ix.local_top_k_grouped(qs, 10, masks, qmask, mask_mode=mode)
        _same(got, want, ("ties", mode))
        assert got[0][0, 0] == off + 2500 and got[1][0, 0] == 0.0
        assert off + 2500 not in got[0][1].tolist()
        assert got[0][2, 0] == off + r and got[1][2, 0] == 0.0
        assert got[0][3, 0] == off + r + 5000 and got[1][3, 0] == 0.0
        # the zero query: its mask's zero row is the identical vector (0.0), every other row 1.0 in
        # index order; the zero row of the other mask is absent
        assert got[0][4, 0] == off + 9000 and got[1][4, 0] == 0.0 and off + 40 not in got[0][4].tolist()
        assert np.all(got[1][4, 1:] == 1.0) and np.all(np.diff(got[0][4, 1:].astype(np.int64)) > 0)
    ix.close()


# ---- 10. device inputs -----------------------------------------------------------------------
def test_device_inputs(bsr_mod, shard, mixed):
    import torch
    ix, rows, qs = shard
    masks, qmask, want = mixed
    words = bsr_mod.pack_allow_masks(N, masks=masks)
    dev = dict(w=torch.from_numpy(words.view(np.int64)).to("cuda:0"),
               m=torch.from_numpy(qmask.view(np.int32)).to("cuda:0"), q=torch.from_numpy(qs).to("cuda:0"))
    host = dict(w=words, m=qmask, q=np.ascontiguousarray(qs))
    for on_host in (None, "w", "m", "q", "out"):
        a = {key: (host if key == on_host else dev)[key] for key in dev}
        if on_host == "out":
            oi, od, oc = np.zeros((40, 10), np.uint64), np.zeros((40, 10), np.float32), np.zeros(40, np.uint32)
        else:
            oi = torch.zeros((40, 10), dtype=torch.int64, device="cuda:0")
            od = torch.zeros((40, 10), dtype=torch.float32, device="cuda:0")
            oc = torch.zeros(40, dtype=torch.int32, device="cuda:0")
        for mode in ("filter", "list"):
            ix.local_top_k_grouped_device(a["q"], 40, 10, oi, od, oc, a["w"], a["m"], mask_mode=mode)
            got = (oi, od, oc) if on_host == "out" else (oi.cpu().numpy().view(np.uint64), od.cpu().numpy(),
                                                         oc.cpu().numpy().view(np.uint32))
            _same(got, want, (on_host, mode))
    # device tensors through local_top_k_grouped as well
    _same(ix.local_top_k_grouped(qs, 10, dev["w"], dev["m"]), want, "tensors")


# ---- 11. state isolation ---------------------------------------------------------------------
def test_state_isolation(bsr_mod, shard, mixed):
    """A grouped search between unmasked ones: their results and their graph replay are untouched."""
    ix, rows, qs = shard
    masks, qmask, want = mixed
    first = None
    for rep in range(3):
        got = ix.local_top_k(qs, 10)
        first = first or got
    assert ix.last_stats().graph_replay == 1
    for mode in ("filter", "list"):
        m = ix.local_top_k_grouped(qs, 10, masks, qmask, mask_mode=mode)
        assert ix.last_stats().graph_replay == 0
        _same(m, want, ("between", mode))
    for rep in range(3):
        _bitwise(ix.local_top_k(qs, 10), first, rep)
    assert ix.last_stats().graph_replay == 1


# ---- 12. errors ------------------------------------------------------------------------------
def test_errors(bsr_mod, shard):
    import torch
    ix, rows, qs = shard
    words = bsr_mod.pack_allow_masks(N, masks=np.ones((4, N), bool))
    nw = words.shape[1]
    q = np.ascontiguousarray(qs[:2])
    qm = np.array([0, 3], np.uint32)
    oi, od, oc = np.zeros((2, 10), np.uint64), np.zeros((2, 10), np.float32), np.zeros(2, np.uint32)
    L = bsr_mod.lib()

    def status(h=None, queries=q, k=10, allow=words.ctypes.data, allow_words=nw, n_masks=4, query_mask=qm, mode=0):
        qmp = query_mask if query_mask is None or isinstance(query_mask, int) else (
            query_mask.data_ptr() if hasattr(query_mask, "data_ptr") else query_mask.ctypes.data)
        return L.bsr_local_top_k_masked_groups(h or ix._h, queries.ctypes.data, 2, k, allow, allow_words, n_masks, qmp,
                                               mode, oi.ctypes.data, od.ctypes.data, oc.ctypes.data)

    assert status() == 0
    assert status(n_masks=0) == -1
    assert status(query_mask=np.array([0, 4], np.uint32)) == -1
    assert b"query_mask" in L.bsr_last_error()
    assert status(query_mask=torch.tensor([4, 0], dtype=torch.int32, device="cuda:0")) == -1
    assert status(query_mask=np.array([2 ** 32 - 1, 0], np.uint32), mode=bsr_mod.BSR_MASK_FILTER) == -1
    # (wrong word counts are refused before a word is read)
    assert status(allow_words=nw - 1) == -1
    assert status(allow_words=nw + 1) == -1
    assert status(mode=3) == -1
    assert status(k=0) == -1
    assert status(k=257) == -1
    bad = q.copy()
    bad[1, 5] = np.nan
    assert status(queries=bad) == -2
    assert status(queries=bad, mode=bsr_mod.BSR_MASK_LIST) == -2
    assert status(allow=None) == -1
    assert status(query_mask=None) == -1
    # the index still searches
    got = ix.local_top_k_grouped(q, 10, np.ones((4, N), bool), qm)
    assert np.all(got[2] == 10)
    _bitwise(got, ix.local_top_k(q, 10), "after the errors")
    with pytest.raises(bsr_mod.BsrError):
        ix.local_top_k_grouped(q, 10, np.ones((4, N), bool), np.zeros(3, np.uint32))
    empty = bsr_mod.Index(D, max_k=16, device=0)
    assert status(h=empty._h) == -7
    empty.close()
    assert isinstance(ctypes.c_uint32(1).value, int)


# ---- 13. seeded sweep ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_seeded_sweep(bsr_mod, oracle_mod, gpu, seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([700, 3001, 12_011, 40_037]))
    if seed == 0:
        n = 40_037
    dim = int(rng.choice([100, 768, 1100]))
    nq = int(rng.integers(1, 41))
    G = int(rng.integers(1, nq + 1))
    k = int(rng.choice([1, 10, 50]))
    off = int(rng.choice([0, 5_000_000_000]))
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    rho = rng.choice([0.0, 0.001, 0.02, 0.1, 0.3, 0.6, 1.0], G)
    masks = rng.random((G, n)) < rho[:, None]
    qmask = rng.integers(0, G, nq).astype(np.uint32)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(rows, global_offset=off)
    want = _want(oracle_mod, rows, masks, qmask, qs, k, offset=off)
    for mode in rng.permutation(["auto", "list", "filter"])[:2]:
        got = ix.local_top_k_grouped(qs, k, masks, qmask, mask_mode=str(mode))
        ctx = (seed, n, dim, nq, G, k, str(mode))
        _same(got, want, ctx)
        _tail_is_empty(got, ctx)
        _path(bsr_mod, ix.last_stats())
    ix.close()
