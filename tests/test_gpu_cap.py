"""Capped search (bsr_local_top_k_capped) through the C ABI, whole calls, bit for bit.

The model (kcheck_cap.cap_model): from the full distance vector of a query over the stored rows
(oracle.np_cosine_distances, the reference's bits) the deleted and disallowed rows are dropped, the
rest is ordered by (distance, index), a row is kept while fewer than m rows of its group were kept,
and the first k kept rows are the result.  Counts, global indices, order, f32 distance bits, groups
and the (~0, +inf, ~0u) tail are compared exactly.

The shards are tests/test_gpu_collapse.py's recipe, restated: U(-1, 1) rows, query q a noisy copy of
row 100 + 37 q, six near and two exact copies of that row planted elsewhere, row_group = i // 7 for
the unplanted rows; for the three queries SCAN_Q another 80 near copies (noise 1e-3) of the nearest
row are planted, and the nearest row with all its 88 copies is one group.  Those queries' 64 nearest
rows lie in that one group of 89, so at fetch_k = 64 and m < k = 10 the walk keeps m rows and cannot
certify them: they take the capped group scan; every other query keeps 10 rows among its first 64."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import kcheck_cap as kp

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID, E_NONFINITE = -1, -2
NONE_IDX = np.uint64(0xFFFFFFFFFFFFFFFF)
OFFSET = 5_000_000_000
SCAN_Q = (1, 17, 33)


def make_shard(n, dim, nq, seed, plant=True, extra=()):
    """(rows, queries, row_group, n_groups); see the module's docstring."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-1, 1, (n, dim)).astype(F)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(F)
    rg = np.arange(n, dtype=np.int64) // 7
    ng = int(rg.max()) + 1
    if plant:
        spots = rng.choice(np.arange(2000, n), (nq, 8), replace=False)
        for q in range(nq):
            r = 100 + 37 * q
            qs[q] = rows[r] + rng.normal(0, 0.3, dim).astype(F)
            for j in range(6):
                rows[spots[q, j]] = rows[r] + rng.normal(0, 1e-3, dim).astype(F)
            rows[spots[q, 6]] = rows[r]
            rows[spots[q, 7]] = rows[r]
        free = np.setdiff1d(np.arange(2000, n), spots.ravel())
        more = rng.choice(free, (len(extra), 80), replace=False)
        for e, q in enumerate(extra):
            r = 100 + 37 * q
            for s in more[e]:
                rows[s] = rows[r] + rng.normal(0, 1e-3, dim).astype(F)
            rg[r] = rg[spots[q]] = rg[more[e]] = ng
            ng += 1
    return rows, qs, rg.astype(np.uint32), ng


def all_dists(oracle_mod, stored, qs):
    """The reference's distance of every stored row to every query: [nq][n] f32."""
    with ThreadPoolExecutor(8) as ex:
        return np.stack(list(ex.map(lambda q: oracle_mod.np_cosine_distances(stored, q), qs)))


def same(got, want, ctx=""):
    """got / want: (idx, dist, count[, group])."""
    assert np.array_equal(got[2], want[2]), (ctx, "counts", got[2], want[2])
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1))
    assert bad.size == 0, (ctx, "indices", bad[:8], got[0][bad[0]], want[0][bad[0]])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (ctx, "distance bits")
    if len(got) > 3 and got[3] is not None:
        assert np.array_equal(got[3], want[3]), (ctx, "groups")


def same_bytes(a, b, ctx=""):
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), ctx


_shards = {}


def shard(bsr_mod, oracle_mod, name):
    """(index, stored rows, queries, row_group, n_groups, distances [nq][n]) of a shared, never
    modified shard."""
    if name not in _shards:
        n, dim, nq, seed, plant, dtype = {
            "big": (20000, 768, 40, 7, True, bsr_mod.BSR_F32),
            "600": (600, 768, 12, 8, False, bsr_mod.BSR_F32),
            "130": (130, 768, 6, 12, False, bsr_mod.BSR_F32),
            "40": (40, 768, 5, 9, False, bsr_mod.BSR_F32),
            "bf16": (5000, 256, 12, 11, True, bsr_mod.BSR_BF16),
        }[name]
        rows, qs, rg, ng = make_shard(n, dim, nq, seed, plant, SCAN_Q if name == "big" else (1,) if plant else ())
        ix = bsr_mod.Index(dim, max_k=256, device=0, dtype=dtype)
        if dtype == bsr_mod.BSR_BF16:
            bits = (rows.view(np.uint32) >> 16).astype(np.uint16)
            rows = (bits.astype(np.uint32) << 16).view(F)  # (the widened values the index keeps)
            ix.load(bits, global_offset=OFFSET)
        else:
            ix.load(rows, global_offset=OFFSET)
        _shards[name] = (ix, rows, qs, rg, ng, all_dists(oracle_mod, rows, qs))
    return _shards[name]


def model(dists, rg, k, m, sel=None, **kw):
    sel = range(len(dists)) if sel is None else sel
    if isinstance(kw.get("allowed"), list):
        kw["allowed"] = [kw["allowed"][q] for q in sel]
    return kp.cap_batch([dists[q] for q in sel], rg, k, m, offset=kw.pop("offset", OFFSET), **kw)


# ---- 1. the big shard: the walk and the scan -------------------------------------------------------
@pytest.mark.parametrize("m", [2, 3])
def test_big_shard(bsr_mod, oracle_mod, gpu, m):
    ix, rows, qs, rg, ng, dists = shard(bsr_mod, oracle_mod, "big")
    P = bsr_mod
    nq, k, fetch_k = 40, 10, 64
    want = model(dists[:nq], rg, k, m)
    got = ix.capped_search(qs[:nq], k, rg, m, fetch_k=fetch_k, return_groups=True)
    same(got, want, "the batch")
    st = ix.last_stats()
    assert st.search_path & P.BSR_PATH_CAP and st.search_path & P.BSR_PATH_CAP_SCAN and st.n_queries == nq
    assert not st.search_path & (P.BSR_PATH_COLLAPSE | P.BSR_PATH_COLLAPSE_SCAN | P.BSR_PATH_RANGE | P.BSR_PATH_MMR |
                                 P.BSR_PATH_MASK_LIST | P.BSR_PATH_MASK_FILTER)
    assert (got[2] == k).all()
    # the construction: the planted queries' 64 nearest rows are one group
    top = ix.local_top_k(qs[:nq], fetch_k)[0]
    for q in range(nq):
        groups = rg[(top[q] - np.uint64(OFFSET)).astype(np.int64)]
        assert (len(set(groups.tolist())) == 1) == (q in SCAN_Q), q
        # at most m rows of a group, and a planted query's result starts with m rows of its group
        assert np.bincount(got[3][q]).max() <= m
        if q in SCAN_Q:
            assert (got[3][q][:m] == rg[100 + 37 * q]).all() and (got[3][q][m:] != rg[100 + 37 * q]).all()
    # the same batch without the planted queries: no scan, the same rows
    keep = [q for q in range(nq) if q not in SCAN_Q]
    got2 = ix.capped_search(qs[keep], k, rg, m, n_groups=ng, fetch_k=fetch_k, return_groups=True)
    same(got2, tuple(w[keep] for w in want), "without the planted queries")
    st = ix.last_stats()
    assert st.search_path & P.BSR_PATH_CAP and not st.search_path & P.BSR_PATH_CAP_SCAN
    # three planted queries alone (a launch of three), and without the groups
    same(ix.capped_search(qs[list(SCAN_Q)], k, rg, m, fetch_k=fetch_k, return_groups=True),
         tuple(w[list(SCAN_Q)] for w in want), "the planted queries")
    same(ix.capped_search(qs[:nq], k, rg, m, fetch_k=fetch_k), want[:3], "no out_group")


def test_fetch_k_independence(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, rg, ng, dists = shard(bsr_mod, oracle_mod, "big")
    nq, k, m = 40, 10, 2
    outs = [ix.capped_search(qs[:nq], k, rg, m, fetch_k=fk, return_groups=True) for fk in (10, 64, 256)]
    for o in outs[1:]:
        same_bytes(outs[0], o, "fetch_k")
    same(outs[0], model(dists[:nq], rg, k, m), "fetch_k = 10")
    # the default fetch_k
    same(ix.capped_search(qs[:8], k, rg, m, return_groups=True), model(dists[:8], rg, k, m), "default fetch_k")


def test_identities(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, rg, ng, dists = shard(bsr_mod, oracle_mod, "big")
    n, nq, k = len(rows), 40, 10
    P = bsr_mod
    # per_group = 1: the collapsed search, byte for byte (planted queries scan in both)
    for kw in (dict(fetch_k=64), dict(fetch_k=64, allow_mask=np.random.default_rng(5).random(n) < 0.5)):
        a = ix.collapsed_search(qs[:nq], k, rg, return_groups=True, **kw)
        b = ix.capped_search(qs[:nq], k, rg, 1, return_groups=True, **kw)
        same_bytes(a, b, "per_group = 1")
        if "allow_mask" not in kw:
            assert ix.last_stats().search_path & P.BSR_PATH_CAP_SCAN
    # per_group >= k: the plain search, and no scan, though the planted queries' lists are one group
    plain = ix.local_top_k(qs[:nq], k)
    for m, fk in ((16, 64), (10, 10), (11, 256)):
        got = ix.capped_search(qs[:nq], k, rg, m, fetch_k=fk, return_groups=True)
        same(got[:3], plain, ("per_group >= k", m))
        assert np.array_equal(got[3], rg[(plain[0] - np.uint64(OFFSET)).astype(np.int64)])
        st = ix.last_stats()
        assert st.search_path & P.BSR_PATH_CAP and not st.search_path & P.BSR_PATH_CAP_SCAN
    # all rows in one group: the top-min(m, k)
    one_rg = np.zeros(n, np.uint32)
    for m, kk in ((3, 10), (16, 10), (4, 2)):
        got = ix.capped_search(qs[:12], kk, one_rg, m, return_groups=True)
        c = min(m, kk)
        top = ix.local_top_k(qs[:12], c)
        assert (got[2] == c).all() and np.array_equal(got[0][:, :c], top[0])
        assert np.array_equal(got[1][:, :c].view(np.uint32), top[1].view(np.uint32)) and (got[3][:, :c] == 0).all()
        assert (got[0][:, c:] == NONE_IDX).all() and np.isposinf(got[1][:, c:]).all()
        assert (got[3][:, c:] == kp.GROUP_NONE).all()
        same(got, model(dists[:12], one_rg, kk, m), "one group")


def test_counts(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, rg, ng, dists = shard(bsr_mod, oracle_mod, "big")
    n, nq, k = len(rows), 9, 10
    rg4 = (np.arange(n) % 4).astype(np.uint32)
    got = ix.capped_search(qs[:nq], k, rg4, 2, return_groups=True)
    same(got, model(dists[:nq], rg4, k, 2), "four groups")
    assert (got[2] == 8).all() and (got[0][:, 8:] == NONE_IDX).all() and np.isposinf(got[1][:, 8:]).all()
    assert (got[3][:, 8:] == kp.GROUP_NONE).all()
    assert (np.sort(got[3][:, :8], axis=1) == np.repeat(np.arange(4), 2)).all()
    assert ix.last_stats().search_path & bsr_mod.BSR_PATH_CAP_SCAN
    # n_groups above the ids in use changes nothing
    same_bytes(ix.capped_search(qs[:nq], k, rg4, 2, n_groups=1000, return_groups=True), got, "n_groups = 1000")


# ---- 2. the other shards ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,fetch_k", [("600", 10, 64), ("130", 10, 32), ("40", 50, 64), ("bf16", 10, 64)])
def test_other_shards(bsr_mod, oracle_mod, gpu, name, k, fetch_k):
    ix, rows, qs, rg, ng, dists = shard(bsr_mod, oracle_mod, name)
    for m in (2, 3):
        got = ix.capped_search(qs, k, rg, m, fetch_k=fetch_k, return_groups=True)
        same(got, model(dists, rg, k, m), (name, m))
        st = ix.last_stats()
        print(f"{name} m={m}: path={st.search_path} direct={st.n_exact_direct} fallback={st.n_fallback} counts={got[2][:4]}")
        assert st.search_path & bsr_mod.BSR_PATH_CAP
        if name == "40":  # 6 groups of at most 7 rows, and the list holds every row
            assert (got[2] == min(k, sum(min(m, int(c)) for c in np.bincount(rg)))).all()
            assert not st.search_path & bsr_mod.BSR_PATH_CAP_SCAN
        if name == "bf16":
            assert st.search_path & bsr_mod.BSR_PATH_CAP_SCAN  # (query 1 is planted)
    # three groups, interleaved, m = 3: nine rows to keep, every query scans unless its list is the
    # whole shard; then m = 8 and 16 with k above the list (tables of 8 and 16 entries per group)
    rg3 = (np.arange(len(rows)) % 3).astype(np.uint32)
    same(ix.capped_search(qs, k, rg3, 3, fetch_k=fetch_k, return_groups=True), model(dists, rg3, k, 3), (name, "3 groups"))
    if name in ("600", "bf16"):
        for m in (8, 16):
            got = ix.capped_search(qs, 60, rg3, m, fetch_k=64, return_groups=True)
            same(got, model(dists, rg3, 60, m), (name, "3 groups", m))
            assert (got[2] == 3 * m).all() and ix.last_stats().search_path & bsr_mod.BSR_PATH_CAP_SCAN


def test_shard_without_a_live_row(bsr_mod, gpu):
    rng = np.random.default_rng(3)
    ix = bsr_mod.Index(16, max_k=64, device=0)
    ix.load(rng.uniform(-1, 1, (10, 16)).astype(F), global_offset=OFFSET)
    assert ix.delete(np.arange(10, dtype=np.uint64) + np.uint64(OFFSET)) == 10
    for kw in (dict(), dict(allow_mask=np.ones(10, bool))):
        got = ix.capped_search(rng.uniform(-1, 1, (3, 16)).astype(F), 4, np.arange(10) // 3, 2, return_groups=True, **kw)
        assert (got[2] == 0).all() and (got[0] == NONE_IDX).all() and np.isposinf(got[1]).all()
        assert (got[3] == kp.GROUP_NONE).all()
    ix.close()


# ---- 3. masks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["list", "filter", "auto"])
def test_one_mask(bsr_mod, oracle_mod, gpu, mode):
    ix, rows, qs, rg, ng, dists = shard(bsr_mod, oracle_mod, "big")
    n, nq, k, fetch_k, m = len(rows), 8, 10, 64, 2
    P = bsr_mod
    allowed = np.random.default_rng(31).random(n) < 0.5
    got = ix.capped_search(qs[:nq], k, rg, m, fetch_k=fetch_k, allow_mask=allowed, mask_mode=mode, return_groups=True)
    same(got, model(dists[:nq], rg, k, m, allowed=allowed), mode)
    st = ix.last_stats()
    assert st.search_path & P.BSR_PATH_CAP and st.graph_replay == 0
    assert st.search_path & (P.BSR_PATH_MASK_LIST if mode == "list" else P.BSR_PATH_MASK_LIST | P.BSR_PATH_MASK_FILTER)
    assert not st.search_path & P.BSR_PATH_MASK_GROUPS
    assert allowed[(got[0] - np.uint64(OFFSET)).astype(np.int64)].all()


def test_three_masks(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, rg, ng, dists = shard(bsr_mod, oracle_mod, "big")
    n, nq, k, fetch_k, m = len(rows), 9, 10, 64, 3
    rng = np.random.default_rng(32)
    masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.05, np.zeros(n, bool)])
    masks[2, :14] = True  # 14 rows of 2 groups: 6 rows to keep, and a list that holds them all
    qm = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2], np.uint32)
    got = ix.capped_search(qs[:nq], k, rg, m, fetch_k=fetch_k, allow_masks=masks, query_mask=qm, return_groups=True)
    same(got, model(dists[:nq], rg, k, m, allowed=[masks[g] for g in qm]), "groups")
    st = ix.last_stats()
    assert st.search_path & bsr_mod.BSR_PATH_CAP and st.search_path & bsr_mod.BSR_PATH_MASK_GROUPS
    assert list(got[2]) == [10, 10, 6] * 3


def test_mask_removes_every_kept_row(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, rg, ng, dists = shard(bsr_mod, oracle_mod, "big")
    n, nq, k, fetch_k, m = len(rows), 20, 10, 64, 2
    P = bsr_mod
    free = model(dists[:nq], rg, k, m)
    # a mask without the kept rows of any query: the next rows of their groups take their places
    kept = (free[0].ravel() - np.uint64(OFFSET)).astype(np.int64)
    allowed = np.ones(n, bool)
    allowed[kept] = False
    got = ix.capped_search(qs[:nq], k, rg, m, fetch_k=fetch_k, allow_mask=allowed, return_groups=True)
    same(got, model(dists[:nq], rg, k, m, allowed=allowed), "kept rows removed")
    assert not np.isin(got[0], free[0]).any()
    assert ix.last_stats().search_path & P.BSR_PATH_CAP_SCAN
    # a mask without the whole planted group of query 1: that query needs no scan any more, query 17
    # still does, and its scan runs under the mask
    allowed = rg != rg[100 + 37 * 1]
    for masks_kw in (dict(allow_mask=allowed),
                     dict(allow_masks=np.stack([allowed, np.ones(n, bool)]), query_mask=np.arange(nq) % 2)):
        got = ix.capped_search(qs[:nq], k, rg, m, fetch_k=fetch_k, return_groups=True, **masks_kw)
        if "query_mask" in masks_kw:
            want = model(dists[:nq], rg, k, m, allowed=[allowed if q % 2 == 0 else np.ones(n, bool) for q in range(nq)])
        else:
            want = model(dists[:nq], rg, k, m, allowed=allowed)
        same(got, want, ("planted group removed", sorted(masks_kw)))
        assert ix.last_stats().search_path & P.BSR_PATH_CAP_SCAN
    # (query 1 has the odd mask: its planted group is allowed, its first rows are the planted group's)
    assert (got[3][1, :m] == rg[100 + 37 * 1]).all() and (got[3][17, :m] == rg[100 + 37 * 17]).all()


# ---- 4. tombstones, update, compaction -------------------------------------------------------------
def test_delete_update_compact(bsr_mod, oracle_mod, gpu):
    rows, qs, rg, ng = make_shard(20000, 768, 8, 7, True, (1,))
    rows = rows.copy()
    n, nq, k, fetch_k, m = len(rows), 8, 10, 64, 2
    ix = bsr_mod.Index(768, max_k=256, device=0)
    ix.load(rows, global_offset=OFFSET)
    live = np.ones(n, bool)

    def check(ctx, stored=rows, groups=rg, alive=None, offset=OFFSET):
        d = all_dists(oracle_mod, stored, qs)
        want = kp.cap_batch(d, groups, k, m, live=live if alive is None else alive, offset=offset)
        got = ix.capped_search(qs, k, groups, m, n_groups=ng, fetch_k=fetch_k, return_groups=True)
        same(got, want, ctx)
        return got

    got = check("loaded")
    # delete every kept row: the next rows of each group take their places
    kept = np.unique(got[0].ravel())
    assert ix.delete(kept) == len(kept)
    live[(kept - np.uint64(OFFSET)).astype(np.int64)] = False
    got2 = check("tombstones")
    assert not np.isin(got2[0], kept).any()
    # update: a live row that is not kept becomes a copy of the query itself, the first of its group
    upd = np.array([5000 + 11 * q for q in range(nq)], np.int64)
    assert live[upd].all() and not np.isin(upd + OFFSET, got2[0].astype(np.int64)).any()
    rows[upd] = qs
    ix.update((upd + OFFSET).astype(np.uint64), qs)
    got3 = check("update")
    assert np.array_equal(got3[0][:, 0], (upd + OFFSET).astype(np.uint64)) and (got3[1][:, 0] == 0).all()
    assert np.array_equal(got3[3][:, 0], rg[upd])
    # compact: the live rows packed, a new offset, row_group remapped through the returned ids
    old = ix.compact(global_offset=123)
    assert np.array_equal(old, (np.flatnonzero(live) + OFFSET).astype(np.uint64))
    rg_new = rg[(old - np.uint64(OFFSET)).astype(np.int64)]
    check("compact", stored=rows[live], groups=rg_new, alive=np.ones(int(live.sum()), bool), offset=123)
    ix.close()


# ---- 5. device buffers -----------------------------------------------------------------------------
def test_device_buffers(bsr_mod, oracle_mod, gpu):
    import torch
    ix, rows, qs, rg, ng, dists = shard(bsr_mod, oracle_mod, "big")
    n, nq, k, fetch_k, m = len(rows), 8, 10, 64, 2
    want = model(dists[:nq], rg, k, m)
    dev = torch.device("cuda:0")
    q = torch.from_numpy(qs[:nq]).to(dev)
    rg_dev = torch.from_numpy(rg.view(np.int32)).to(dev)

    def outs(on_dev):
        t = [torch.full((nq, k), 7, dtype=torch.int64), torch.full((nq, k), 7, dtype=torch.float32),
             torch.full((nq,), 7, dtype=torch.int32), torch.full((nq, k), 7, dtype=torch.int32)]
        return [x.to(dev) if on_dev else x for x in t]

    def read(oi, od, oc, og):
        return (oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32),
                og.cpu().numpy().view(np.uint32))

    # everything on the device (query 1 scans: the finish writes the caller's arrays too)
    oi, od, oc, og = outs(True)
    ix.capped_search_device(q, nq, k, fetch_k, m, rg_dev, ng, oi, od, oc, out_group=og)
    same(read(oi, od, oc, og), want, "device everything")
    assert ix.last_stats().search_path & bsr_mod.BSR_PATH_CAP_SCAN
    # out_group NULL: the other three as before, the group tensor untouched
    oi, od, oc, og = outs(True)
    ix.capped_search_device(q, nq, k, fetch_k, m, rg_dev, ng, oi, od, oc)
    same(read(oi, od, oc, og)[:3], want[:3], "no groups")
    assert (og == 7).all()
    # a host row_group with device outputs
    oi, od, oc, og = outs(True)
    ix.capped_search_device(q, nq, k, fetch_k, m, rg, ng, oi, od, oc, out_group=og)
    same(read(oi, od, oc, og), want, "host row_group, device outputs")
    # mixed outputs: host indices and groups, device distances and counts
    oi, od, oc, og = outs(True)
    hi, _, _, hg = outs(False)
    ix.capped_search_device(q, nq, k, fetch_k, m, rg_dev, ng, hi, od, oc, out_group=hg)
    same(read(hi, od, oc, hg), want, "mixed outputs")
    # a device mask and a device query_mask, host outputs; the wrapper with a tensor row_group
    allowed = np.random.default_rng(31).random(n) < 0.5
    words = np.stack([bsr_mod.pack_allow_mask(n, mask=allowed), bsr_mod.pack_allow_mask(n, mask=np.ones(n, bool))])
    words_dev = torch.from_numpy(words.view(np.int64)).to(dev)
    qm = (np.arange(nq) % 2).astype(np.int32)
    hi, hd, hc, hg = outs(False)
    ix.capped_search_device(np.ascontiguousarray(qs[:nq]), nq, k, fetch_k, m, rg_dev, ng, hi, hd, hc, out_group=hg,
                            allow_words=words_dev, query_mask=torch.from_numpy(qm).to(dev))
    wantm = model(dists[:nq], rg, k, m, allowed=[allowed if g == 0 else np.ones(n, bool) for g in qm])
    same(read(hi, hd, hc, hg), wantm, "device masks")
    same(ix.capped_search(qs[:nq], k, rg_dev, m, n_groups=ng, return_groups=True), want, "tensor row_group")


# ---- 6. the candidate search keeps its graphs ------------------------------------------------------
@pytest.mark.parametrize("nq", [40, 3])
def test_graph_replay(bsr_mod, oracle_mod, gpu, nq):
    ix, rows, qs, rg, ng, dists = shard(bsr_mod, oracle_mod, "big")
    k, fetch_k, m = 7, 52, 2  # (a shape of this test's own)
    want = model(dists[:nq], rg, k, m)
    replays = []
    for rep in range(4):
        got = ix.capped_search(qs[:nq], k, rg, m, n_groups=ng, fetch_k=fetch_k, return_groups=True)
        same(got, want, ("rep", rep))
        st = ix.last_stats()
        assert st.search_path & bsr_mod.BSR_PATH_CAP
        replays.append(st.graph_replay)
    print(f"nq={nq}: graph_replay per call {replays}, path={st.search_path}")
    # from the third call on, wherever the plain search of this shape replays (a batch whose queries
    # all certify; a rerun of the self-thresholded path launches directly)
    plain = [None] * 3
    for rep in range(3):
        plain[rep] = ix.local_top_k(qs[:nq], fetch_k)
        plain_replay = ix.last_stats().graph_replay
    assert replays[2] == replays[3] == plain_replay
    if not st.search_path & bsr_mod.BSR_PATH_TOP_RERUN:
        assert replays[2] == 1
    # and a plain search afterwards is still bit-exact
    wi, wd, wc = oracle_mod.parallel_top_k(rows, qs[:nq], fetch_k, size=8, threads=8)
    same(plain[2], (wi + np.uint64(OFFSET), wd, wc), "plain after a capped search")


# ---- 7. the table budget ---------------------------------------------------------------------------
def test_table_budget(bsr_mod, oracle_mod, gpu, monkeypatch):
    ix, rows, qs, rg, ng, dists = shard(bsr_mod, oracle_mod, "big")
    n, nq, k, m = len(rows), 40, 10, 2
    rg4 = (np.arange(n) % 4).astype(np.uint32)  # (8 rows to keep: every query scans)
    for groups, n_groups in ((rg, ng), (rg4, 4)):
        ref = ix.capped_search(qs[:nq], k, groups, m, n_groups=n_groups, fetch_k=64, return_groups=True)
        assert ix.last_stats().search_path & bsr_mod.BSR_PATH_CAP_SCAN
        table = 8 * m * n_groups
        for budget in (table, 1, 3 * table, 3 * table + table - 1):  # one query a round (twice), three (twice)
            monkeypatch.setenv("BSR_COLLAPSE_TABLE_BUDGET", str(budget))
            got = ix.capped_search(qs[:nq], k, groups, m, n_groups=n_groups, fetch_k=64, return_groups=True)
            same_bytes(ref, got, budget)
        monkeypatch.delenv("BSR_COLLAPSE_TABLE_BUDGET")
    same(ref, model(dists[:nq], rg4, k, m), "four groups, every query scanned")


# ---- 8. errors -------------------------------------------------------------------------------------
def test_errors_leave_outputs_untouched(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, rg, ng, dists = shard(bsr_mod, oracle_mod, "big")
    n, nq, k, m = len(rows), 4, 5, 2
    oi, od = np.full((nq, k), 7, np.uint64), np.full((nq, k), 7, F)
    oc, og = np.full(nq, 7, np.uint32), np.full((nq, k), 7, np.uint32)

    def untouched():
        return (oi == 7).all() and (od == 7).all() and (oc == 7).all() and (og == 7).all()

    q = np.ascontiguousarray(qs[:nq])
    # per_group out of range
    for bad_m in (0, 17):
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.capped_search_device(q, nq, k, 20, bad_m, rg, ng, oi, od, oc, out_group=og)
        assert e.value.status == E_INVALID and "per_group" in str(e.value) and untouched()
    # a row_group entry = n_groups (found on the device), at either end
    for pos in (0, n - 1):
        bad_rg = rg.copy()
        bad_rg[pos] = ng
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.capped_search_device(q, nq, k, 20, m, bad_rg, ng, oi, od, oc, out_group=og)
        assert e.value.status == E_INVALID and "n_groups" in str(e.value) and untouched()
    # row_group of the wrong length
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.capped_search_device(q, nq, k, 20, m, rg[:-1].copy(), ng, oi, od, oc, out_group=og)
    assert e.value.status == E_INVALID and "row_group_len" in str(e.value) and untouched()
    # a NaN query: as the candidate search reports it
    bad = q.copy()
    bad[2, 17] = np.nan
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.capped_search_device(bad, nq, k, 20, m, rg, ng, oi, od, oc, out_group=og)
    assert e.value.status == E_NONFINITE and untouched()
    # allow_words of the wrong length: as the masked search reports it
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.capped_search_device(q, nq, k, 20, m, rg, ng, oi, od, oc, out_group=og, allow_words=np.zeros(3, np.uint64))
    assert e.value.status == E_INVALID and untouched()
    # the index still answers
    same(ix.capped_search(q, k, rg, m, return_groups=True), model(dists[:nq], rg, k, m), "after the errors")
