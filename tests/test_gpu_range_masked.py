"""Masked range search (bsr_local_range_search_masked) through the C ABI: every row
that is in query q's allow mask, not deleted, and within radius[q] of the query -- exact.

The model needs no tolerance: a row's reference distance does not depend on the other rows, so the
expected list of query q is the reference's whole list over the shard --
oracle.local_top_k(all rows, 0, 1, n, q), computed once per shard -- restricted to the allowed live
rows (which keeps its order) and cut at distance <= radius[q].  Counts, global indices, order and
f32 distance bits, with the (~0, +inf) tail; a count above the capacity leaves only the tail."""
import numpy as np
import pytest

from test_gpu_range import (NONE_IDX, cluster_rows, cut, kth_radius, make_shard, rows_at_distance, same, shard,
                            sorted_lists)

pytestmark = pytest.mark.gpu

F = np.float32
E_INVALID, E_NONFINITE = -1, -2
NEG_INF = F(-np.inf)
OFFSET = 7_000_000_000  # (the shared shards' global offset, test_gpu_range.shard)
MODES = ("list", "filter", "auto")


def restrict(lists, allowed):
    """The lists restricted to the rows with allowed[row] (a bool array over the shard, or one per query)."""
    out = []
    for q, (oi, od) in enumerate(lists):
        a = allowed[q] if np.ndim(allowed) == 2 else allowed
        keep = a[oi.astype(np.int64)]
        out.append((oi[keep], od[keep]))
    return out


def want_for(lists, allowed, radius, capacity, n, offset):
    return cut(restrict(lists, allowed), np.arange(n), radius, capacity, offset)


def radii_in_mask(lists_r, lists, ms, below):
    """radius[q] = the exact distance of query q's ms[q]-th nearest ALLOWED row -- of the last allowed
    row of its planted cluster (distance < 0.2) where the mask left fewer, of the mask's nearest row
    where it left none of the cluster; an empty mask: of the shard's ms[q]-th -- or one f32 below it."""
    r = np.array([(od_r[min(m, max(1, int(np.count_nonzero(od_r < 0.2)))) - 1] if len(od_r) else od[m - 1])
                  for (_, od_r), (_, od), m in zip(lists_r, lists, ms)], F)
    return np.nextafter(r, NEG_INF) if below else r


def rho_mask(rng, n, rho):
    return np.ones(n, bool) if rho == 1 else np.zeros(n, bool) if rho == 0 else rng.random(n) < rho


# ---- 1. one mask ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", [1, 1 / 2, 1 / 16, 1 / 1000, 0])
@pytest.mark.parametrize("name", ["768", "130"])
def test_one_mask(bsr_mod, oracle_mod, gpu, name, rho):
    ix, rows, qs, lists, ms = shard(bsr_mod, oracle_mod, name)
    n = len(rows)
    rng = np.random.default_rng(int(rho * 5000) + n)
    mask = rho_mask(rng, n, rho)  # (a random mask takes part of each planted cluster)
    P = bsr_mod
    for nq, capacity in ((40, 64), (3, 512)):
        lr = restrict(lists[:nq], mask)
        for below in (False, True):
            radius = radii_in_mask(lr, lists[:nq], ms[:nq], below)
            far = int(np.count_nonzero(radius >= 0.2))  # (queries whose mask holds no row of their cluster)
            assert 0 < radius.min() and (far == 0 or 0 < rho <= 1 / 16)
            want = want_for(lists[:nq], mask, radius, capacity, n, OFFSET)
            res = {}
            for mode in MODES:
                got = ix.range_search(qs[:nq], radius, max_results=capacity, allow_mask=mask, mask_mode=mode)
                st = ix.last_stats()
                print(f"{name} rho={rho:.4f} nq={nq} below={below} {mode}: A={int(mask.sum())} counts<={want[2].max()} "
                      f"emitted={st.n_emitted} direct={st.n_exact_direct} fallback={st.n_fallback} path={st.search_path}")
                same(got, want, (name, rho, nq, below, mode))
                assert st.n_queries == nq and st.graph_replay == 0
                assert not (st.search_path & (P.BSR_PATH_RANGE_SCAN | P.BSR_PATH_MASK_GROUPS))
                if mode == "filter":
                    # the emitted lists are the unmasked search's: below the cap on these shards for
                    # every radius inside a cluster, so only the far queries can leave the filter
                    assert st.n_fallback + st.n_exact_direct <= far
                    assert st.search_path & ~P.BSR_PATH_MASK_LIST == P.BSR_PATH_RANGE | P.BSR_PATH_MASK_FILTER
                    assert bool(st.search_path & P.BSR_PATH_MASK_LIST) == (st.n_fallback + st.n_exact_direct > 0)
                    assert st.n_emitted >= int(want[2][radius < 0.2].sum())
                if mode == "list":
                    assert st.search_path == P.BSR_PATH_RANGE | P.BSR_PATH_MASK_LIST
                    assert st.n_exact_direct == nq and st.n_fallback == 0 and st.n_emitted == 0
                res[mode] = got
            same(res["filter"], res["list"], "the modes agree")
            same(res["auto"], res["list"], "the modes agree")
            if rho > 1 / 1000 and not below:
                assert (want[2] >= 1).all()
            if rho == 0:
                assert not want[2].any()


def test_all_ones_mask_equals_the_unmasked_search(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, lists, ms = shard(bsr_mod, oracle_mod, "768")
    n, nq = len(rows), 50
    radius = kth_radius(lists[:nq], ms[:nq])
    radius[:4] = (-1.0, 2.0, np.inf, 0.0)
    plain = ix.range_search(qs[:nq], radius, max_results=64)
    words = np.full((n + 63) // 64, 2 ** 64 - 1, np.uint64)  # (the bits at positions >= n are ignored)
    for mode in MODES:
        for mask in (np.ones(n, bool), words):
            same(ix.range_search(qs[:nq], radius, max_results=64, allow_mask=mask, mask_mode=mode), plain, mode)
    assert plain[2][1] == n and plain[2][2] == n and plain[2][0] == 0


# ---- 2. groups ------------------------------------------------------------------------------------
def test_groups(bsr_mod, oracle_mod, gpu):
    import torch
    ix, rows, qs, lists, ms = shard(bsr_mod, oracle_mod, "768")
    n, nq, capacity = len(rows), 300, 64
    rng = np.random.default_rng(21)
    rhos = (1, 1 / 2, 1 / 16, 1 / 100, 1 / 1000, 0, 1 / 4)  # mask 5 is empty, mask 6 has no query
    masks = np.stack([rho_mask(rng, n, r) for r in rhos])
    qm = rng.integers(0, 6, nq).astype(np.uint32)
    qm[:6] = np.arange(6)
    allowed = masks[qm]
    lr = restrict(lists, allowed)
    radius = radii_in_mask(lr, lists, ms, False)
    radius[10:13] = (2.0, -1.0, np.inf)
    want = want_for(lists, allowed, radius, capacity, n, OFFSET)
    P = bsr_mod
    paths = {}
    for mode in MODES:
        for qm_arg in (qm, torch.from_numpy(qm.astype(np.int32)).to("cuda:0")):
            got = ix.range_search(qs, radius, max_results=capacity, allow_masks=masks, query_mask=qm_arg, mask_mode=mode)
            st = ix.last_stats()
            same(got, want, ("groups", mode, type(qm_arg).__name__))
            assert st.search_path & P.BSR_PATH_RANGE and st.search_path & P.BSR_PATH_MASK_GROUPS
            assert not (st.search_path & P.BSR_PATH_RANGE_SCAN)
            paths[mode] = st.search_path
            print(f"groups {mode}: emitted={st.n_emitted} direct={st.n_exact_direct} fallback={st.n_fallback} path={st.search_path}")
    assert paths["list"] & P.BSR_PATH_MASK_LIST and not (paths["list"] & P.BSR_PATH_MASK_FILTER)
    assert paths["filter"] & P.BSR_PATH_MASK_FILTER
    # AUTO sends the dense masks' groups to the filter and the sparse ones' to the list
    assert paths["auto"] & P.BSR_PATH_MASK_FILTER and paths["auto"] & P.BSR_PATH_MASK_LIST
    # one call per mask gives the same rows
    for g in range(6):
        sel = np.flatnonzero(qm == g)
        one = ix.range_search(qs[sel], radius[sel], max_results=capacity, allow_mask=masks[g])
        same(one, tuple(x[sel] for x in want), ("one call per mask", g))
    c = want[2]
    assert c[10] == masks[qm[10]].sum() and c[11] == 0 and c[12] == masks[qm[12]].sum()
    assert not c[qm == 5].any()


# ---- 3. the ladder: filter -> list scan -> count only ---------------------------------------------
def test_ladder(bsr_mod, oracle_mod, gpu):
    rng = np.random.default_rng(78)
    n, dim = 9000, 768
    rows = rng.uniform(-1, 1, (n, dim)).astype(F)
    qs = rng.uniform(-1, 1, (5, dim)).astype(F)
    qs[3] = 0.0  # a zero query: every row at distance 1, answered by the list scan
    pos = rng.permutation(n)
    dup, ordinary, rest = pos[:3000], pos[3000:3030], pos[3030:]
    rows[dup] = rows_at_distance(rng, qs[4], rng.uniform(0.001, 0.03, 3000))  # near-duplicates of query 4
    rows[ordinary] = cluster_rows(rng, qs[0], 30)
    mask = np.zeros(n, bool)
    mask[dup[:1500]] = mask[ordinary[::2]] = True
    mask[rest[:3000 - int(mask.sum())]] = True
    assert mask.sum() == 3000
    ix = bsr_mod.Index(dim, max_k=64, device=0).load(rows, global_offset=11)
    lists = sorted_lists(oracle_mod, rows, qs)
    lr = restrict(lists, mask)
    #         filters      radius >= 2  < 0   zero query   its emitted list overflows at 512 slots
    radius = np.array([lr[0][1][9], 2.0, -1.0, 1.0, 0.05], F)
    P = bsr_mod
    for capacity in (512, 4096):
        want = want_for(lists, mask, radius, capacity, n, 11)
        assert list(want[2]) == [10, 3000, 0, 3000, 1500]
        for mode in ("filter", "auto"):
            got = ix.range_search(qs, radius, max_results=capacity, allow_mask=mask, mask_mode=mode)
            st = ix.last_stats()
            print(f"ladder cap={capacity} {mode}: emitted={st.n_emitted} direct={st.n_exact_direct} "
                  f"fallback={st.n_fallback} path={st.search_path}")
            same(got, want, ("ladder", capacity, mode))
            if capacity == 4096:
                # A_g = 3000 fits: the list scan delivers every allowed row, sorted
                assert (got[0][1, :3000] != NONE_IDX).all() and (np.diff(got[1][1, :3000]) >= 0).all()
                assert set((got[0][1, :3000] - np.uint64(11)).tolist()) == set(np.flatnonzero(mask).tolist())
                assert (got[0][4, :1500] != NONE_IDX).all()
            else:
                # A_g > capacity: count only -- exact, with every slot padding
                assert (got[0][1] == NONE_IDX).all() and (got[0][3] == NONE_IDX).all() and (got[0][4] == NONE_IDX).all()
            if mode == "filter":
                assert st.search_path == P.BSR_PATH_RANGE | P.BSR_PATH_MASK_FILTER | P.BSR_PATH_MASK_LIST
                assert st.n_exact_direct == 2, "radius >= 2 and the zero query; radius < 0 is never scanned"
                # 3000 near-duplicates overflow a list of 1024 keys, not one of 8192
                assert st.n_fallback == (1 if capacity == 512 else 0)
    ix.close()


# ---- 4. the row lifecycle -------------------------------------------------------------------------
def test_tombstones_update_compact(bsr_mod, oracle_mod, gpu):
    n, dim, nq, per, cap = 6000, 130, 6, 40, 64
    rows, qs, pos = make_shard(n, dim, nq, per, 4321)
    rng = np.random.default_rng(9)
    ix = bsr_mod.Index(dim, max_k=64, device=0).load(rows, global_offset=1000)
    mask = rng.random(n) < 0.5
    ms = (12, 20, 5, 9, 15, 7)

    def check(ctx, rows, allowed, offset):
        lists = sorted_lists(oracle_mod, rows, qs)
        radius = radii_in_mask(restrict(lists, allowed), lists, ms, False)
        want = want_for(lists, allowed, radius, cap, len(rows), offset)
        for mode in MODES:
            same(ix.range_search(qs, radius, max_results=cap, allow_mask=allowed if mode != "auto" else None,
                                 allow_ids=np.flatnonzero(allowed) if mode == "auto" else None, mask_mode=mode),
                 want, (ctx, mode))
        return radius, want

    check("before any delete", rows, mask, 1000)
    gone = np.concatenate([pos[0][::2], rng.choice(np.setdiff1d(np.arange(n), pos.ravel()), 100, False)])
    assert ix.delete(gone + 1000) == len(gone)
    dead = np.zeros(n, bool)
    dead[gone] = True
    radius, want = check("tombstones", rows, mask & ~dead, 1000)  # (the mask still names the deleted rows)
    for mode in MODES:
        got = ix.range_search(qs, radius, max_results=cap, allow_mask=mask, mask_mode=mode)
        same(got, want, ("the mask names deleted rows", mode))
        assert not np.isin(got[0], gone.astype(np.uint64) + np.uint64(1000)).any()
    # a range search on an index with tombstones = a masked range search with ~deleted_mask() on a fresh copy
    assert np.array_equal(ix.deleted_mask(), dead)
    fresh = bsr_mod.Index(dim, max_k=64, device=0).load(rows, global_offset=1000)
    r2 = np.full(nq, 0.1, F)
    r2[1] = 2.0
    plain = ix.range_search(qs, r2, max_results=cap)
    for mode in MODES:
        same(fresh.range_search(qs, r2, max_results=cap, allow_mask=~ix.deleted_mask(), mask_mode=mode), plain, mode)
    assert plain[2][1] == n - len(gone)
    fresh.close()
    # update: cluster 1 loses ten rows to the background, cluster 2 gains ten from it
    live = np.flatnonzero(~dead)
    ids = np.concatenate([pos[1][:10], rng.choice(np.setdiff1d(live, pos.ravel()), 10, False)])
    new = np.concatenate([rng.uniform(-1, 1, (10, dim)).astype(F), cluster_rows(rng, qs[2], 10)])
    ix.update(ids + 1000, new)
    rows = rows.copy()
    rows[ids] = new
    check("after an update", rows, mask & ~dead, 1000)
    # compaction: the live rows packed, a new offset, the mask re-packed for the new n
    old = ix.compact(global_offset=50_000)
    assert np.array_equal(old, live.astype(np.uint64) + np.uint64(1000))
    check("after a compaction", rows[live], mask[live], 50_000)
    # every row deleted: no live row, every count 0 in every mode
    assert ix.delete(np.arange(len(live)) + 50_000) == len(live)
    for mode in MODES:
        got = ix.range_search(qs, 2.0, max_results=cap, allow_mask=mask[live], mask_mode=mode)
        assert not got[2].any() and (got[0] == NONE_IDX).all() and np.isposinf(got[1]).all(), mode
    ix.close()


def test_exact_only_index(bsr_mod, oracle_mod, gpu):
    rows, qs, pos = make_shard(3000, 130, 17, 30, 99)
    n = len(rows)
    mask = np.random.default_rng(1).random(n) < 0.5
    lists = sorted_lists(oracle_mod, rows, qs)
    radius = radii_in_mask(restrict(lists, mask), lists, [1 + q for q in range(17)], False)
    want = want_for(lists, mask, radius, 64, n, 40)
    P = bsr_mod
    for flags in (0, P.BSR_FLAG_EXACT_ONLY):
        ix = P.Index(130, max_k=64, device=0, flags=flags).load(rows, global_offset=40)
        for mode in MODES:
            got = ix.range_search(qs, radius, max_results=64, allow_mask=mask, mask_mode=mode)
            st = ix.last_stats()
            same(got, want, ("flags", flags, mode))
            if flags:  # every query goes to the list
                assert st.search_path == P.BSR_PATH_RANGE | P.BSR_PATH_MASK_LIST
                assert st.n_exact_direct == 17 and st.n_fallback == 0 and st.n_emitted == 0
        ix.close()


# ---- 5. errors found on the device leave the outputs untouched ------------------------------------
def test_device_errors_write_nothing(bsr_mod, oracle_mod, gpu):
    import torch
    ix, rows, qs, lists, ms = shard(bsr_mod, oracle_mod, "130")
    n, nq, cap = len(rows), 6, 8
    words = bsr_mod.pack_allow_masks(n, masks=np.ones((2, n), bool))
    dev = lambda a: torch.from_numpy(a).to("cuda:0")  # noqa: E731
    q, radius, qm = qs[:nq].copy(), np.full(nq, 0.1, F), np.array([0, 1, 0, 1, 1, 0], np.int32)
    bad_qm, bad_r, bad_q = qm.copy(), radius.copy(), q.copy()
    bad_qm[3] = 2
    bad_r[4] = np.nan
    bad_q[2, 5] = np.inf
    cases = [("query_mask entry >= n_masks", q, radius, words, bad_qm, E_INVALID),
             ("NaN radius", q, bad_r, words, qm, E_INVALID),
             ("non-finite query", bad_q, radius, words, qm, E_NONFINITE),
             ("wrong allow_words", q, radius, words[:, :-1].copy(), qm, E_INVALID)]
    for what, cq, cr, cw, cqm, status in cases:
        for on_dev in (False, True):
            hi, hd, hc = np.full((nq, cap), 9, np.uint64), np.full((nq, cap), 9, F), np.full(nq, 9, np.uint32)
            di = torch.full((nq, cap), 9, dtype=torch.int64, device="cuda:0")
            dd = torch.full((nq, cap), 9.0, dtype=torch.float32, device="cuda:0")
            dc = torch.full((nq,), 9, dtype=torch.int32, device="cuda:0")
            outs = (di, dd, dc) if on_dev else (hi, hd, hc)
            ins = (dev(cq), nq, dev(cr), cap) if on_dev else (cq, nq, cr, cap)
            with pytest.raises(bsr_mod.BsrError) as e:
                ix.range_search_device(*ins, *outs, allow_words=dev(cw.view(np.int64)) if on_dev else cw,
                                       query_mask=dev(cqm) if on_dev else cqm.view(np.uint32), mask_mode="filter")
            assert e.value.status == status, (what, on_dev)
            torch.cuda.synchronize()
            assert bool((di == 9).all()) and bool((dd == 9).all()) and bool((dc == 9).all()), (what, on_dev)
            assert (hi == 9).all() and (hd == 9).all() and (hc == 9).all(), (what, on_dev)
    # and the same arrays without the faults are served
    hi, hd, hc = np.full((nq, cap), 9, np.uint64), np.full((nq, cap), 9, F), np.full(nq, 9, np.uint32)
    ix.range_search_device(q, nq, radius, cap, hi, hd, hc, allow_words=words, query_mask=qm.view(np.uint32))
    same((hi, hd, hc), want_for(lists[:nq], np.ones(n, bool), radius, cap, n, OFFSET), "served")
    assert ix.range_search(qs[:0], np.zeros(0, F), max_results=4, allow_mask=np.ones(n, bool))[2].shape == (0,)


# ---- 6. the list budget, and the plain search afterwards -------------------------------------------
def test_list_budget_splits_a_list_over_chunks(bsr_mod, oracle_mod, gpu, monkeypatch):
    ix, rows, qs, lists, ms = shard(bsr_mod, oracle_mod, "768")
    n, nq, capacity = len(rows), 30, 64
    rng = np.random.default_rng(33)
    masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.05, rng.random(n) < 0.2])
    qm = (np.arange(nq) % 3).astype(np.uint32)
    allowed = masks[qm]
    radius = radii_in_mask(restrict(lists[:nq], allowed), lists[:nq], ms[:nq], False)
    radius[0] = 2.0  # (every row of the long list, through all of its chunks)
    want = want_for(lists[:nq], allowed, radius, capacity, n, OFFSET)
    assert want[2][0] == masks[0].sum() > 9000
    kw = dict(max_results=capacity, allow_masks=masks, query_mask=qm, mask_mode="list")
    same(ix.range_search(qs[:nq], radius, **kw), want, "default budget")
    # 4000 ids a chunk: mask 0's ~10000 rows take three chunks, and share the last with the others
    monkeypatch.setenv("BSR_MASK_LIST_BUDGET", str(4 * 4000))
    same(ix.range_search(qs[:nq], radius, **kw), want, "three chunks")
    monkeypatch.setenv("BSR_MASK_LIST_BUDGET", "4")  # one id a chunk is legal too: a single query, a sparse mask
    one = ix.range_search(qs[1:2], radius[1:2], max_results=capacity, allow_mask=masks[1] & (np.arange(n) % 8 == 0),
                          mask_mode="list")
    same(one, want_for(lists[1:2], masks[1] & (np.arange(n) % 8 == 0), radius[1:2], capacity, n, OFFSET), "one id a chunk")


def test_plain_search_afterwards(bsr_mod, oracle_mod, gpu):
    """Masked range searches between plain searches: the top-k results and their graph replay are untouched."""
    ix, rows, qs, lists, ms = shard(bsr_mod, oracle_mod, "130")
    n, nq, k = len(rows), 20, 10
    gold_i = np.stack([lists[q][0][:k] for q in range(nq)]) + np.uint64(OFFSET)
    gold_d = np.stack([lists[q][1][:k] for q in range(nq)])

    def plain():
        for rep in range(3):
            gi, gd, gc = ix.local_top_k(qs[:nq], k)
            assert np.array_equal(gi, gold_i) and np.array_equal(gd.view(np.uint32), gold_d.view(np.uint32)), rep
            assert (gc == k).all()
        assert ix.last_stats().graph_replay == 1

    plain()
    mask = np.random.default_rng(2).random(n) < 0.25
    radius = radii_in_mask(restrict(lists[:nq], mask), lists[:nq], ms[:nq], False)
    for mode in MODES:
        same(ix.range_search(qs[:nq], radius, max_results=64, allow_mask=mask, mask_mode=mode),
             want_for(lists[:nq], mask, radius, 64, n, OFFSET), mode)
        assert ix.last_stats().graph_replay == 0
    plain()
