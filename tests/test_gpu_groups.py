"""Group search (bsr_local_top_groups) through the C ABI, whole calls, bit for bit.

The model: the oracle's f32 distances of every (query, row) pair (test_gpu_collapse.all_dists), the
deleted and disallowed rows dropped, the rest sorted by (distance, index); the groups in the order
of their first row are the result groups, the first k of them, each with its first m rows.  Indices,
f32 distance bits, rows per group, group ids, counts and the padding are compared exactly.

The shards are test_gpu_collapse's (shared, never modified); row_group is this file's, per call."""
import numpy as np
import pytest

import test_gpu_collapse as tc

pytestmark = pytest.mark.gpu

F = np.float32
OFFSET = tc.OFFSET
NONE_IDX = tc.NONE_IDX
NONE_GRP = np.uint32(0xFFFFFFFF)


def model(dists, rg, k, m, ok=None, offset=OFFSET):
    """ok: None, a bool [n] or one per query.  -> (idx [Q,k,m], dist, rows [Q,k], group [Q,k], count [Q])."""
    nq, n = len(dists), len(rg)
    idx = np.full((nq, k, m), NONE_IDX, np.uint64)
    dist = np.full((nq, k, m), np.inf, F)
    nrows, grp, cnt = np.zeros((nq, k), np.uint32), np.full((nq, k), NONE_GRP, np.uint32), np.zeros(nq, np.uint32)
    for q in range(nq):
        okq = np.ones(n, bool) if ok is None else ok if np.ndim(ok[0]) == 0 else ok[q]
        rows = np.flatnonzero(okq)
        rows = rows[np.lexsort((rows, dists[q][rows]))]
        g = rg[rows]
        ug, first = np.unique(g, return_index=True)
        heads = ug[np.argsort(first)][:k]
        cnt[q] = len(heads)
        for s, h in enumerate(heads):
            mem = rows[g == h][:m]
            idx[q, s, :len(mem)] = mem.astype(np.uint64) + np.uint64(offset)
            dist[q, s, :len(mem)] = dists[q][mem]
            nrows[q, s], grp[q, s] = len(mem), h
    return idx, dist, nrows, grp, cnt


def same(got, want, ctx=""):
    for name, g, w in zip(("idx", "dist", "rows", "group", "count"), got, want):
        if name == "dist":
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (ctx, name, bad[:4], g[tuple(bad[0])], w[tuple(bad[0])])


def layout(name, n, dists=None):
    """row_group [n] u32 with the rows of a group scattered over the shard."""
    rng = np.random.default_rng(5)
    if name == "arange":
        return np.arange(n, dtype=np.uint32)
    if name == "one":
        return np.zeros(n, np.uint32)
    sizes = rng.integers(1, 9, n)
    rg = np.repeat(np.arange(n), sizes)[:n][rng.permutation(n)].astype(np.uint32)
    if name in ("long", "split"):
        # one group of 600 rows (ten items, the last partial) that holds every query's nearest row
        near = dists.argmin(axis=1)
        rest = np.setdiff1d(rng.choice(n, 600, replace=False), near)
        rg[np.concatenate([near, rest[:600 - len(np.unique(near))]])] = rg.max() + 1
    return rg


KM = [(1, 1), (10, 3), (64, 64), (256, 16), (7, 64)]


@pytest.mark.parametrize("k,m", KM)
@pytest.mark.parametrize("lay", ["random", "arange", "one", "long", "split"])
def test_layouts(bsr_mod, oracle_mod, gpu, monkeypatch, lay, k, m):
    ix, rows, qs, _, _, dists = tc.shard(bsr_mod, oracle_mod, "big")
    nq = 40 if k <= 64 else 12
    rg = layout(lay, len(rows), dists)
    if lay == "split":
        monkeypatch.setenv("BSR_GROUPS_SPLIT_ITEMS", "2")
    got = ix.group_search(qs[:nq], k, rg, m, fetch_k=max(k, 64))
    same(got, model(dists[:nq], rg, k, m), (lay, k, m))
    st = ix.last_stats()
    assert st.search_path & bsr_mod.BSR_PATH_GROUPS and not st.search_path & bsr_mod.BSR_PATH_COLLAPSE
    if lay in ("long", "split"):  # the long group comes first everywhere, with min(m, 600) rows
        assert (got[3][:, 0] == rg.max()).all() and (got[2][:, 0] == min(m, 600)).all()


@pytest.mark.parametrize("name,k,m", [("w130", 10, 3), ("w130", 7, 64), ("w1100", 10, 3), ("bf16", 10, 3)])
def test_other_shards(bsr_mod, oracle_mod, gpu, name, k, m):
    """w130: 3000 rows of width 130 (a padded ld, a partial last chunk of the dimension), this file's;
    w1100: rows longer than 1024 floats (the fill reads the query from global memory, not LDS);
    bf16: test_gpu_collapse's, compared on the widened values."""
    if name[0] == "w":
        dim = int(name[1:])
        rng = np.random.default_rng(13)
        rows, qs = rng.uniform(-1, 1, (3000, dim)).astype(F), rng.uniform(-1, 1, (8, dim)).astype(F)
        ix = bsr_mod.Index(dim, max_k=256, device=0)
        ix.load(rows, global_offset=OFFSET)
        dists = tc.all_dists(oracle_mod, rows, qs)
    else:
        ix, rows, qs, _, _, dists = tc.shard(bsr_mod, oracle_mod, name)
    for lay in ("random", "long"):
        rg = layout(lay, len(rows), dists)
        same(ix.group_search(qs, k, rg, m, fetch_k=min(64, max(k, 32))), model(dists, rg, k, m), (name, lay))
    if name[0] == "w":
        ix.close()


def test_fetch_k_and_identities(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, _, _, dists = tc.shard(bsr_mod, oracle_mod, "big")
    n, k = len(rows), 10
    rg = layout("long", n, dists)
    a, b = ix.group_search(qs, k, rg, 3, fetch_k=k), ix.group_search(qs, k, rg, 3, fetch_k=256)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    same(a, model(dists, rg, k, 3), "fetch_k = k")
    ci, cd, cc, cg = ix.collapsed_search(qs, k, rg, fetch_k=64, return_groups=True)
    one = ix.group_search(qs, k, rg, 1, fetch_k=64)
    assert one[0].tobytes() == ci.tobytes() and one[1].tobytes() == cd.tobytes()
    assert one[3].tobytes() == cg.tobytes() and one[4].tobytes() == cc.tobytes()
    assert np.array_equal(a[0][:, :, 0], ci) and np.array_equal(a[1][:, :, 0].view(np.uint32), cd.view(np.uint32))
    ti, td, tn = ix.local_top_k(qs, k)
    g = ix.group_search(qs, k, np.arange(n, dtype=np.uint32), 3, fetch_k=64)
    assert np.array_equal(g[0][:, :, 0], ti) and np.array_equal(g[1][:, :, 0].view(np.uint32), td.view(np.uint32))
    assert (g[2] == 1).all() and np.array_equal(g[4], tn) and (g[0][:, :, 1:] == NONE_IDX).all()


def test_scan_route(bsr_mod, oracle_mod, gpu):
    """test_gpu_collapse's planted queries: their 64 nearest rows are one group of 89 rows."""
    ix, rows, qs, rg, ng, dists = tc.shard(bsr_mod, oracle_mod, "big")
    sel = list(tc.SCAN_Q) + [0]
    for m in (3, 64):
        got = ix.group_search(qs[sel], 10, rg, m, n_groups=ng, fetch_k=64)
        same(got, model(dists[sel], rg, 10, m), m)
        st = ix.last_stats()
        assert st.search_path & bsr_mod.BSR_PATH_GROUPS and st.search_path & bsr_mod.BSR_PATH_COLLAPSE_SCAN
    assert (got[2][:3, 0] == 64).all()


def test_tombstones_masks_and_edges(bsr_mod, oracle_mod, gpu):
    rows, qs, _, _ = tc.make_shard(600, 768, 12, 8, plant=False)
    n, nq, k, m = 600, 12, 5, 4
    rows[5] = rows[6] = rows[7] = rows[300]  # identical rows, tied by index, and a zero row: one group
    rows[8] = 0
    qs[0] = rows[5]
    rg = layout("random", n)
    rg[[5, 6, 7, 8, 300]] = rg.max() + 1
    ix = bsr_mod.Index(768, max_k=64, device=0)
    ix.load(rows, global_offset=OFFSET)
    dists = tc.all_dists(oracle_mod, rows, qs)
    want = model(dists, rg, k, m)
    same(ix.group_search(qs, k, rg, m), want, "ties")
    assert want[0][0, 0].tolist() == [OFFSET + 5, OFFSET + 6, OFFSET + 7, OFFSET + 300] and want[1][0, 0, 0] == 0
    # query 0: the second row of its best group and its whole second group deleted
    live = np.ones(n, bool)
    live[6] = False
    live[rg == want[3][0, 1]] = False
    dead = np.flatnonzero(~live).astype(np.uint64) + np.uint64(OFFSET)
    assert ix.delete(dead) == len(dead)
    same(ix.group_search(qs, k, rg, m), model(dists, rg, k, m, ok=live), "tombstones")
    # two masks in one batch (the first allows half of every larger group), and one that allows nothing
    masks = np.stack([np.arange(n) % 2 == 0, np.ones(n, bool), np.zeros(n, bool)])
    qm = np.arange(nq, dtype=np.uint32) % 3
    got = ix.group_search(qs, k, rg, m, allow_masks=masks, query_mask=qm)
    same(got, model(dists, rg, k, m, ok=[masks[g] & live for g in qm]), "masks")
    assert (got[4][qm == 2] == 0).all() and (got[2][qm == 2] == 0).all() and (got[3][qm == 2] == NONE_GRP).all()
    # no query; an empty shard
    assert [x.shape for x in ix.group_search(qs[:0], k, rg, m)] == [(0, k, m), (0, k, m), (0, k), (0, k), (0,)]
    ix.close()
    ix = bsr_mod.Index(768, max_k=64, device=0)
    ix.load(np.zeros((0, 768), F), global_offset=OFFSET)
    got = ix.group_search(qs, k, np.zeros(0, np.uint32), m, n_groups=1)
    assert (got[4] == 0).all() and (got[0] == NONE_IDX).all() and np.isposinf(got[1]).all() and (got[2] == 0).all()
    ix.close()


@pytest.mark.parametrize("case", ["m=0", "m=65", "km=4097", "k>fetch_k", "group", "len"])
def test_errors_leave_outputs_untouched(bsr_mod, oracle_mod, gpu, case):
    ix, rows, qs, rg, ng, dists = tc.shard(bsr_mod, oracle_mod, "big")
    nq = 4
    k, m, fk = {"m=0": (5, 0, 20), "m=65": (5, 65, 20), "km=4097": (241, 17, 256), "k>fetch_k": (21, 3, 20)}.get(
        case, (5, 3, 20))
    out = [np.full((nq, k, max(m, 1)), 7, np.uint64), np.full((nq, k, max(m, 1)), 7, F), np.full(nq, 7, np.uint32),
           np.full((nq, k), 7, np.uint32), np.full((nq, k), 7, np.uint32)]
    g = rg.copy()
    if case == "group":
        g[len(g) - 1] = ng
    elif case == "len":
        g = g[:-1].copy()
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.group_search_device(np.ascontiguousarray(qs[:nq]), nq, k, m, fk, g, ng, out[0], out[1], out[2],
                               out_group=out[3], out_rows=out[4])
    assert e.value.status == tc.E_INVALID and all((o == 7).all() for o in out), case
    same(ix.group_search(qs[:nq], 5, rg, 3, n_groups=ng), model(dists[:nq], rg, 5, 3), "after the error")
