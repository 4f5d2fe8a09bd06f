"""Deep group search (bsr_local_top_groups_deep) through the C ABI, whole calls, bit
for bit against test_gpu_groups.model over the oracle distances of test_gpu_collapse's shards (shared,
never modified); row_group is test_gpu_groups.layout's, per call."""
import numpy as np
import pytest

import test_gpu_collapse as tc
import test_gpu_groups as tg

pytestmark = pytest.mark.gpu

F = np.float32
OFFSET = tc.OFFSET
# the first k the shallow call refuses (both table builds at it), the slot limit from both sides, m = 64
KM = [(257, 1), (257, 3), (1024, 8), (128, 64), (1000, 2)]


def path_ok(bsr_mod, st, masks=False):
    p, B = st.search_path, bsr_mod
    never = B.BSR_PATH_CAP | B.BSR_PATH_COLLAPSE | B.BSR_PATH_DEEP_SCAN | B.BSR_PATH_COLLAPSE_SCAN
    want = B.BSR_PATH_DEEP | B.BSR_PATH_GROUPS
    return p & want == want and not p & never and bool(p & (B.BSR_PATH_MASK_LIST | B.BSR_PATH_MASK_FILTER)) == masks


@pytest.mark.parametrize("k,m", KM)
@pytest.mark.parametrize("lay", ["random", "arange", "one", "long", "long-split"])
def test_layouts(bsr_mod, oracle_mod, gpu, monkeypatch, lay, k, m):
    """"one" is a single group of 20000 rows (313 items: above the budget, the split launch and the
    finish run); "long-split" lowers the budget below the 600-row group of a 2-query batch."""
    ix, rows, qs, _, _, dists = tc.shard(bsr_mod, oracle_mod, "big")
    nq = 2 if lay == "long-split" else 12 if k >= 1000 else 40
    rg = tg.layout(lay.split("-")[0], len(rows), dists)
    if lay == "long-split":
        monkeypatch.setenv("BSR_GROUPS_SPLIT_ITEMS", "2")
    got = ix.deep_group_search(qs[:nq], k, rg, m)
    tg.same(got, tg.model(dists[:nq], rg, k, m), (lay, k, m))
    assert path_ok(bsr_mod, ix.last_stats())
    if lay == "one":
        assert (got[4] == 1).all() and ix.last_stats().search_path & bsr_mod.BSR_PATH_CAP_SCAN
    if lay.startswith("long"):  # the long group comes first everywhere, with min(m, 600) rows
        assert (got[3][:, 0] == rg.max()).all() and (got[2][:, 0] == min(m, 600)).all()


def test_identities(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, _, _, dists = tc.shard(bsr_mod, oracle_mod, "big")
    n, nq = len(rows), 12
    rg = tg.layout("long", n, dists)
    # group_size = 1 is the deep collapsed search; slot [g][0] is its head for every group_size
    ci, cd, cc, cg = ix.deep_capped_search(qs[:nq], 1000, rg, per_group=1, return_groups=True)
    one = ix.deep_group_search(qs[:nq], 1000, rg, 1)
    assert one[0].tobytes() == ci.tobytes() and one[1].tobytes() == cd.tobytes()
    assert one[3].tobytes() == cg.tobytes() and one[4].tobytes() == cc.tobytes()
    deep = ix.deep_group_search(qs[:nq], 1000, rg, 3)
    assert np.array_equal(deep[0][:, :, 0], ci) and np.array_equal(deep[1][:, :, 0].view(np.uint32), cd.view(np.uint32))
    # k <= 256: the shallow call's five outputs, byte for byte; the result at k is a prefix in k
    a, b = ix.deep_group_search(qs[:nq], 200, rg, 3), ix.group_search(qs[:nq], 200, rg, 3, fetch_k=256)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert all(np.array_equal(x, y[:, :200]) for x, y in zip(a[:4], deep[:4]))
    # row_group[i] = i: the deep search in the [g][0] slots
    ti, td, tn = ix.deep_search(qs[:nq], 300)
    g = ix.deep_group_search(qs[:nq], 300, np.arange(n, dtype=np.uint32), 3)
    assert np.array_equal(g[0][:, :, 0], ti) and np.array_equal(g[1][:, :, 0].view(np.uint32), td.view(np.uint32))
    assert (g[2] == 1).all() and np.array_equal(g[4], tn) and (g[0][:, :, 1:] == tg.NONE_IDX).all()


def test_tombstones_and_masks(bsr_mod, oracle_mod, gpu):
    """A shard of its own (it deletes): 3000 rows, k above the 256 of the shallow call; then two masks in
    one batch, one of them empty, over the tombstones."""
    rows, qs, _, _ = tc.make_shard(3000, 768, 12, 8, plant=False)
    n, nq, k, m = 3000, 12, 300, 4
    dists = tc.all_dists(oracle_mod, rows, qs)
    rg = tg.layout("long", n, dists)
    ix = bsr_mod.Index(768, max_k=64, device=0)
    ix.load(rows, global_offset=OFFSET)
    want = tg.model(dists, rg, k, m)
    live = np.ones(n, bool)
    live[int(want[0][0, 0, 1]) - OFFSET] = False  # query 0: the second row of its best group
    live[rg == want[3][0, 1]] = False             # ... and its whole second group
    dead = np.flatnonzero(~live).astype(np.uint64) + np.uint64(OFFSET)
    assert ix.delete(dead) == len(dead)
    tg.same(ix.deep_group_search(qs, k, rg, m), tg.model(dists, rg, k, m, ok=live), "tombstones")
    masks = np.stack([np.arange(n) % 2 == 0, np.zeros(n, bool)])
    qm = np.arange(nq, dtype=np.uint32) % 2
    got = ix.deep_group_search(qs, k, rg, m, allow_masks=masks, query_mask=qm)
    tg.same(got, tg.model(dists, rg, k, m, ok=[masks[g] & live for g in qm]), "masks")
    assert (got[4][qm == 1] == 0).all() and (got[2][qm == 1] == 0).all() and (got[3][qm == 1] == tg.NONE_GRP).all()
    assert path_ok(bsr_mod, ix.last_stats(), masks=True) and ix.last_stats().search_path & bsr_mod.BSR_PATH_MASK_GROUPS
    ix.close()
    ix = bsr_mod.Index(768, max_k=64, device=0)  # an empty shard: every count 0, every slot padded
    ix.load(np.zeros((0, 768), F), global_offset=OFFSET)
    got = ix.deep_group_search(qs, k, np.zeros(0, np.uint32), m, n_groups=1)
    assert (got[4] == 0).all() and (got[0] == tg.NONE_IDX).all() and np.isposinf(got[1]).all() and (got[2] == 0).all()
    ix.close()


@pytest.mark.parametrize("name", ["w130", "bf16"])
def test_other_shards(bsr_mod, oracle_mod, gpu, name):
    """w130: 3000 rows of width 130 (a padded ld, a partial last chunk of the dimension), as
    test_gpu_groups makes it; bf16: test_gpu_collapse's, compared on the widened values."""
    if name == "w130":
        rng = np.random.default_rng(13)
        rows, qs = rng.uniform(-1, 1, (3000, 130)).astype(F), rng.uniform(-1, 1, (8, 130)).astype(F)
        ix = bsr_mod.Index(130, max_k=256, device=0)
        ix.load(rows, global_offset=OFFSET)
        dists = tc.all_dists(oracle_mod, rows, qs)
    else:
        ix, rows, qs, _, _, dists = tc.shard(bsr_mod, oracle_mod, name)
    rg = tg.layout("long", len(rows), dists)
    tg.same(ix.deep_group_search(qs, 300, rg, 3), tg.model(dists, rg, 300, 3), name)
    if name == "w130":
        ix.close()


def test_device_outputs_and_bad_group(bsr_mod, oracle_mod, gpu):
    import torch
    ix, rows, qs, _, _, dists = tc.shard(bsr_mod, oracle_mod, "big")
    nq, k, m = 8, 300, 3
    rg = tg.layout("long", len(rows), dists)
    ng = int(rg.max()) + 1
    dev = torch.device("cuda:0")
    shapes = [((nq, k, m), torch.int64), ((nq, k, m), torch.float32), ((nq,), torch.int32), ((nq, k), torch.int32),
              ((nq, k), torch.int32)]
    out = [torch.full(s, 7, dtype=t, device=dev) for s, t in shapes]
    q, rg_dev = torch.from_numpy(qs[:nq]).to(dev), torch.from_numpy(rg.view(np.int32)).to(dev)
    ix.deep_group_search_device(q, nq, k, m, rg_dev, ng, out[0], out[1], out[2], out_group=out[3], out_rows=out[4])
    oi, od, oc, og, orows = [o.cpu().numpy() for o in out]
    got = (oi.view(np.uint64), od, orows.view(np.uint32), og.view(np.uint32), oc.view(np.uint32))
    tg.same(got, tg.model(dists[:nq], rg, k, m), "device outputs")
    # a row_group entry >= n_groups: BSR_E_INVALID, host and device arrays untouched
    bad = rg.copy()
    bad[-1] = ng
    host = [np.full(s, 7, np.dtype(str(t).split(".")[1])) for s, t in shapes]
    for o, g in ((host, bad), ([torch.full(s, 7, dtype=t, device=dev) for s, t in shapes],
                               torch.from_numpy(bad.view(np.int32)).to(dev))):
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.deep_group_search_device(q, nq, k, m, g, ng, o[0], o[1], o[2], out_group=o[3], out_rows=o[4])
        assert e.value.status == tc.E_INVALID and all(bool((x == 7).all()) for x in o)
