"""The wide device merge (k_merge_wide): bsr_global_top_k and bsr_global_top_k_capped
with every array in device memory, beyond k_merge_lists' limits, against the host merge of the same
arrays (merge.cpp).  Indices, f32 distance bits, groups, counts and padding must be equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_INVALID, E_NONFINITE = -1, -2


def lists(seed, P, Q, k_in, sorted_=True, overlap=True, full=True):
    """idx / dist / group [P,Q,k_in], count [P,Q]: tied distances with both zeros among them, indices
    in a shared range (overlap) or one range per list, groups just below 2^32 - 1 (a function of the index)."""
    rng = np.random.default_rng(seed)
    ld = rng.choice(np.linspace(0, 1, 997, dtype=np.float32), (P, Q, k_in))
    z = rng.random((P, Q, k_in)) < 0.1
    ld[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    if sorted_:
        ld = np.sort(ld, axis=2)
    span = max(P * k_in // 3, 2) if overlap else 1 << 33
    li = rng.integers(0, span, (P, Q, k_in)).astype(np.uint64)
    if not overlap:
        li += np.arange(P, dtype=np.uint64)[:, None, None] << np.uint64(33)
    lg = (np.uint64(2 ** 32 - 2) - li % np.uint64(37)).astype(np.uint32)
    lc = np.full((P, Q), k_in, np.uint32)
    if not full:
        lc = rng.integers(0, k_in + 1, (P, Q)).astype(np.uint32)
        lc[rng.random((P, Q)) < 0.2] = 0
        lc[rng.random((P, Q)) < 0.2] = k_in + 7  # (read as k_in)
        lc[:, 0] = 0                             # every list of query 0 empty
    return li, ld, lg, lc


def merged(bsr_mod, li, ld, lc, k, lg=None, per_group=0, groups=True):
    """(device result, host result) of one merge, each (idx, dist bits, count[, group])."""
    import torch
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()  # noqa: E731
    Q = li.shape[1]
    oi = torch.full((Q, k), 7, dtype=torch.int64, device="cuda")
    od = torch.full((Q, k), 7, dtype=torch.float32, device="cuda")
    og = torch.full((Q, k), 7, dtype=torch.int32, device="cuda")
    oc = torch.full((Q,), 7, dtype=torch.int32, device="cuda")
    if lg is None:
        bsr_mod.merge_top_k_lists_device(dev(li, np.int64), dev(ld, np.float32), dev(lc, np.int32), k, oi, od, oc)
        hi, hd, hc = bsr_mod.merge_top_k_lists(li, ld, lc, k)
        host = (hi, hd.view(np.uint32), hc)
    else:
        bsr_mod.merge_top_k_lists_capped_device(dev(li, np.int64), dev(ld, np.float32), dev(lg, np.int32),
                                                dev(lc, np.int32), k, per_group, oi, od, og if groups else None, oc)
        hi, hd, hg, hc = bsr_mod.merge_top_k_lists_capped(li, ld, lg, lc, k, per_group)
        host = (hi, hd.view(np.uint32), hc, hg if groups else np.full((Q, k), 7, np.uint32))
    got = (oi.cpu().numpy().view(np.uint64), od.cpu().numpy().view(np.uint32), oc.cpu().numpy().view(np.uint32))
    return got + ((og.cpu().numpy().view(np.uint32),) if lg is not None else ()), host


def same(pair):
    got, host = pair
    for g, h, what in zip(got, host, ("indices", "distance bits", "counts", "groups")):
        assert np.array_equal(g, h), what
    return got


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("sorted_", [True, False])
@pytest.mark.parametrize("P,k_in,k,Q", [(5, 205, 10, 5), (2, 200, 257, 5), (2, 1024, 1024, 3), (3, 683, 700, 3),
                                        (64, 1024, 1024, 3)])
def test_plain_shapes(bsr_mod, gpu, P, k_in, k, Q, sorted_, overlap):
    li, ld, _, lc = lists(P * k_in + k, P, Q, k_in, sorted_, overlap)
    same(merged(bsr_mod, li, ld, lc, k))


def test_plain_identical_copies(bsr_mod, gpu):
    """8 copies of one 300-entry list: the k = 300 distinct rows lie in several windows."""
    li, ld, _, lc = lists(3, 1, 2, 300, overlap=False)
    got = same(merged(bsr_mod, np.repeat(li, 8, 0), np.repeat(ld, 8, 0), np.repeat(lc, 8, 0), 300))
    assert [int(c) for c in got[2]] == [len(np.unique(li[0, q])) for q in range(2)]


@pytest.mark.parametrize("overlap", [False, True])
def test_plain_equal_distances(bsr_mod, gpu, overlap):
    li, ld, _, lc = lists(4, 4, 3, 600, overlap=overlap)
    ld[:] = np.float32(0.25)
    same(merged(bsr_mod, li, ld, lc, 500))


@pytest.mark.parametrize("P,k_in,k", [(5, 205, 10), (3, 683, 700)])
def test_plain_ragged_counts(bsr_mod, gpu, P, k_in, k):
    li, ld, _, lc = lists(5, P, 9, k_in, sorted_=False, full=False)
    got = same(merged(bsr_mod, li, ld, lc, k))
    assert got[2][0] == 0 and (got[0][0] == np.uint64(2 ** 64 - 1)).all()


@pytest.mark.parametrize("one_group", [False, True])
@pytest.mark.parametrize("per_group", [1, 2, 150])
@pytest.mark.parametrize("P,k_in", [(8, 300), (3, 683)])
def test_capped(bsr_mod, gpu, P, k_in, per_group, one_group):
    li, ld, lg, lc = lists(P + per_group, P, 4, k_in, sorted_=False, full=P == 8)
    if one_group:
        lg[:] = np.uint32(2 ** 32 - 2)
    got = same(merged(bsr_mod, li, ld, lc, 150, lg, per_group))
    if one_group:
        assert (got[2] == np.minimum(per_group, lc.clip(0, k_in).sum(0))).all()


def test_capped_without_out_group(bsr_mod, gpu):
    li, ld, lg, lc = lists(6, 8, 4, 300)
    same(merged(bsr_mod, li, ld, lc, 150, lg, 2, groups=False))  # (the group tensor stays as it was)


def test_errors(bsr_mod, gpu):
    li, ld, lg, lc = lists(7, 3, 6, 683)
    ld[1, 4, 17] = ld[2, 2, 600] = np.nan
    for grp in (None, lg):
        with pytest.raises(bsr_mod.BsrError) as e:
            merged(bsr_mod, li, ld, lc, 700, grp, 2)
        assert e.value.status == E_NONFINITE and "query 2" in str(e.value)
    import torch
    z = lambda *s, t=torch.int64: torch.zeros(s, dtype=t, device="cuda")  # noqa: E731
    for P, k_in, k in ((2, 2, 1025), (2, 1025, 2), (65, 2, 257)):
        i, d, g, c = z(P, 1, k_in), z(P, 1, k_in, t=torch.float32), z(P, 1, k_in, t=torch.int32), z(P, 1, t=torch.int32)
        oi, od, oc = z(1, k), z(1, k, t=torch.float32), z(1, t=torch.int32)
        for call in (lambda: bsr_mod.merge_top_k_lists_device(i, d, c, k, oi, od, oc),
                     lambda: bsr_mod.merge_top_k_lists_capped_device(i, d, g, c, k, 1, oi, od, None, oc)):
            with pytest.raises(bsr_mod.BsrError) as e:
                call()
            assert e.value.status == E_INVALID and "1024" in str(e.value)
    with pytest.raises(bsr_mod.BsrError) as e:  # mixed memory: a host out_idx
        bsr_mod.merge_top_k_lists_capped_device(z(2, 1, 3), z(2, 1, 3, t=torch.float32), z(2, 1, 3, t=torch.int32),
                                                z(2, 1, t=torch.int32), 2, 1, np.zeros((1, 2), np.uint64),
                                                z(1, 2, t=torch.float32), None, z(1, t=torch.int32))
    assert e.value.status == E_INVALID


def test_three_shards_end_to_end(bsr_mod, oracle_mod, gpu):
    """Deep and capped searches of 3 shards with device outputs, stacked and merged on the device."""
    import torch
    rng = np.random.default_rng(8)
    n, dim, nq, P = 3000, 24, 5, 3
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    rows[1000:1010] = rows[990:1000]  # the same rows on both sides of a shard border
    rows[2000] = rows[999]
    qs = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
    qs[0] = rows[995]
    rg = rng.integers(0, 40, n).astype(np.uint32)
    q = torch.from_numpy(qs).cuda()
    out = lambda k, t: torch.zeros((P, nq, k), dtype=t, device="cuda")  # noqa: E731
    di, dd, dc = out(300, torch.int64), out(300, torch.float32), torch.zeros((P, nq), dtype=torch.int32, device="cuda")
    ci, cd, cg, cc = out(20, torch.int64), out(20, torch.float32), out(20, torch.int32), torch.zeros_like(dc)
    for r in range(P):
        iv = bsr_mod.interval_by_rank(r, P, n)
        ix = bsr_mod.Index(dim, max_k=256, device=0)
        ix.load(rows[iv.start_index:iv.end_index], global_offset=iv.start_index)
        ix.deep_search_device(q, nq, 300, di[r], dd[r], dc[r])
        ix.capped_search_device(q, nq, 20, 64, 2, rg[iv.start_index:iv.end_index].copy(), 40, ci[r], cd[r], cc[r],
                                out_group=cg[r])
        ix.close()
    oi, od, oc = out(300, torch.int64)[0], out(300, torch.float32)[0], dc[0].clone()
    bsr_mod.merge_top_k_lists_device(di, dd, dc, 300, oi, od, oc)
    wi, wd, wc = oracle_mod.parallel_top_k(rows, qs, 300, size=P, threads=4)
    assert np.array_equal(oc.cpu().numpy().view(np.uint32), wc) and (wc == 300).all()
    assert np.array_equal(oi.cpu().numpy().view(np.uint64), wi)
    assert np.array_equal(od.cpu().numpy().view(np.uint32), wd.view(np.uint32))
    host = lambda t, v: t.cpu().numpy().view(v)  # noqa: E731
    same(merged(bsr_mod, host(ci, np.uint64), host(cd, np.float32), host(cc, np.uint32), 20,
                host(cg, np.uint32), 2))
