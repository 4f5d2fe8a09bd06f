"""Masked deep capped search (bsr_local_top_k_deep_capped_masked) through the C ABI, on
test_gpu_deep_cap's shards (made once, shared).  Every expected row is kcheck_cap's pure-numpy model of
the capped contract over the oracle's distances, cut to the live rows the query's mask allows; indices,
order, distance bits, groups, counts and padding must be equal -- no tolerance anywhere."""
import numpy as np
import pytest

import kcheck_cap as kp
from test_gpu_deep_cap import E_INVALID, E_NONFINITE, OFFSET, groups, same, shard

pytestmark = pytest.mark.gpu

SHAPES = [(64, 40_000), (130, 50_001)]
NQ = 9  # (with 8 masks: groups of two queries and of one)
# the seed of row_group per (dim, n // G) of the filter-rung case: one at which, by the model, the cap
# drops a row of the batch's top 257 under the mask (found on the CPU; the test asserts it)
SEEDS = {(64, 10): 0, (64, 40): 0, (130, 10): 0, (130, 40): 0}


def masks_of(n, n_masks, rho, seed=11):
    rng = np.random.default_rng(seed)
    return rng.random((n_masks, n)) < rho


def path(bsr_mod, rung, grouped):
    return (bsr_mod.BSR_PATH_DEEP | bsr_mod.BSR_PATH_CAP | rung | (bsr_mod.BSR_PATH_MASK_GROUPS if grouped else 0))


@pytest.mark.parametrize("k", [1, 257, 1000])
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("n_masks", [1, 8])
@pytest.mark.parametrize("dim,n", SHAPES)
def test_list_rung(bsr_mod, oracle_mod, gpu, dim, n, n_masks, m, k):
    ix, rows, qs, dists = shard(bsr_mod, oracle_mod, dim, n)
    G = n // 400  # (about 8 allowed rows a group: the cap drops most of them, few rows can be kept)
    rg, masks = groups(n, G), masks_of(n, n_masks, 1 / 50)
    qmask = np.arange(NQ) % n_masks if n_masks > 1 else None
    allowed = [masks[qmask[q] if n_masks > 1 else 0] for q in range(NQ)]
    want = kp.cap_batch(dists[:NQ], rg, k, m, allowed=allowed, offset=OFFSET)
    kw = dict(allow_masks=masks, query_mask=qmask) if n_masks > 1 else dict(allow_mask=masks[0])
    same(ix.deep_capped_search(qs[:NQ], k, rg, m, n_groups=G, return_groups=True, mask_mode="list", **kw), want)
    st = ix.last_stats()
    assert st.search_path == path(bsr_mod, bsr_mod.BSR_PATH_MASK_LIST, n_masks > 1)
    assert st.n_exact_direct == NQ and st.n_fallback == 0 and st.n_emitted == 0
    if k == 1000:
        assert (want[2] < k).all()  # (fewer keepable rows than k)


def test_chunks_and_carry(bsr_mod, oracle_mod, gpu, monkeypatch):
    """A list of about 2500 rows split over three chunks by the budget, a second mask sharing the last."""
    monkeypatch.setenv("BSR_MASK_LIST_BUDGET", str(4 * 900))
    ix, rows, qs, dists = shard(bsr_mod, oracle_mod, 64, 40_000)
    n, k, m, G = len(rows), 1000, 3, 400
    rg = groups(n, G)
    masks = np.stack([masks_of(n, 1, 1 / 16)[0], masks_of(n, 1, 1 / 100, seed=12)[0]])
    qmask = np.array([0, 1, 0, 0, 1, 0, 0, 0, 1])
    want = kp.cap_batch(dists[:NQ], rg, k, m, allowed=[masks[g] for g in qmask], offset=OFFSET)
    same(ix.deep_capped_search(qs[:NQ], k, rg, m, n_groups=G, return_groups=True, allow_masks=masks, query_mask=qmask,
                               mask_mode="list"), want)
    assert ix.last_stats().search_path == path(bsr_mod, bsr_mod.BSR_PATH_MASK_LIST, True)


@pytest.mark.parametrize("gdiv,m", [(10, 1), (40, 3)])
@pytest.mark.parametrize("dim,n", SHAPES)
def test_filter_rung(bsr_mod, oracle_mod, gpu, dim, n, gdiv, m):
    nq, k = 40, 257
    ix, rows, qs, dists = shard(bsr_mod, oracle_mod, dim, n)
    G = n // gdiv
    rg, mask = groups(n, G, SEEDS[(dim, gdiv)]), masks_of(n, 1, 1 / 2)[0]
    want = kp.cap_batch(dists, rg, k, m, allowed=mask, offset=OFFSET)
    # the inputs do what the case is about, by the model alone: the cap drops a row, and the k-th kept
    # row lies within the first 1.5 k allowed rows of the plain order
    plain = kp.cap_batch(dists, np.arange(n), k, 1, allowed=mask, offset=OFFSET)
    assert not np.array_equal(want[0], plain[0])
    for q in range(nq):
        d, i = want[1][q, k - 1], int(want[0][q, k - 1]) - OFFSET
        ahead = (dists[q] < d) | ((dists[q] == d) & (np.arange(n) <= i))
        assert np.count_nonzero(ahead & mask) <= 1.5 * k
    same(ix.deep_capped_search(qs, k, rg, m, n_groups=G, return_groups=True, allow_mask=mask, mask_mode="filter"), want)
    st = ix.last_stats()
    print(f"emitted/query={st.n_emitted / nq:.0f} fallback={st.n_fallback} direct={st.n_exact_direct}")
    assert st.search_path & ~bsr_mod.BSR_PATH_MASK_LIST == path(bsr_mod, bsr_mod.BSR_PATH_MASK_FILTER, False)
    assert st.n_fallback + st.n_exact_direct <= nq / 10  # (the list scan must not hide a rung that never certifies)


def test_identities(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, dists = shard(bsr_mod, oracle_mod, 64, 40_000)
    n, G = len(rows), 1000
    rg, qs = groups(n, G), qs[:NQ]
    ones, mask = np.ones(n, bool), masks_of(n, 1, 1 / 20)[0]

    def run(k, row_group=rg, n_groups=G, m=3, allow=mask):
        return ix.deep_capped_search(qs, k, row_group, m, n_groups=n_groups, return_groups=True, allow_mask=allow)

    for a, b in zip(run(1000, allow=ones), ix.deep_capped_search(qs, 1000, rg, 3, n_groups=G, return_groups=True)):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(run(1000, np.arange(n), n, 7), ix.deep_search(qs, 1000, allow_mask=mask)):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(run(200), ix.capped_search(qs, 200, rg, 3, n_groups=G, fetch_k=256, allow_mask=mask,
                                               return_groups=True)):
        assert a.tobytes() == b.tobytes()
    deep, shallow = run(1000), run(257)
    assert all(np.array_equal(deep[j][:, :257], shallow[j]) for j in (0, 1, 3))


@pytest.mark.parametrize("where", ["host", "device", "mixed"])
@pytest.mark.parametrize("dtype", ["BSR_F32", "BSR_BF16"])
def test_deleted_rows_and_pointers(bsr_mod, oracle_mod, gpu, dtype, where):
    import torch
    n, nq, k, m, G = 40_000, 6, 1000, 3, 300
    ix, rows, qs, dists = shard(bsr_mod, oracle_mod, 64, n, nq=nq, dtype=getattr(bsr_mod, dtype), tag="masked")
    rg, masks = groups(n, G), masks_of(n, 2, 1 / 30)
    qmask = np.array([0, 1, 1, 0, 0, 1], np.int32)
    allowed = [masks[g] for g in qmask]
    heads = kp.cap_batch(dists[:1], rg, 40, 1, allowed=allowed[0])[0][0].astype(np.int64)  # query 0's 40 best groups' heads
    gone = np.union1d(heads[::2], np.flatnonzero(np.random.default_rng(5).random(n) < 0.05))
    ix.delete(gone + OFFSET)  # (the later runs of the set delete nothing new)
    live = np.ones(n, bool)
    live[gone] = False
    want = kp.cap_batch(dists, rg, k, m, live=live, allowed=allowed, offset=OFFSET)
    dev = torch.device("cuda:0")
    on = {"host": (None, None), "device": (dev, dev), "mixed": (dev, None)}[where]  # (inputs, outputs)
    words = torch.from_numpy(bsr_mod.pack_allow_masks(n, masks=masks).view(np.int64)).to(on[0])
    oi, od, og = (torch.zeros((nq, k), dtype=t, device=on[1]) for t in (torch.int64, torch.float32, torch.int32))
    oc = torch.zeros(nq, dtype=torch.int32, device=on[1])
    ix.deep_capped_search_device(torch.from_numpy(qs).to(on[1]), nq, k, m, torch.from_numpy(rg.view(np.int32)).to(on[0]),
                                 G, oi, od, oc, out_group=og, allow_words=words,
                                 query_mask=torch.from_numpy(qmask).to(on[0]), mask_mode="list")
    torch.cuda.synchronize()
    same((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32),
          og.cpu().numpy().view(np.uint32)), want)


@pytest.mark.parametrize("case", ["bad_group", "bad_query_mask", "nan_query", "allow_words", "short_row_group", "no_rows"])
def test_errors_leave_outputs_untouched(bsr_mod, oracle_mod, gpu, case):
    import torch
    ix, rows, qs, dists = shard(bsr_mod, oracle_mod, 64, 40_000)
    n, nq, k, G = len(rows), 4, 300, 1000
    rg, q, status = groups(n, G), qs[:nq].copy(), E_INVALID
    masks = masks_of(n, 2, 0.0 if case == "no_rows" else 1 / 50)
    words = bsr_mod.pack_allow_masks(n, masks=masks)
    qmask = np.array([0, 1, 2 if case == "bad_query_mask" else 1, 0], np.uint32)
    if case == "bad_group":
        rg[n - 1] = G
    elif case == "nan_query":
        q[2, 7], status = np.nan, E_NONFINITE
    elif case == "allow_words":
        words = np.ascontiguousarray(words[:, :-1])
    elif case == "short_row_group":
        rg = rg[:-1].copy()
    for dev in (None, torch.device("cuda:0")):
        outs = [torch.full((nq, k), 7, dtype=t, device=dev) for t in (torch.int64, torch.float32, torch.int32)]
        outs.insert(2, torch.full((nq,), 7, dtype=torch.int32, device=dev))
        args = (q, nq, k, 3, rg, G, outs[0], outs[1], outs[2])
        if case == "no_rows":  # (masks that allow nothing: every count 0, every slot padding, no error)
            ix.deep_capped_search_device(*args, out_group=outs[3], allow_words=words, query_mask=qmask)
            torch.cuda.synchronize()
            assert bool((outs[2] == 0).all() and (outs[0] == -1).all() and torch.isposinf(outs[1]).all()
                        and (outs[3] == -1).all())
            continue
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.deep_capped_search_device(*args, out_group=outs[3], allow_words=words, query_mask=qmask)
        assert e.value.status == status
        torch.cuda.synchronize()
        assert all(bool((o == 7).all()) for o in outs)
