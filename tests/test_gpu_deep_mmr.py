"""Deep MMR search (bsr_local_top_k_deep_mmr) through the C ABI, whole calls, bit for
bit: the candidates are the reference's top-fetch_k over the allowed live rows (test_gpu_mmr.Cands),
the selection kcheck_mmr.mmr_model.  Every call also holds last_mmr_pairs to the bound of a full
column per pick.

The big shard plants a cluster of 250 near copies and 12 exact copies around each query's nearest
row: the cluster is longer than 256 and fills the head of every candidate list.  The model's cost
sets the cases: 40 queries up to k = 50, 3 at k = 256."""
import numpy as np
import pytest

import test_gpu_mmr as tm
from test_gpu_mmr import OFFSET, Cands, F, differing, same

pytestmark = pytest.mark.gpu

_big = {}


def big(bsr_mod, oracle_mod):
    """(index, rows, queries, the candidate lists of depth 1024) of the clustered 20000 x 768 shard."""
    if not _big:
        n, dim, nq = 20000, 768, 40
        rng = np.random.default_rng(17)
        rows = rng.uniform(-1, 1, (n, dim)).astype(F)
        qs = np.empty((nq, dim), F)
        spots = rng.choice(np.arange(2000, n), (nq, 262), replace=False)
        for q in range(nq):
            r = 100 + 37 * q
            qs[q] = rows[r] + rng.normal(0, 0.3, dim).astype(F)
            rows[spots[q, :250]] = rows[r] + rng.normal(0, 1e-3, (250, dim)).astype(F)
            rows[spots[q, 250:]] = rows[r]
        ix = bsr_mod.Index(dim, max_k=256, device=0)
        ix.load(rows, global_offset=OFFSET)
        _big.update(ix=ix, rows=rows, qs=qs, c=Cands(oracle_mod, rows, np.arange(n), OFFSET, qs, 1024))
    return _big["ix"], _big["rows"], _big["qs"], _big["c"]


def prefix(c, nq, fetch_k):
    """The lists of the first nq queries cut to fetch_k: a prefix of a deeper list is the shallower list."""
    p = object.__new__(Cands)
    p.stored, p.offset = c.stored, c.offset
    p.loc, p.dq = [l[:fetch_k] for l in c.loc[:nq]], [d[:fetch_k] for d in c.dq[:nq]]
    return p


def dense_pairs(c, got):
    return sum(max(int(n) - 1, 0) * len(l) for n, l in zip(got[2], c.loc))


def run(ix, c, qs, k, fetch_k, lam, ctx, want=None, **kw):
    got = ix.deep_mmr_search(qs, k, fetch_k=fetch_k, lambda_mult=lam, return_rank=True, **kw)
    same(got, c.mmr(k, lam) if want is None else want, ctx)
    pairs, dense = ix.last_mmr_pairs(), dense_pairs(c, got)
    print(f"{ctx}: pairs {pairs} of {dense}")
    assert pairs <= dense
    return got


# (a model column over 1024 x 768 rows takes about 10 ms: 40 queries go with k = 10, 3 with the deeper k)
@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("nq,k,fetch_k", [(40, 10, 300), (40, 10, 64), (3, 10, 300), (3, 50, 1000), (3, 256, 1024)])
def test_big_shard(bsr_mod, oracle_mod, gpu, nq, k, fetch_k, lam):
    ix, rows, qs, call = big(bsr_mod, oracle_mod)
    c = prefix(call, nq, fetch_k)
    P = bsr_mod
    want, top = c.mmr(k, lam), c.top_k(k)
    # on the CPU, for this seed: lambda = 0.5 changes every list that reaches past the cluster (some of
    # the lists that lie inside it: a pass-through of the top-k fails either way), lambda = 1 is the top-k
    if lam == 0.5:
        assert differing(want, top) == nq if fetch_k > 262 else differing(want, top) >= 1
    if lam == 1.0:
        same(want, top, "the model at lambda = 1")
    got = run(ix, c, qs[:nq], k, fetch_k, lam, (nq, k, fetch_k, lam), want=want)
    assert (got[3][:, 0] == 0).all(), "pick 0 is the top-1"
    st = ix.last_stats()
    assert st.search_path & P.BSR_PATH_MMR and st.search_path & P.BSR_PATH_DEEP and st.graph_replay == 0
    assert not st.search_path & (P.BSR_PATH_MASK_LIST | P.BSR_PATH_MASK_FILTER) and st.n_queries == nq
    if lam == 1.0:
        same(got[:3], ix.deep_search(qs[:nq], k), "lambda = 1 against deep_search")


@pytest.mark.parametrize("k,fetch_k", [(10, 64), (5, 200)])
def test_equals_mmr_search(bsr_mod, oracle_mod, gpu, k, fetch_k):
    ix, rows, qs, _ = big(bsr_mod, oracle_mod)
    for lam in (0.0, 0.5, 1.0):
        same(ix.deep_mmr_search(qs, k, fetch_k=fetch_k, lambda_mult=lam, return_rank=True),
             ix.mmr_search(qs, k, fetch_k=fetch_k, lambda_mult=lam, return_rank=True), ("mmr_search", lam))


def test_lazy_at_lambda_one(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, call = big(bsr_mod, oracle_mod)
    c = prefix(call, 40, 1024)
    got = ix.deep_mmr_search(qs, 64, fetch_k=1024, lambda_mult=1.0)
    same(got, c.top_k(64)[:3], "lambda = 1, k = 64")
    assert ix.last_mmr_pairs() < dense_pairs(c, got) / 2


@pytest.mark.parametrize("name,k,fetch_k", [("600", 10, 1000), ("bf16", 10, 300)])
def test_other_shards(bsr_mod, oracle_mod, gpu, name, k, fetch_k):
    ix, rows, qs = tm.shard(bsr_mod, name)
    c = Cands(oracle_mod, rows, np.arange(len(rows)), OFFSET, qs, fetch_k)
    for lam in (0.5, 1.0):
        got = run(ix, c, qs, k, fetch_k, lam, (name, lam))
    assert name != "600" or all(len(l) == 600 for l in c.loc)  # (m < fetch_k)


def test_tombstones(bsr_mod, oracle_mod, gpu):
    rows, qs = tm.make_shard(5000, 130, 6, 12)
    ix = bsr_mod.Index(130, max_k=64, device=0)
    ix.load(rows, global_offset=OFFSET)
    dead = np.unique(ix.deep_search(qs, 40)[0][:, ::3]) - np.uint64(OFFSET)
    assert ix.delete(dead + np.uint64(OFFSET)) == len(dead)
    c = Cands(oracle_mod, rows, np.setdiff1d(np.arange(5000), dead.astype(np.int64)), OFFSET, qs, 300)
    run(ix, c, qs, 20, 300, 0.5, "tombstones")
    ix.close()


@pytest.mark.parametrize("mode", ["list", "filter"])
def test_one_mask(bsr_mod, oracle_mod, gpu, mode):
    ix, rows, qs, _ = big(bsr_mod, oracle_mod)
    ids = np.flatnonzero(np.random.default_rng(31).random(len(rows)) < 0.5)
    if "mask" not in _big:
        _big["mask"] = Cands(oracle_mod, rows, ids, OFFSET, qs[:6], 300)
    got = run(ix, _big["mask"], qs[:6], 10, 300, 0.5, mode, allow_ids=ids, mask_mode=mode)
    P, st = bsr_mod, ix.last_stats()
    assert st.search_path & P.BSR_PATH_MMR and st.search_path & P.BSR_PATH_DEEP
    assert st.search_path & (P.BSR_PATH_MASK_LIST if mode == "list" else P.BSR_PATH_MASK_FILTER)
    assert np.isin((got[0] - np.uint64(OFFSET)).astype(np.int64), ids).all()


def test_three_masks(bsr_mod, oracle_mod, gpu):
    ix, rows, qs, _ = big(bsr_mod, oracle_mod)
    n = len(rows)
    rng = np.random.default_rng(32)
    masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.05, np.zeros(n, bool)])
    masks[2, :30] = True
    qm = np.array([0, 1, 2, 0, 1, 2], np.uint32)
    id_lists = [np.flatnonzero(m) for m in masks]
    c = Cands(oracle_mod, rows, [id_lists[g] for g in qm], OFFSET, qs[:6], 300)
    got = run(ix, c, qs[:6], 40, 300, 0.5, "groups", allow_masks=masks, query_mask=qm)
    assert list(got[2]) == [40, 40, 30] * 2


def test_device_buffers_and_errors(bsr_mod, oracle_mod, gpu):
    import torch
    ix, rows, qs, call = big(bsr_mod, oracle_mod)
    nq, k, fetch_k = 8, 10, 300
    want = prefix(call, nq, fetch_k).mmr(k, 0.5)
    dev = torch.device("cuda:0")
    q = torch.from_numpy(qs[:nq]).to(dev)

    def outs(on_dev):
        t = [torch.full((nq, k), 7, dtype=torch.int64), torch.full((nq, k), 7, dtype=torch.float32),
             torch.full((nq,), 7, dtype=torch.int32), torch.full((nq, k), 7, dtype=torch.int32)]
        return [x.to(dev) if on_dev else x for x in t]

    def read(oi, od, oc, orank):
        return (oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32),
                orank.cpu().numpy().view(np.uint32))
    oi, od, oc, orank = outs(True)
    ix.deep_mmr_search_device(q, nq, k, fetch_k, 0.5, oi, od, oc, out_rank=orank)
    same(read(oi, od, oc, orank), want, "device outputs")
    oi, od, oc, orank = outs(True)
    ix.deep_mmr_search_device(q, nq, k, fetch_k, 0.5, oi, od, oc)
    same(read(oi, od, oc, orank)[:3], want[:3], "no rank")
    assert (orank == 7).all()
    hi, _, _, hr = outs(False)
    ix.deep_mmr_search_device(q, nq, k, fetch_k, 0.5, hi, od, oc, out_rank=hr)
    same(read(hi, od, oc, hr), want, "mixed outputs")
    # a non-finite query, and allow_words of the wrong length: the outputs stay as they were
    bad = qs[:nq].copy()
    bad[2, 17] = np.nan
    hi, hd, hc, hr = (x.numpy() for x in outs(False))
    for kw, status in ((dict(), -2), (dict(allow_words=np.zeros(3, np.uint64)), -1)):
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.deep_mmr_search_device(bad if not kw else qs[:nq].copy(), nq, k, fetch_k, 0.5, hi, hd, hc, out_rank=hr, **kw)
        assert e.value.status == status
        assert (hi == 7).all() and (hd == 7).all() and (hc == 7).all() and (hr == 7).all()
