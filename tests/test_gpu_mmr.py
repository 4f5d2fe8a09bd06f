"""MMR search (bsr_local_top_k_mmr) through the C ABI, whole calls, bit for bit.

The model: the candidates are the reference's own top-fetch_k (oracle.parallel_top_k) over the allowed
live rows, mapped through their ids; the selection is kcheck_mmr.mmr_model on the stored rows of those
candidates.  Counts, global indices, selection order, f32 distance bits and candidate positions, with
the (~0, +inf, ~0u) tail.

The big shard plants, for each query, a cluster around its nearest row: six near copies (noise 1e-3)
and two exact copies.  The plain top-10 of such a query is the cluster; at lambda = 0.5 MMR keeps one of
it.  Checked on the CPU with the model for this seed (8 queries, k = 10, fetch_k = 64): every query's
list differs from the top-k at lambda = 0.5 and at 0, 4 of 8 at 0.7, and none at 1; the same holds for
all 40 queries and for the other (k, fetch_k) pairs used below."""
import numpy as np
import pytest

import kcheck_mmr as km

pytestmark = pytest.mark.gpu

F = np.float32
THREADS = 8
E_NONFINITE = -2
NONE_IDX = np.uint64(0xFFFFFFFFFFFFFFFF)
OFFSET = 5_000_000_000


def make_shard(n, dim, nq, seed, plant=True):
    """U(-1, 1) rows and queries; query q is a noisy copy (0.3) of row 100 + 37 q, so that row is its
    nearest; with plant, six near copies (noise 1e-3) and two exact copies of that row elsewhere."""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-1, 1, (n, dim)).astype(F)
    qs = rng.uniform(-1, 1, (nq, dim)).astype(F)
    if plant:
        spots = rng.choice(np.arange(2000, n), (nq, 8), replace=False)
        for q in range(nq):
            r = 100 + 37 * q
            qs[q] = rows[r] + rng.normal(0, 0.3, dim).astype(F)
            for j in range(6):
                rows[spots[q, j]] = rows[r] + rng.normal(0, 1e-3, dim).astype(F)
            rows[spots[q, 6]] = rows[r]
            rows[spots[q, 7]] = rows[r]
    return rows, qs


class Cands:
    """The reference's candidate lists of a batch over the rows `ids` (ascending local ids, one array
    for the batch or one per query), and the model's MMR outputs from them."""

    def __init__(self, oracle_mod, stored, ids, offset, qs, fetch_k):
        self.stored, self.offset = stored, offset
        nq = len(qs)
        per_query = isinstance(ids, list)
        self.loc, self.dq = [None] * nq, [None] * nq
        groups = {}
        for q in range(nq):
            key = id(ids[q]) if per_query else 0
            groups.setdefault(key, (ids[q] if per_query else ids, []))[1].append(q)
        for sub_ids, members in groups.values():
            sub_ids = np.asarray(sub_ids, np.int64)
            if len(sub_ids) == 0:
                for q in members:
                    self.loc[q], self.dq[q] = np.zeros(0, np.int64), np.zeros(0, F)
                continue
            wi, wd, wc = oracle_mod.parallel_top_k(np.ascontiguousarray(stored[sub_ids]),
                                                   np.ascontiguousarray(qs[members]), fetch_k, size=THREADS,
                                                   threads=THREADS)
            for j, q in enumerate(members):
                c = int(wc[j])
                self.loc[q] = sub_ids[wi[j, :c].astype(np.int64)]
                self.dq[q] = wd[j, :c].copy()

    def top_k(self, k):
        """The plain search's result rows: the first k candidates."""
        return self._rows([list(range(min(k, len(l)))) for l in self.loc], k)

    def mmr(self, k, lam):
        return self._rows([km.mmr_model(self.stored[l], d, k, lam)[0] for l, d in zip(self.loc, self.dq)], k)

    def _rows(self, picks, k):
        nq = len(picks)
        idx, dist = np.empty((nq, k), np.uint64), np.empty((nq, k), F)
        rank, cnt = np.empty((nq, k), np.uint32), np.empty(nq, np.uint32)
        for q in range(nq):
            gids = (self.loc[q] + self.offset).astype(np.uint64)
            idx[q], dist[q], rank[q], cnt[q] = km.mmr_outputs(picks[q], gids, self.dq[q], k)
        return idx, dist, cnt, rank


def same(got, want, ctx=""):
    assert np.array_equal(got[2], want[2]), (ctx, "counts", got[2], want[2])
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1))
    assert bad.size == 0, (ctx, "indices", bad[:8], got[0][bad[0]], want[0][bad[0]])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (ctx, "distance bits")
    if len(got) > 3 and got[3] is not None:
        assert np.array_equal(got[3], want[3]), (ctx, "ranks")


def differing(a, b):
    return int((a[0] != b[0]).any(axis=1).sum())


_shards = {}


def shard(bsr_mod, name):
    """(index, stored rows, queries) of a shared, never modified shard."""
    if name not in _shards:
        n, dim, nq, seed, plant, dtype = {
            "big": (20000, 768, 40, 7, True, bsr_mod.BSR_F32),
            "600": (600, 768, 12, 8, False, bsr_mod.BSR_F32),
            "40": (40, 768, 5, 9, False, bsr_mod.BSR_F32),
            "130": (5000, 130, 12, 10, True, bsr_mod.BSR_F32),
            "bf16": (5000, 256, 12, 11, True, bsr_mod.BSR_BF16),
        }[name]
        rows, qs = make_shard(n, dim, nq, seed, plant)
        ix = bsr_mod.Index(dim, max_k=256, device=0, dtype=dtype)
        if dtype == bsr_mod.BSR_BF16:
            bits = (rows.view(np.uint32) >> 16).astype(np.uint16)
            rows = (bits.astype(np.uint32) << 16).view(F)  # (the widened values the index keeps)
            ix.load(bits, global_offset=OFFSET)
        else:
            ix.load(rows, global_offset=OFFSET)
        _shards[name] = (ix, rows, qs)
    return _shards[name]


_cands = {}


def cands(oracle_mod, bsr_mod, name, nq, fetch_k):
    key = (name, nq, fetch_k)
    if key not in _cands:
        _, rows, qs = shard(bsr_mod, name)
        _cands[key] = Cands(oracle_mod, rows, np.arange(len(rows)), OFFSET, qs[:nq], fetch_k)
    return _cands[key]


# ---- 1. the big shard: the filter paths ------------------------------------------------------------
@pytest.mark.parametrize("k,fetch_k", [(10, 64), (32, 32), (5, 200)])
@pytest.mark.parametrize("nq", [40, 3])
def test_big_shard(bsr_mod, oracle_mod, gpu, nq, k, fetch_k):
    ix, rows, qs = shard(bsr_mod, "big")
    c = cands(oracle_mod, bsr_mod, "big", nq, fetch_k)
    P = bsr_mod
    plain = ix.local_top_k(qs[:nq], k)
    same(plain, c.top_k(k), "the plain search")
    # lambda = 1: the top-k itself, bit for bit
    got = ix.mmr_search(qs[:nq], k, fetch_k=fetch_k, lambda_mult=1.0, return_rank=True)
    same(got, c.top_k(k), "lambda = 1")
    same(got[:3], plain, "lambda = 1 against local_top_k")
    st = ix.last_stats()
    assert st.search_path & P.BSR_PATH_MMR and st.n_queries == nq and st.n_exact_direct == 0
    assert not st.search_path & (P.BSR_PATH_RANGE | P.BSR_PATH_MASK_LIST | P.BSR_PATH_MASK_FILTER)
    for lam in (0.5, 0.0, 0.3):
        want = c.mmr(k, lam)
        got = ix.mmr_search(qs[:nq], k, fetch_k=fetch_k, lambda_mult=lam, return_rank=True)
        same(got, want, ("lambda", lam))
        assert (got[3][:, 0] == 0).all(), "pick 0 is the top-1"
        d = differing(got, plain)
        print(f"nq={nq} k={k} fetch_k={fetch_k} lambda={lam}: {d} of {nq} lists differ from the top-k; "
              f"path={ix.last_stats().search_path}")
        if lam in (0.5, 0.0) and k < fetch_k:
            assert d == nq, "a pass-through of the top-k would pass otherwise"
        if k == fetch_k:  # a permutation of the candidate list
            assert (np.sort(got[3], axis=1) == np.arange(k)).all()
            assert np.array_equal(np.sort(got[0], axis=1), np.sort(plain[0], axis=1))
            assert d >= 1
    # without the ranks: the same rows
    same(ix.mmr_search(qs[:nq], k, fetch_k=fetch_k, lambda_mult=0.5), c.mmr(k, 0.5)[:3])


def test_default_fetch_k(bsr_mod, oracle_mod, gpu):
    ix, rows, qs = shard(bsr_mod, "big")
    same(ix.mmr_search(qs[:8], 16), cands(oracle_mod, bsr_mod, "big", 8, 64).mmr(16, 0.5)[:3], "fetch_k = 4 k")


# ---- 2. the other shards ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,fetch_k", [("600", 10, 64), ("40", 50, 64), ("130", 10, 64), ("bf16", 10, 64)])
def test_other_shards(bsr_mod, oracle_mod, gpu, name, k, fetch_k):
    ix, rows, qs = shard(bsr_mod, name)
    nq = len(qs)
    c = cands(oracle_mod, bsr_mod, name, nq, fetch_k)
    same(ix.mmr_search(qs, k, fetch_k=fetch_k, lambda_mult=1.0, return_rank=True), c.top_k(k), (name, 1.0))
    for lam in (0.5, 0.0, 0.7):
        got = ix.mmr_search(qs, k, fetch_k=fetch_k, lambda_mult=lam, return_rank=True)
        same(got, c.mmr(k, lam), (name, lam))
    st = ix.last_stats()
    assert st.search_path & bsr_mod.BSR_PATH_MMR
    print(f"{name}: path={st.search_path} emitted={st.n_emitted} direct={st.n_exact_direct} fallback={st.n_fallback}")
    if name == "40":
        assert (got[2] == 40).all() and (got[0][:, 40:] == NONE_IDX).all() and np.isposinf(got[1][:, 40:]).all()
        assert (got[3][:, 40:] == km.RANK_NONE).all()
    assert differing(got, c.top_k(k)) >= 1


# ---- 3. tombstones, update, compaction -------------------------------------------------------------
def test_delete_update_compact(bsr_mod, oracle_mod, gpu):
    rows, qs = make_shard(20000, 768, 8, 7)
    rows = rows.copy()
    n, nq, k, fetch_k = len(rows), 8, 10, 64
    ix = bsr_mod.Index(768, max_k=256, device=0)
    ix.load(rows, global_offset=OFFSET)
    live = np.ones(n, bool)

    def check(ctx, stored=rows, ids=None, offset=OFFSET):
        c = Cands(oracle_mod, stored, np.flatnonzero(live) if ids is None else ids, offset, qs, fetch_k)
        for lam in (0.5, 1.0):
            same(ix.mmr_search(qs, k, fetch_k=fetch_k, lambda_mult=lam, return_rank=True), c.mmr(k, lam), (ctx, lam))
        return c

    # delete each query's top-1: the model over the live rows still matches
    top1 = ix.local_top_k(qs, 1)[0][:, 0]
    assert ix.delete(top1) == nq
    live[(top1 - np.uint64(OFFSET)).astype(np.int64)] = False
    c = check("tombstones")
    assert not np.isin(top1, ix.mmr_search(qs, k, fetch_k=fetch_k)[0]).any()
    # update: a live row of each candidate list becomes a copy of the query itself (the new top-1)
    upd = np.array([c.loc[q][5] for q in range(nq)], np.int64)
    rows[upd] = qs
    ix.update((upd + OFFSET).astype(np.uint64), qs)
    c = check("update")
    assert all(c.loc[q][0] == upd[q] and c.dq[q][0] == 0.0 for q in range(nq))
    # compact: the live rows packed, a new offset
    old = ix.compact(global_offset=123)
    packed = rows[live]
    assert np.array_equal(old, (np.flatnonzero(live) + OFFSET).astype(np.uint64))
    check("compact", stored=packed, ids=np.arange(len(packed)), offset=123)
    ix.close()


# ---- 4. masks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["list", "filter", "auto"])
def test_one_mask(bsr_mod, oracle_mod, gpu, mode):
    ix, rows, qs = shard(bsr_mod, "big")
    n, nq, k, fetch_k = len(rows), 8, 10, 64
    ids = np.flatnonzero(np.random.default_rng(31).random(n) < 0.5)
    key = ("big-mask", nq, fetch_k)
    if key not in _cands:
        _cands[key] = Cands(oracle_mod, rows, ids, OFFSET, qs[:nq], fetch_k)
    c = _cands[key]
    P = bsr_mod
    for lam in (0.5, 1.0):
        got = ix.mmr_search(qs[:nq], k, fetch_k=fetch_k, lambda_mult=lam, allow_ids=ids, mask_mode=mode, return_rank=True)
        same(got, c.mmr(k, lam), (mode, lam))
    st = ix.last_stats()
    assert st.search_path & P.BSR_PATH_MMR and st.graph_replay == 0
    assert st.search_path & (P.BSR_PATH_MASK_LIST if mode == "list" else P.BSR_PATH_MASK_LIST | P.BSR_PATH_MASK_FILTER)
    if mode == "filter":
        assert st.search_path & P.BSR_PATH_MASK_FILTER
    assert not st.search_path & P.BSR_PATH_MASK_GROUPS
    assert np.isin((got[0] - np.uint64(OFFSET)).astype(np.int64), ids).all()


def test_three_masks(bsr_mod, oracle_mod, gpu):
    ix, rows, qs = shard(bsr_mod, "big")
    n, nq, k, fetch_k = len(rows), 9, 10, 64
    rng = np.random.default_rng(32)
    masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.05, np.zeros(n, bool)])
    masks[2, :30] = True  # fewer allowed rows than fetch_k, and than k for none
    qm = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2], np.uint32)
    id_lists = [np.flatnonzero(m) for m in masks]
    c = Cands(oracle_mod, rows, [id_lists[g] for g in qm], OFFSET, qs[:nq], fetch_k)
    for lam in (0.5, 1.0):
        got = ix.mmr_search(qs[:nq], k, fetch_k=fetch_k, lambda_mult=lam, allow_masks=masks, query_mask=qm,
                            return_rank=True)
        same(got, c.mmr(k, lam), ("groups", lam))
    st = ix.last_stats()
    assert st.search_path & bsr_mod.BSR_PATH_MMR and st.search_path & bsr_mod.BSR_PATH_MASK_GROUPS
    got = ix.mmr_search(qs[:nq], 40, fetch_k=fetch_k, lambda_mult=0.5, allow_masks=masks, query_mask=qm)
    same(got, c.mmr(40, 0.5)[:3], "groups, k above a mask's rows")
    assert list(got[2]) == [40, 40, 30] * 3


# ---- 5. device buffers, the optional rank ----------------------------------------------------------
def test_device_buffers(bsr_mod, oracle_mod, gpu):
    import torch
    ix, rows, qs = shard(bsr_mod, "big")
    nq, k, fetch_k = 8, 10, 64
    want = cands(oracle_mod, bsr_mod, "big", nq, fetch_k).mmr(k, 0.5)
    dev = torch.device("cuda:0")
    q = torch.from_numpy(qs[:nq]).to(dev)

    def outs(on_dev):
        t = [torch.full((nq, k), 7, dtype=torch.int64), torch.full((nq, k), 7, dtype=torch.float32),
             torch.full((nq,), 7, dtype=torch.int32), torch.full((nq, k), 7, dtype=torch.int32)]
        return [x.to(dev) if on_dev else x for x in t]

    def read(oi, od, oc, orank):
        return (oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32),
                orank.cpu().numpy().view(np.uint32))

    # everything on the device
    oi, od, oc, orank = outs(True)
    ix.mmr_search_device(q, nq, k, fetch_k, 0.5, oi, od, oc, out_rank=orank)
    same(read(oi, od, oc, orank), want, "device outputs")
    # out_rank NULL: the other three as before, the rank tensor untouched
    oi, od, oc, orank = outs(True)
    ix.mmr_search_device(q, nq, k, fetch_k, 0.5, oi, od, oc)
    same(read(oi, od, oc, orank)[:3], want[:3], "no rank")
    assert (orank == 7).all()
    # mixed: device queries, host indices and ranks, device distances and counts
    oi, od, oc, orank = outs(True)
    hi, _, _, hr = outs(False)
    ix.mmr_search_device(q, nq, k, fetch_k, 0.5, hi, od, oc, out_rank=hr)
    same(read(hi, od, oc, hr), want, "mixed outputs")
    # host queries (numpy), host outputs, a device mask
    ids = np.flatnonzero(np.random.default_rng(31).random(len(rows)) < 0.5)
    words = torch.from_numpy(bsr_mod.pack_allow_mask(len(rows), ids=ids).view(np.int64)).to(dev)
    hi, hd, hc, hr = outs(False)
    ix.mmr_search_device(np.ascontiguousarray(qs[:nq]), nq, k, fetch_k, 0.5, hi, hd, hc, out_rank=hr, allow_words=words)
    c = Cands(oracle_mod, rows, ids, OFFSET, qs[:nq], fetch_k)
    same(read(hi, hd, hc, hr), c.mmr(k, 0.5), "device mask")


# ---- 6. the candidate search keeps its graphs ------------------------------------------------------
@pytest.mark.parametrize("nq", [40, 3])
def test_graph_replay(bsr_mod, oracle_mod, gpu, nq):
    ix, rows, qs = shard(bsr_mod, "big")
    k, fetch_k = 7, 48  # (a shape of this test's own)
    c = cands(oracle_mod, bsr_mod, "big", nq, fetch_k)
    want = c.mmr(k, 0.5)
    replays = []
    for rep in range(4):
        got = ix.mmr_search(qs[:nq], k, fetch_k=fetch_k, lambda_mult=0.5, return_rank=True)
        same(got, want, ("rep", rep))
        st = ix.last_stats()
        assert st.search_path & bsr_mod.BSR_PATH_MMR
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
    same(plain[2], c.top_k(fetch_k), "plain after mmr")
    same(ix.local_top_k(qs[:nq], k), c.top_k(k), "plain k after mmr")


# ---- 7. errors the candidate search reports --------------------------------------------------------
def test_nonfinite_query_leaves_outputs_untouched(bsr_mod, gpu):
    ix, rows, qs = shard(bsr_mod, "big")
    nq, k = 4, 5
    bad = qs[:nq].copy()
    bad[2, 17] = np.nan
    oi, od = np.full((nq, k), 7, np.uint64), np.full((nq, k), 7, F)
    oc, orank = np.full(nq, 7, np.uint32), np.full((nq, k), 7, np.uint32)
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.mmr_search_device(bad, nq, k, 20, 0.5, oi, od, oc, out_rank=orank)
    assert e.value.status == E_NONFINITE
    assert (oi == 7).all() and (od == 7).all() and (oc == 7).all() and (orank == 7).all()
    # allow_words of the wrong length: as the masked search reports it
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.mmr_search_device(qs[:nq].copy(), nq, k, 20, 0.5, oi, od, oc, allow_words=np.zeros(3, np.uint64))
    assert e.value.status == -1 and (oi == 7).all() and (oc == 7).all()
    # the index still answers
    assert ix.mmr_search(qs[:nq], k)[2].tolist() == [k] * nq
