"""Scoring caller-chosen rows (bsr_local_score_ids / bsr_local_rerank_ids) through
the C ABI.  Every expected distance is oracle.np_cosine_distances(rows, query)[id - offset] over
the rows the index returns from get_many, compared as uint32 bit patterns -- no tolerance anywhere;
an absent slot is +inf.  Every parametrised case checks that at least half of its slots are present."""
import numpy as np
import pytest

import kcheck_score as ks

pytestmark = pytest.mark.gpu

F = np.float32
PADI = 2 ** 64 - 1  # the padding value, as a Python integer (for lists) ...
PAD = np.uint64(PADI)  # ... and as an array element
NONE_IDX = PAD
E_NONFINITE = -2
N, DIM, OFFSET, NQ = 1000, 768, 12345, 17
TWIN = (40, 700)  # two identical stored rows


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


class Shard:
    """An index with its rows on the host (as get_many returns them: a bf16 index's widened values),
    its offset, its tombstones, and the oracle's distance of every row to every query, computed once."""

    def __init__(self, oracle_mod, ix, qs):
        self.oracle, self.ix, self.qs = oracle_mod, ix, qs
        self.refresh()

    def refresh(self, dead=None):
        self.rows = self.ix.get_many()
        self.offset = self.ix.global_offset()
        self.dead = np.zeros(len(self.rows), bool) if dead is None else dead
        self.all_dist = [self.oracle.np_cosine_distances(self.rows, q) for q in self.qs]

    def want(self, ids, queries=None):
        """(dist [nq][m], found [nq]) of ids [nq][m] for the first nq queries (or the positions given)."""
        qsel = range(len(ids)) if queries is None else queries
        dist = np.empty((len(ids), len(ids[0])), F)
        found = np.zeros(len(ids), np.uint32)
        for i, q in enumerate(qsel):
            dist[i], found[i], _ = ks.score_model(self.all_dist[q], ids[i], self.offset, self.dead)
        return dist, found


def make_rows(seed, n=N, dim=DIM):
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-1, 1, (n, dim)).astype(F)
    if n > TWIN[1]:
        rows[TWIN[1]] = rows[TWIN[0]]
    qs = rng.uniform(-1, 1, (NQ, dim)).astype(F)
    qs[0] = rows[3]  # a query equal to a stored row
    return rows, qs


@pytest.fixture(scope="module")
def shards(bsr_mod, oracle_mod, gpu):
    """The small index in f32 and in bf16 (read-only: the tests that change an index build their own)."""
    rows, qs = make_rows(31)
    f32 = bsr_mod.Index(DIM, max_k=256, device=0)
    f32.load(rows, global_offset=OFFSET)
    b16 = bsr_mod.Index(DIM, max_k=256, device=0, dtype=bsr_mod.BSR_BF16)
    b16.load((rows.view(np.uint32) >> 16).astype(np.uint16), global_offset=OFFSET)
    out = {"f32": Shard(oracle_mod, f32, qs), "bf16": Shard(oracle_mod, b16, qs)}
    yield out
    f32.close()
    b16.close()


def fresh(bsr_mod, oracle_mod, seed=31, offset=OFFSET, **kw):
    rows, qs = make_rows(seed)
    ix = bsr_mod.Index(DIM, max_k=256, device=0, **kw)
    ix.load(rows, global_offset=offset)
    return Shard(oracle_mod, ix, qs)


def mixed_lists(rng, nq, m, offset, n, dead=None):
    """ids [nq][m]: about 70% name live rows of the shard (with replacement: repeats), the rest are
    padding, ids below and above the shard, and deleted rows where there are any.  m = 1: present."""
    live = np.arange(n) if dead is None else np.flatnonzero(~dead)
    gone = np.zeros(0, np.int64) if dead is None else np.flatnonzero(dead)
    ids = np.empty((nq, m), np.uint64)
    for q in range(nq):
        for j in range(m):
            kind = 0 if m == 1 else int(rng.integers(0, 10))
            if kind < 7:
                ids[q, j] = offset + int(rng.choice(live))
            elif kind == 7:
                ids[q, j] = PAD
            elif kind == 8:
                ids[q, j] = (offset - 1 - int(rng.integers(0, offset)) if offset and rng.random() < 0.5
                             else offset + n + int(rng.integers(0, 1 << 40)))
            else:
                ids[q, j] = offset + int(rng.choice(gone)) if len(gone) else 2 ** 64 - 2
    return ids


# ---- score_ids against the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 100, 257))
@pytest.mark.parametrize("nq", (1, 17))
@pytest.mark.parametrize("kind", ("f32", "bf16"))
def test_score_ids_matches_the_oracle(bsr_mod, shards, kind, nq, m):
    s = shards[kind]
    rng = np.random.default_rng(1000 * nq + m)
    ids = mixed_lists(rng, nq, m, s.offset, len(s.rows))
    wd, wf = s.want(ids)
    assert 2 * int(wf.sum()) >= nq * m
    dist, found = s.ix.score_ids(s.qs[:nq], ids, return_found=True)
    assert dist.dtype == F and dist.shape == (nq, m) and found.dtype == np.uint32
    assert np.array_equal(bits(dist), bits(wd))
    assert np.array_equal(found, wf)
    st = s.ix.last_stats()
    assert st.search_path == bsr_mod.BSR_PATH_SCORE and st.n_queries == nq and st.n_candidates == m
    assert st.graph_replay == 0 and st.n_emitted == 0 and st.n_exact_direct == 0 and st.n_fallback == 0
    assert st.n_rescued == 0 and st.filter_op == 0 and st.row_ebound == 0
    if kind == "bf16":  # (the values scored are the widened stored ones)
        assert np.array_equal(s.rows.view(np.uint32) & 0xFFFF, np.zeros_like(s.rows, np.uint32))


def test_special_rows(bsr_mod, oracle_mod, gpu):
    s = fresh(bsr_mod, oracle_mod)
    ix, off = s.ix, s.offset
    ix.update([off + 9], np.zeros((1, DIM), F))  # a zero stored row
    s.refresh()
    qs = s.qs.copy()
    qs[1] = 0  # a zero query
    s.qs = qs
    s.refresh()
    ids = np.array([[off + 3, off + 9, off + 500], [off + 3, off + 4, off + 500], [off + 3, off + 9, off + 500]],
                   np.uint64)
    dist, found = ix.score_ids(qs[:3], ids, return_found=True)
    assert np.array_equal(bits(dist), bits(s.want(ids)[0])) and found.tolist() == [3, 3, 3]
    assert bits(dist[0, 0]) == 0, "a query equal to a stored row scores exactly 0.0"
    assert dist[0, 1] == 1.0 and dist[2, 1] == 1.0, "a zero stored row scores 1.0"
    assert (dist[1] == 1.0).all(), "a zero query scores 1.0 everywhere"
    # ... except against the zero row itself: the reference's identical-vectors rule comes first
    d00 = ix.score_ids(qs[1], [off + 9])
    assert bits(d00[0, 0]) == 0 and d00[0, 0] == s.all_dist[1][9]
    ix.close()


def test_absent_kinds(bsr_mod, shards):
    s = shards["f32"]
    off, n = s.offset, len(s.rows)
    lists = [[off, off + n - 1, off - 1, off + n], [PADI, 0, 2 ** 64 - 2, off + 5], [off + n + 10 ** 12, PADI, PADI, PADI]]
    dist, found = s.ix.score_ids(s.qs[:3], lists, return_found=True)
    assert np.isfinite(dist[0, :2]).all() and np.isposinf(dist[0, 2:]).all()
    assert np.isposinf(dist[1, :3]).all() and np.isfinite(dist[1, 3])
    assert np.isposinf(dist[2]).all()
    assert found.tolist() == [2, 1, 0]
    assert np.array_equal(bits(dist), bits(s.want(np.array(lists, np.uint64))[0]))
    # ragged lists and negative entries through the wrapper: padding
    dist = s.ix.score_ids(s.qs[:2], [[off + 1, -1, off + 2], [off + 3]])
    assert np.isposinf(dist[0, 1]) and np.isposinf(dist[1, 1:]).all() and np.isfinite(dist[:, 0]).all()
    idx, rd, cnt = s.ix.rerank(s.qs[:3], lists)
    assert cnt.tolist() == [2, 1, 0] and (idx[2] == NONE_IDX).all() and np.isposinf(rd[2]).all()


def test_empty_shard(bsr_mod, gpu):
    ix = bsr_mod.Index(DIM, max_k=64, device=0)
    ix.load(np.zeros((0, DIM), F), global_offset=7)
    q = np.ones((2, DIM), F)
    dist, found = ix.score_ids(q, [[7, 8, 0], [PADI, 6, 7]], return_found=True)
    assert np.isposinf(dist).all() and found.tolist() == [0, 0]
    idx, rd, cnt = ix.rerank(q, [[7, 8, 0], [PADI, 6, 7]], k=2)
    assert cnt.tolist() == [0, 0] and (idx == NONE_IDX).all() and np.isposinf(rd).all()
    ix.close()


def test_mutations(bsr_mod, oracle_mod, gpu):
    s = fresh(bsr_mod, oracle_mod)
    ix, off, nq = s.ix, s.offset, 5
    rng = np.random.default_rng(5)
    ids = mixed_lists(rng, nq, 100, off, N)
    ids[:, 0] = off + 17
    gone = np.unique(ids[0, 1:40][(ids[0, 1:40] >= off) & (ids[0, 1:40] < off + N)])[:10]
    kill = np.append(gone, np.uint64(off + 17))
    ix.delete(kill)
    dead = np.zeros(N, bool)
    dead[(kill - np.uint64(off)).astype(np.int64)] = True
    s.refresh(dead)
    dist, found = ix.score_ids(s.qs[:nq], ids, return_found=True)
    wd, wf = s.want(ids)
    assert np.isposinf(dist[:, 0]).all(), "a deleted row's slot turns +inf"
    assert np.array_equal(bits(dist), bits(wd)) and np.array_equal(found, wf) and 2 * int(wf.sum()) >= ids.size
    # update (the tombstones stay), then append
    upd = np.array([off + 1, off + 400, off + N - 1], np.uint64)
    ids[:, 1:4] = upd
    ix.update(upd, rng.uniform(-1, 1, (3, DIM)).astype(F))
    ix.append_many(rng.uniform(-1, 1, (50, DIM)).astype(F))
    ids[:, 4] = off + N + 49
    ids[:, 5] = off + N + 50  # (one past the appended rows)
    s.refresh(np.append(dead, np.zeros(50, bool)))
    dist, found = ix.score_ids(s.qs[:nq], ids, return_found=True)
    wd, wf = s.want(ids)
    assert np.array_equal(bits(dist), bits(wd)) and np.array_equal(found, wf)
    assert np.isfinite(dist[:, 4]).all() and np.isposinf(dist[:, 5]).all()
    # compact: the ids remapped through the returned map score what they scored, deleted ones are gone
    old = ix.compact(global_offset=77)
    new_of = {int(g): 77 + j for j, g in enumerate(old.tolist())}
    ids2 = np.array([[new_of.get(int(g), 2 ** 64 - 1) for g in row] for row in ids.tolist()], np.uint64)
    s.refresh()
    assert s.offset == 77 and len(s.rows) == len(old)
    dist2, found2 = ix.score_ids(s.qs[:nq], ids2, return_found=True)
    wd2, wf2 = s.want(ids2)
    assert np.array_equal(bits(dist2), bits(wd2)) and np.array_equal(found2, wf2)
    assert np.array_equal(bits(dist2), bits(dist)), "compaction moves rows, it does not change a distance"
    ix.close()


# ---- rerank -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("f32", "bf16"))
def test_rerank_is_the_sorted_scores(bsr_mod, shards, kind):
    s = shards[kind]
    rng = np.random.default_rng(8)
    for nq, m in ((1, 1), (17, 100), (3, 257)):
        ids = mixed_lists(rng, nq, m, s.offset, len(s.rows))
        if m > 2:
            ids[0, :2] = [s.offset + TWIN[1], s.offset + TWIN[0]]
        dist = s.ix.score_ids(s.qs[:nq], ids)
        assert np.array_equal(bits(dist), bits(s.want(ids)[0]))
        assert 2 * int(np.isfinite(dist).sum()) >= nq * m
        for k in sorted({1, max(m // 2, 1), m}):
            idx, rd, cnt = s.ix.rerank(s.qs[:nq], ids, k=k)
            for q in range(nq):
                wi, wd, wc = ks.rerank_model(ids[q], dist[q], k)
                assert cnt[q] == wc, (nq, m, k, q)
                assert np.array_equal(idx[q], wi), (nq, m, k, q)
                assert np.array_equal(bits(rd[q]), bits(wd)), (nq, m, k, q)
    assert s.ix.last_stats().search_path == bsr_mod.BSR_PATH_SCORE


def test_rerank_equals_the_grouped_list_search(bsr_mod, shards):
    """Distinct in-range lists with m <= max_k: the route a caller had before, bit for bit."""
    s = shards["f32"]
    rng = np.random.default_rng(9)
    n = len(s.rows)
    for nq, m in ((5, 100), (17, 256), (2, 1)):
        local = np.stack([rng.choice(n, m, replace=False) for _ in range(nq)])
        masks = np.zeros((nq, n), bool)
        for q in range(nq):
            masks[q, local[q]] = True
        want = s.ix.local_top_k_grouped(s.qs[:nq], m, masks, np.arange(nq), mask_mode="list")
        got = s.ix.rerank(s.qs[:nq], local.astype(np.uint64) + np.uint64(s.offset))
        assert np.array_equal(got[2], want[2]) and (got[2] == m).all()
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(bits(got[1]), bits(want[1]))


def test_identical_rows_come_out_in_id_order(bsr_mod, shards):
    s = shards["f32"]
    a, b = s.offset + TWIN[0], s.offset + TWIN[1]
    dist = s.ix.score_ids(s.qs[:2], [[b, a], [b, a]])
    assert np.array_equal(bits(dist[:, 0]), bits(dist[:, 1]))
    idx, rd, cnt = s.ix.rerank(s.qs[:2], [[b, a], [b, a]])
    assert idx.tolist() == [[a, b], [a, b]] and cnt.tolist() == [2, 2]
    idx, rd, cnt = s.ix.rerank(s.qs[:1], [[b, a, b, b, a]], k=3)  # repeats: each id once
    assert idx.tolist() == [[a, b, int(NONE_IDX)]] and cnt.tolist() == [2]


def test_longest_list(bsr_mod, oracle_mod, gpu):
    """m = BSR_SCORE_MAX_IDS = 4096, nq = 2, on a 5000 x 64 index."""
    rng = np.random.default_rng(4096)
    n, dim, off, m = 5000, 64, 3, 4096
    rows = rng.uniform(-1, 1, (n, dim)).astype(F)
    qs = rng.uniform(-1, 1, (2, dim)).astype(F)
    ix = bsr_mod.Index(dim, max_k=64, device=0)
    ix.load(rows, global_offset=off)
    ids = np.stack([rng.choice(n, m, replace=False), rng.integers(0, n + 1000, m)]).astype(np.uint64) + np.uint64(off)
    all_dist = [oracle_mod.np_cosine_distances(ix.get_many(), q) for q in qs]
    dist, found = ix.score_ids(qs, ids, return_found=True)
    for q in range(2):
        wd, wf, _ = ks.score_model(all_dist[q], ids[q], off)
        assert np.array_equal(bits(dist[q]), bits(wd)) and found[q] == wf
    assert found[0] == m and 2 * int(found.sum()) >= 2 * m
    for k in (m, 10):
        idx, rd, cnt = ix.rerank(qs, ids, k=k)
        for q in range(2):
            wi, wd, wc = ks.rerank_model(ids[q], dist[q], k)
            assert cnt[q] == wc and np.array_equal(idx[q], wi) and np.array_equal(bits(rd[q]), bits(wd))
    assert cnt[0] == 10
    with pytest.raises(bsr_mod.BsrError):
        ix.rerank_device(qs, 2, np.zeros((2, 4097), np.uint64), 4097, 1, idx, rd, cnt)
    dist = ix.score_ids(qs, np.zeros((2, 4097), np.uint64) + np.uint64(off))  # (the scores have no such limit)
    assert dist.shape == (2, 4097) and np.array_equal(bits(dist[:, 0]), bits(np.array([d[0] for d in all_dist])))
    ix.close()


# ---- several ranks ------------------------------------------------------------------------------
def test_two_shards_combine_with_a_minimum(bsr_mod, oracle_mod, gpu):
    rows, qs = make_rows(31)
    half = N // 2
    whole, lo, hi = (bsr_mod.Index(DIM, max_k=64, device=0) for _ in range(3))
    whole.load(rows, global_offset=0)
    lo.load(rows[:half], global_offset=0)
    hi.load(rows[half:], global_offset=half)
    ids = mixed_lists(np.random.default_rng(2), 7, 100, 0, N)
    dw, fw = whole.score_ids(qs[:7], ids, return_found=True)
    dl, fl = lo.score_ids(qs[:7], ids, return_found=True)
    dh, fh = hi.score_ids(qs[:7], ids, return_found=True)
    assert np.array_equal(bits(np.minimum(dl, dh)), bits(dw))
    assert np.array_equal(fl + fh, fw) and fl.all() and fh.all() and 2 * int(fw.sum()) >= ids.size
    assert not (np.isfinite(dl) & np.isfinite(dh)).any(), "an id is present on at most one rank"
    for ix in (whole, lo, hi):
        ix.close()


# ---- pointers, errors, state --------------------------------------------------------------------
def test_device_pointers_match_the_host_form(bsr_mod, shards):
    import torch
    s = shards["f32"]
    nq, m, k = 5, 100, 30
    ids = mixed_lists(np.random.default_rng(3), nq, m, s.offset, len(s.rows))
    hd, hf = s.ix.score_ids(s.qs[:nq], ids, return_found=True)
    hi, hrd, hc = s.ix.rerank(s.qs[:nq], ids, k=k)
    dq = torch.from_numpy(s.qs[:nq].copy()).to("cuda:0")
    dids = torch.from_numpy(ids.view(np.int64)).to("cuda:0")
    od = torch.full((nq, m), 5.0, dtype=torch.float32, device="cuda:0")
    of = torch.full((nq,), 5, dtype=torch.int32, device="cuda:0")
    s.ix.score_ids_device(dq, nq, dids, m, od, of)
    torch.cuda.synchronize()
    assert np.array_equal(bits(od.cpu().numpy()), bits(hd)) and np.array_equal(of.cpu().numpy().view(np.uint32), hf)
    # mixed: device queries, host ids, a host output, no found
    od2 = np.full((nq, m), 5, F)
    s.ix.score_ids_device(dq, nq, ids, m, od2)
    assert np.array_equal(bits(od2), bits(hd))
    oi = torch.full((nq, k), 5, dtype=torch.int64, device="cuda:0")
    ord_ = torch.full((nq, k), 5.0, dtype=torch.float32, device="cuda:0")
    oc = torch.full((nq,), 5, dtype=torch.int32, device="cuda:0")
    s.ix.rerank_device(dq, nq, dids, m, k, oi, ord_, oc)
    torch.cuda.synchronize()
    assert np.array_equal(oi.cpu().numpy().view(np.uint64), hi) and np.array_equal(bits(ord_.cpu().numpy()), bits(hrd))
    assert np.array_equal(oc.cpu().numpy().view(np.uint32), hc)
    hc2 = np.full(nq, 5, np.uint32)  # (a host count beside device rows)
    s.ix.rerank_device(s.qs[:nq].copy(), nq, dids, m, k, oi, ord_, hc2)
    assert np.array_equal(hc2, hc)


def test_nan_query_is_an_error_and_writes_nothing(bsr_mod, shards):
    import torch
    s = shards["f32"]
    nq, m, k = 3, 8, 4
    qs = s.qs[:nq].copy()
    qs[1, 5] = np.nan
    ids = np.full((nq, m), s.offset + 1, np.uint64)
    od, of = np.full((nq, m), 9, F), np.full(nq, 9, np.uint32)
    oi, ord_, oc = np.full((nq, k), 9, np.uint64), np.full((nq, k), 9, F), np.full(nq, 9, np.uint32)
    with pytest.raises(bsr_mod.BsrError) as e:
        s.ix.score_ids_device(qs, nq, ids, m, od, of)
    assert e.value.status == E_NONFINITE and "query 1" in str(e.value)
    with pytest.raises(bsr_mod.BsrError) as e:
        s.ix.rerank_device(qs, nq, ids, m, k, oi, ord_, oc)
    assert e.value.status == E_NONFINITE
    assert all((a == 9).all() for a in (od, of, oi, ord_, oc))
    dd = torch.full((nq, m), 9.0, dtype=torch.float32, device="cuda:0")
    df = torch.full((nq,), 9, dtype=torch.int32, device="cuda:0")
    di = torch.full((nq, k), 9, dtype=torch.int64, device="cuda:0")
    dr = torch.full((nq, k), 9.0, dtype=torch.float32, device="cuda:0")
    dc = torch.full((nq,), 9, dtype=torch.int32, device="cuda:0")
    dq = torch.from_numpy(qs).to("cuda:0")
    with pytest.raises(bsr_mod.BsrError) as e:
        s.ix.score_ids_device(dq, nq, ids, m, dd, df)
    assert e.value.status == E_NONFINITE
    with pytest.raises(bsr_mod.BsrError) as e:
        s.ix.rerank_device(dq, nq, ids, m, k, di, dr, dc)
    assert e.value.status == E_NONFINITE
    torch.cuda.synchronize()
    assert all(bool((t == 9).all()) for t in (dd, df, di, dr, dc))


def test_plain_searches_around_a_score_call(bsr_mod, oracle_mod, gpu):
    """A score call and a rerank between plain searches: their results and their graph replay are
    untouched (the first score call of a size allocates: the plain search re-captures once)."""
    rng = np.random.default_rng(12)
    rows = rng.uniform(-1, 1, (6000, 130)).astype(F)
    qs = rng.uniform(-1, 1, (6, 130)).astype(F)
    ix = bsr_mod.Index(130, max_k=64, device=0)
    ix.load(rows, global_offset=OFFSET)
    first = None
    for rep in range(3):
        got = ix.local_top_k(qs, 10)
        first = first or got
    assert ix.last_stats().graph_replay == 1
    ids = first[0]  # the plain search's own result, scored again: the same distances at the same places
    dist = ix.score_ids(qs, ids)
    st = ix.last_stats()
    assert st.search_path == bsr_mod.BSR_PATH_SCORE and st.graph_replay == 0
    assert np.array_equal(bits(dist), bits(first[1]))
    idx, rd, cnt = ix.rerank(qs, ids[:, ::-1].copy())
    assert ix.last_stats().search_path == bsr_mod.BSR_PATH_SCORE and ix.last_stats().graph_replay == 0
    assert np.array_equal(idx, first[0]) and np.array_equal(bits(rd), bits(first[1])) and (cnt == 10).all()
    for rep in range(3):
        got = ix.local_top_k(qs, 10)
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[2], first[2]), rep
        assert np.array_equal(bits(got[1]), bits(first[1])), rep
    assert ix.last_stats().graph_replay == 1
    ix.close()
