"""Kernel-level checks of the MMR selection (csrc/k_exact.hip: launch_mmr_select) through the
test-only shim, against the model of tests/kcheck_mmr.py -- bit for bit.

The lists are handed to the kernel in arbitrary order with query distances made up here: the kernel
takes both as they stand.  The rows come from kcheck_exact.Corpus (identical copies, a near copy,
zero rows, a negated row, a run of 100 identical rows)."""
import functools

import numpy as np
import pytest

import kcheck_exact as kx
import kcheck_mmr as km

pytestmark = pytest.mark.gpu

F = np.float32
N = 3000
OFFSET = 1000
DIMS = (64, 130, 768, 1100)  # one chunk; a partial last chunk; 12 chunks; past the LDS vector (global reads)
MS = (0, 1, 2, 63, 64, 65, 100, 256)


@functools.lru_cache(maxsize=None)
def corpus(dim):
    return kx.Corpus(N, dim, 2, seed=100 + dim)


class Lists:
    """A batch of candidate lists over one corpus: rows [nq] of arrays (local row ids, any order, a
    row may repeat), dq [nq] of arrays; the kernel's inputs with garbage behind every list, and the
    model's outputs with the pair distances computed once per (list, column)."""

    def __init__(self, c, fetch_k, lists):
        self.c, self.fetch_k = c, fetch_k
        self.rows = [np.asarray(r, np.int64) for r, _ in lists]
        self.dq = [np.asarray(d, F) for _, d in lists]
        nq = len(lists)
        self.idx = np.full((nq, fetch_k), 0xFFFFFFFFFFFFFFFF, np.uint64)
        self.idx[:, 1::2] = np.uint64(OFFSET + N)  # (ids past the shard behind the lists: never read)
        self.dist = np.full((nq, fetch_k), np.nan, F)
        self.cnt = np.zeros(nq, np.uint32)
        for q, (r, d) in enumerate(zip(self.rows, self.dq)):
            assert len(r) == len(d) <= fetch_k and (r < N).all()
            self.idx[q, :len(r)] = (OFFSET + r).astype(np.uint64)
            self.dist[q, :len(r)] = d
            self.cnt[q] = len(r)
        self._cols = [dict() for _ in lists]

    def _pair(self, q):
        def pair(cand_rows, j):
            col = self._cols[q].get(j)
            if col is None:
                col = self._cols[q][j] = km.pair_distances(cand_rows, j)
            return col
        return pair

    def want(self, k, lam):
        nq = len(self.rows)
        idx = np.empty((nq, k), np.uint64)
        dist = np.empty((nq, k), F)
        rank = np.empty((nq, k), np.uint32)
        cnt = np.empty(nq, np.uint32)
        for q in range(nq):
            picks, _ = km.mmr_model(self.c.a[self.rows[q]], self.dq[q], k, lam, pair=self._pair(q))
            idx[q], dist[q], rank[q], cnt[q] = km.mmr_outputs(picks, self.idx[q, :len(self.rows[q])], self.dq[q], k)
        return idx, dist, rank, cnt

    def check(self, k, lam, with_rank=True):
        c = self.c
        rc, idx, dist, rank, cnt = km.mmr_select(c.rows, c.dim, N, OFFSET, c.na, self.idx, self.dist, self.cnt, k, lam,
                                                 with_rank=with_rank)
        assert rc == 0
        w_idx, w_dist, w_rank, w_cnt = self.want(k, lam)
        assert np.array_equal(cnt, w_cnt)
        bad = np.flatnonzero((idx != w_idx).any(axis=1))
        assert bad.size == 0, (bad[:8], idx[bad[0]], w_idx[bad[0]])
        assert np.array_equal(dist.view(np.uint32), w_dist.view(np.uint32))
        if with_rank:
            assert np.array_equal(rank, w_rank)
        return w_rank, w_cnt


def shape_lists(c, seed, ms=MS):
    """One list per m: random rows mixed with the corpus's special rows, random dq."""
    rng = np.random.default_rng(seed)
    special = np.array(c.special_rows())
    out = []
    for m in ms:
        ns = min(m // 2, len(special))
        rows = np.concatenate([rng.choice(special, ns, replace=False), rng.choice(N, m - ns, replace=False)])
        rng.shuffle(rows)
        out.append((rows, rng.uniform(0, 1, m).astype(F)))
    return out


def crafted_lists(c, seed):
    rng = np.random.default_rng(seed)
    out = []
    # every score a tie: position 0 a random row, then 80 rows of the identical run, every dq equal --
    # each pick must be the lowest position left
    rows = np.concatenate([[17], np.arange(c.run, c.run + 80)])
    out.append((rows, np.full(len(rows), 0.25, F)))
    # two mutually identical rows (positions 5 and 9) with equal dq well below the others: they tie
    # for the second pick
    rows = rng.choice(np.arange(100, 1000), 40, replace=False)
    rows[5], rows[9] = c.ident[0], c.ident[1]
    dq = rng.uniform(0.3, 0.9, 40).astype(F)
    dq[5] = dq[9] = F(0.01)
    out.append((rows, dq))
    # the same row in different waves (positions 10, 70, 140, 200), equal dq: a tie across waves, then
    # the copies drop with mind = 0
    rows = rng.choice(np.arange(1000, 2000), 256, replace=False)
    dq = rng.uniform(0.3, 0.9, 256).astype(F)
    for p in (10, 70, 140, 200):
        rows[p], dq[p] = 2500, F(0.02)
    out.append((rows, dq))
    # zero rows, the negated row and the near copy next to their originals, sorted dq as a search gives
    rows = np.array(c.ident + [c.near] + c.zero + [c.neg, 40, 41, 42])
    out.append((rows, np.sort(rng.uniform(0, 1, len(rows))).astype(F)))
    return out


@pytest.mark.parametrize("dim", DIMS)
def test_mmr_select_shapes(gpu, dim):
    c = corpus(dim)
    L = Lists(c, 256, shape_lists(c, dim) + crafted_lists(c, dim + 1))
    for lam in (0.0, 0.3, 0.5, 1.0):
        L.check(10, lam)
    # k = 1, 2, and every k that equals an m or straddles a wave; k = fetch_k
    for k in (1, 2, 63, 64, 65, 100, 256):
        rank, cnt = L.check(k, 0.5, with_rank=(k != 2))
        assert list(cnt[:len(MS)]) == [min(k, m) for m in MS]
    rank, cnt = L.check(256, 0.0)
    # k = fetch_k: a permutation of the list
    for q in range(len(L.rows)):
        assert sorted(rank[q, :cnt[q]]) == list(range(len(L.rows[q])))


def test_mmr_select_crafted_orders(gpu):
    """What the crafted lists are there for, read off the model's picks (the kernel equals them)."""
    c = corpus(768)
    L = Lists(c, 256, crafted_lists(c, 5))
    rank, cnt = L.check(6, 0.5)
    assert list(rank[0]) == [0, 1, 2, 3, 4, 5]           # all ties: position order
    assert list(rank[1][:2]) == [0, 5] and 9 not in rank[1]  # the tie to the lower; its copy drops
    r2 = list(rank[2])
    assert r2[:2] == [0, 10] and not {70, 140, 200} & set(r2)
    rank, _ = L.check(4, 1.0)                             # lambda = 1: position 0, then dq order, ties by position
    assert list(rank[2]) == [0, 10, 70, 140]


def test_mmr_select_smaller_fetch_k(gpu):
    # a stride below 256: fetch_k = 100 with m up to 100, k = fetch_k; and cand_cnt above fetch_k is cut
    c = corpus(130)
    L = Lists(c, 100, shape_lists(c, 9, ms=(0, 1, 65, 100)))
    L.check(100, 0.3)
    L.check(7, 0.5)
    L.cnt[3] = 1000
    L.check(7, 0.5)


def test_mmr_select_large_batch(gpu):
    # more workgroups than the 256 CUs hold at once: 300 lists of 0 .. 70 rows
    c = corpus(64)
    rng = np.random.default_rng(3)
    lists = []
    for _ in range(300):
        m = int(rng.integers(0, 71))
        lists.append((rng.choice(N, m, replace=False), rng.uniform(0, 1, m).astype(F)))
    L = Lists(c, 72, lists)
    L.check(8, 0.5)
    L.check(8, 0.7, with_rank=False)


def test_mmr_select_refusals(gpu):
    c = corpus(64)
    L = Lists(c, 256, shape_lists(c, 1, ms=(5,)))
    for k, lam in ((0, 0.5), (257, 0.5), (4, np.nan), (4, -0.1), (4, 1.5)):
        rc, idx, dist, rank, cnt = km.mmr_select(c.rows, c.dim, N, OFFSET, c.na, L.idx, L.dist, L.cnt, k, lam)
        assert rc == 1, (k, lam)
        assert (idx == 0x1234).all() and np.isnan(dist).all() and (rank == 0x5A5A5A5A).all() and (cnt == 0x5A5A5A5A).all()
    # fetch_k above 256
    big = Lists(c, 257, shape_lists(c, 1, ms=(5,)))
    rc, idx, *_ = km.mmr_select(c.rows, c.dim, N, OFFSET, c.na, big.idx, big.dist, big.cnt, 4, 0.5)
    assert rc == 1 and (idx == 0x1234).all()
