"""Kernel-level checks of the deep MMR selection (csrc/k_mmr.hip: launch_mmr_deep_select) through
the test-only shim, against kcheck_mmr.mmr_model -- bit for bit.  The lists are in arbitrary order
with made-up dq, so a stale score is often above a fresh one; a row id of -1 stands for an id
outside the shard."""
import functools

import numpy as np
import pytest

import kcheck_deep_mmr as kd
import kcheck_exact as kx
import kcheck_mmr as km

pytestmark = pytest.mark.gpu

F = np.float32
N = 3000
OFFSET = 1000
MS = (0, 1, 2, 64, 65, 255, 256, 257, 1023, 1024)


@functools.lru_cache(maxsize=None)
def corpus(dim):
    """kcheck_exact.Corpus with 40 near-copies of one row planted at rows 2000 .. 2039."""
    c = kx.Corpus(N, dim, 2, seed=200 + dim)
    rng = np.random.default_rng(dim)
    c.a[2001:2040] = c.a[2000] + rng.uniform(-1e-3, 1e-3, (39, dim)).astype(F)
    c.rows[:N, :dim] = c.a
    c.na[:N] = kx.seq_norm_f32(c.a)
    return c


def random_lists(c, seed, ms=MS):
    rng = np.random.default_rng(seed)
    return [(rng.choice(N, m, replace=False), rng.uniform(0, 1, m).astype(F)) for m in ms]


def check(c, fetch_k, lists, k, lam, cols, with_rank=True):
    """The kernel over `lists` ((local rows, dq) per query; garbage behind every list) equals the
    model over the in-shard positions; cols caches the model's columns per (query, position).
    Returns (ranks, counts, pairs, the pairs of a full column per pick)."""
    nq = len(lists)
    idx = np.full((nq, fetch_k), OFFSET + 5, np.uint64)
    dist = np.full((nq, fetch_k), np.nan, F)
    cnt = np.array([len(r) for r, _ in lists], np.uint32)
    for q, (r, d) in enumerate(lists):
        r = np.asarray(r, np.int64)
        idx[q, :len(r)] = np.where(r >= 0, OFFSET + r, OFFSET + N + 7).astype(np.uint64)
        dist[q, :len(r)] = d
    rc, gi, gd, gr, gc, pairs = kd.deep_mmr_select(c.rows, c.dim, N, OFFSET, c.na, idx, dist, cnt, k, lam, with_rank)
    assert rc == 0
    dense = 0
    for q, (r, d) in enumerate(lists):
        r = np.asarray(r, np.int64)
        pos = np.flatnonzero(r >= 0)

        def pair(cand_rows, j, q=q):
            if (q, j) not in cols:
                cols[q, j] = km.pair_distances(cand_rows, j)
            return cols[q, j]
        picks, _ = km.mmr_model(c.a[r[pos]], np.asarray(d, F)[pos], k, lam, pair=pair)
        wi, wd, wr, wc = km.mmr_outputs(pos[picks], idx[q, :len(r)], d, k)
        assert gc[q] == wc and np.array_equal(gi[q], wi), (q, len(r), gr[q] if with_rank else None, wr)
        assert np.array_equal(gd[q].view(np.uint32), wd.view(np.uint32))
        assert not with_rank or np.array_equal(gr[q], wr)
        dense += max(wc - 1, 0) * len(pos)
    assert pairs <= dense  # (every pair distance at most once)
    return gr, gc, pairs, dense


@pytest.mark.parametrize("dim,ks,lams", [(64, (1, 2, 65, 256), (0.0, 0.3, 0.5, 1.0)), (130, (2, 65), (0.5,)),
                                         (768, (65,), (0.3,)), (1100, (2, 65), (0.5, 1.0))])
def test_shapes(gpu, dim, ks, lams):
    c, cols = corpus(dim), {}
    lists = random_lists(c, dim)
    for k in ks:
        for lam in lams:
            _, cnt, _, _ = check(c, 1024, lists, k, lam, cols, with_rank=(k != 2))
            assert list(cnt) == [min(k, m) for m in MS]


def test_crafted(gpu):
    c, cols = corpus(64), {}
    rng = np.random.default_rng(1)
    ties = (np.concatenate([[17], np.arange(c.run, c.run + 80)]), np.full(81, 0.25, F))  # every score ties
    rows = rng.choice(np.arange(100, 1000), 300, replace=False)
    rows[5], rows[290] = c.ident[0], c.ident[1]                  # two identical rows, equal dq
    dq = rng.uniform(0.8, 0.9, 300).astype(F)
    dq[5] = dq[290] = F(0.01)
    # 40 near-copies at the head of a sorted 1024-list: the rows behind them wait several picks
    head = np.concatenate([np.arange(2000, 2040), rng.choice(1900, 984, replace=False)])
    cluster = (head, np.sort(rng.uniform(0.1, 0.9, 1024)).astype(F))
    scattered = rng.choice(N, 500, replace=False)                # ids outside the shard through the list
    scattered[rng.choice(500, 120, replace=False)] = -1
    scattered[0] = -1
    lists = [ties, (rows, dq), cluster, (scattered, rng.uniform(0, 1, 500).astype(F))]
    rank, _, _, _ = check(c, 1024, lists, 6, 0.5, cols)
    assert list(rank[0]) == [0, 1, 2, 3, 4, 5]
    assert list(rank[1][:2]) == [0, 5] and 290 not in rank[1]
    rank, _, pairs, dense = check(c, 1024, lists, 50, 0.5, cols)
    assert len(set(rank[2]) & set(range(40))) < 5                # (the cluster gives few picks)
    check(c, 1024, lists, 64, 1.0, cols)
    # a smaller stride with k = fetch_k: a permutation of each list
    check(c, 100, random_lists(c, 3, ms=(0, 1, 65, 100)), 100, 0.3, {})


def test_lazy_at_lambda_one(gpu):
    # scores do not depend on mind: after the dense first column only the head of the order is refreshed
    c = corpus(64)
    lists = random_lists(c, 9, ms=(1024,))
    _, _, pairs, dense = check(c, 1024, lists, 64, 1.0, {})
    assert dense == 63 * 1024 and pairs < dense // 2


def test_large_batch(gpu):
    c = corpus(64)
    rng = np.random.default_rng(3)
    ms = [int(m) for m in rng.choice([0, 1, 30, 70, 200, 300], 200)]
    lists = random_lists(c, 4, ms=ms)
    check(c, 300, lists, 8, 0.5, {})
    check(c, 300, lists, 8, 0.7, {}, with_rank=False)


def test_refusals(gpu):
    c = corpus(64)
    (r, d), = random_lists(c, 1, ms=(5,))

    def call(fetch_k, k, lam):
        idx = np.full((1, fetch_k), OFFSET, np.uint64)
        rc, gi, gd, gr, gc, pairs = kd.deep_mmr_select(c.rows, c.dim, N, OFFSET, c.na, idx, np.zeros((1, fetch_k), F),
                                                       np.array([5], np.uint32), k, lam)
        assert rc == 1 and (gi == 0x1234).all() and np.isnan(gd).all() and (gc == 0x5A5A5A5A).all() and pairs == 0
    for fetch_k, k, lam in ((1024, 0, 0.5), (1024, 257, 0.5), (4, 5, 0.5), (1025, 4, 0.5), (1024, 4, np.nan),
                            (1024, 4, -0.1), (1024, 4, 1.5)):
        call(fetch_k, k, lam)
