"""The sample scored once: for batches of more than 16 queries over a
shard whose sample is compact (ceil(n / 32) >= 256 ks, i.e. n >= 65,505 rows at k <= 10), the
sample pass scores one 128-row tile of the filter operand in 32 (tiles 31, 63, ...), the emit
pass skips those tiles and a fix-up kernel emits their rows from the sample maxima and the final
threshold.  Every case is compared with the oracle -- counts, indices, order and f32 distance
bits -- and asserts from last_stats() that the filter answered every query: a broken fix-up must
not pass on the exact-scan fallback.  (The inputs take no fallback on the every-32nd-row sample
either; only the ties case's emitted count is particular to the sample tiles.)

Shapes: d = 768, shards of 65k-200k rows; the oracle runs over a subset of a large batch's
queries, and every query of such a batch is also compared with the same index searched 16
queries at a time (the skinny kernels: another sample, another emit kernel, the same answer).
BSR_SAMPLE_TILES=0 switches the sample tiles off (the every-32nd-row sample for every batch)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, K = 768, 10
THREADS = 16
TILE, EVERY, PHASE = 128, 32, 31          # a sample tile: 128 rows, tile index % 32 == 31
N_FULL = 17 * 4096                        # 69,632: 544 tiles, the last one a (full) sample tile
N_PART_SAMPLE = N_FULL - 37               # 69,595: the partial last tile (91 rows) is sample tile 543
N_PART_OTHER = 70_001                     # 547 tiles: the partial last tile (113 rows) is no sample tile
N_COMPACT_MIN = 2047 * 32 + 1             # 65,505: ceil(n / 32) = 2048 = 256 ks, the compact limit
N_MAX = N_PART_OTHER


def _tile0(t):
    return t * TILE


def _is_sample_tile(t):
    return t % EVERY == PHASE


@pytest.fixture(scope="module")
def base(gpu):
    """One uniform corpus and query set; every case takes a prefix of the rows (a copy when it plants)."""
    rng = np.random.default_rng(20261019)
    rows = rng.uniform(-1, 1, (N_MAX, D)).astype(np.float32)
    qs = rng.uniform(-1, 1, (1000, D)).astype(np.float32)
    return rows, qs


def _oracle(oracle_mod, rows, qs):
    return oracle_mod.parallel_top_k(np.ascontiguousarray(rows), np.ascontiguousarray(qs), K, size=4,
                                     threads=THREADS)


def _same(got, want, sub, ctx, k=K):
    gi, gd, gc = got
    wi, wd, wc = want
    for j, q in enumerate(sub):
        c = int(wc[j])
        assert int(gc[q]) == min(c, k), (ctx, q, gc[q], c)
        c = min(c, k)
        assert np.array_equal(gi[q, :c], wi[j, :c]), (ctx, q, gi[q, :c], wi[j, :c])
        assert np.array_equal(gd[q, :c].view(np.uint32), wd[j, :c].view(np.uint32)), (ctx, q)


def _filtered(st, nq, ctx):
    """The filter answered every query: no exact scan, by design or as a fallback."""
    print(f"{ctx}: fallback={st.n_fallback} exact_direct={st.n_exact_direct} rescued={st.n_rescued} "
          f"emitted={st.n_emitted} candidates={st.n_candidates} path={st.search_path}")
    assert st.n_queries == nq, ctx
    assert st.n_fallback == 0 and st.n_exact_direct == 0, (ctx, st.n_fallback, st.n_exact_direct)
    assert st.n_candidates == 63 and st.n_emitted >= nq, (ctx, st.n_candidates, st.n_emitted)


def _search(bsr_mod, rows, qs, k=K):
    ix = bsr_mod.Index(D, max_k=16, device=0)
    ix.load(rows)
    got = ix.local_top_k(qs, k)
    st = ix.last_stats()
    return ix, got, st


# ---- row counts ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N_FULL, N_PART_SAMPLE, N_PART_OTHER, N_COMPACT_MIN, N_COMPACT_MIN - 1])
def test_row_counts(bsr_mod, oracle_mod, base, monkeypatch, n):
    """n a multiple of 4096; a partial last tile that is a sample tile; one that is not; n at the
    compact limit and one row below it (the every-32nd-row sample: still exact).  Queries equal to
    rows at the shard's end, in sample tiles and beside them."""
    rows, qs = base
    rows = rows[:n]
    nq = 24
    q = qs[:nq].copy()
    last_tile = (n - 1) // TILE
    picks = [0, n - 1, n - 33, _tile0(last_tile), _tile0(31) + 5, _tile0(31) - 1, _tile0(32), _tile0(63) + 127]
    for j, r in enumerate(picks):
        q[j] = rows[r]
    ix, got, st = _search(bsr_mod, rows, q)
    _filtered(st, nq, f"n={n}")
    _same(got, _oracle(oracle_mod, rows, q), range(nq), f"n={n}")
    for j, r in enumerate(picks):
        assert got[0][j, 0] == r and got[1][j, 0] == 0.0, (n, j, r, got[0][j, :3])
    if n in (N_COMPACT_MIN, N_COMPACT_MIN - 1):
        # Which sample ran shows in the emitted count (the threshold differs): with the sample
        # tiles switched off it is unchanged below the compact limit -- the every-32nd-row sample
        # ran both times -- and changes at the limit.
        monkeypatch.setenv("BSR_SAMPLE_TILES", "0")
        off = ix.local_top_k(q, K)
        st_off = ix.last_stats()
        _filtered(st_off, nq, f"n={n} sample tiles off")
        assert all(np.array_equal(a, b) for a, b in zip(got, off))
        assert (st_off.n_emitted == st.n_emitted) == (n < N_COMPACT_MIN), (n, st_off.n_emitted, st.n_emitted)
    ix.close()


# ---- batch sizes -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch_shard(bsr_mod, oracle_mod, base):
    """The shard of the batch-size cases (a partial last sample tile) and, computed once, every
    query's answer from searches of 16 queries at a time and the oracle's over a subset."""
    rows, qs = base
    rows = rows[:N_PART_SAMPLE]
    ix = bsr_mod.Index(D, max_k=16, device=0)
    ix.load(rows)
    sub = [0, 1, 15, 16, 17, 31, 32, 255, 256, 257, 511, 512, 767, 768, 998, 999]
    q = qs.copy()
    q[16] = rows[_tile0(95) + 64]      # (a sample tile)
    q[256] = rows[N_PART_SAMPLE - 1]   # (the last valid row of the partial sample tile)
    q[999] = rows[_tile0(96)]
    by16 = {}
    for k in (K, 1):
        parts = [ix.local_top_k(q[i:i + 16], k) for i in range(0, len(q), 16)]
        by16[k] = tuple(np.concatenate([p[j] for p in parts]) for j in range(3))
    want = _oracle(oracle_mod, rows, q[sub])
    yield ix, q, sub, want, by16
    ix.close()


@pytest.mark.parametrize("nq,k", [(17, K), (256, K), (257, K), (1000, K), (1000, 1)])
def test_batch_sizes(bsr_mod, batch_shard, nq, k):
    """The query-tile edges (17, 256, 257, 1000 queries) and k = 1; three searches of each shape,
    the third replaying the captured graph (the fix-up is one of its kernel nodes)."""
    ix, q, sub, want, by16 = batch_shard
    sub = [s for s in sub if s < nq]
    for rep in range(3):
        got = ix.local_top_k(q[:nq], k)
        st = ix.last_stats()
        _filtered(st, nq, f"nq={nq} k={k} rep={rep}")
        wi, wd, wc = want
        _same(got, (wi[:len(sub)], wd[:len(sub)], wc[:len(sub)]), sub, (nq, k, rep), k)
        for a, b in zip(got, by16[k]):
            a = a.view(np.uint32) if a.dtype == np.float32 else a
            b = b.view(np.uint32) if b.dtype == np.float32 else b
            assert np.array_equal(a, b[:nq]), (nq, k, rep)
    assert st.graph_replay == 1


# ---- planted answers inside sample tiles and beside them -------------------------------------
def _near(rng, q, m):
    return (q + 1e-3 * rng.standard_normal((m, D))).astype(np.float32)


def test_planted_answers(bsr_mod, oracle_mod, base):
    rows, qs = base
    n = N_PART_SAMPLE
    rows = rows[:n].copy()
    nq = 24
    q = qs[:nq].copy()
    rng = np.random.default_rng(7)
    assert _is_sample_tile(63) and _is_sample_tile(95) and _is_sample_tile((n - 1) // TILE)
    plants = {
        0: np.arange(_tile0(63) + 3, _tile0(63) + 13),        # the best 10 rows in one sample tile
        1: np.arange(_tile0(95) + 20, _tile0(95) + 60),       # 40 near-duplicates across a 32-row block edge
        2: np.array([n - 1]),                                 # the last valid row of the partial sample tile
        3: np.arange(_tile0(63) - 10, _tile0(63)),            # the 10 rows before a sample tile
        4: np.arange(_tile0(64), _tile0(64) + 10),            # the 10 rows after it
        5: np.arange(_tile0(96) + 20, _tile0(96) + 60),       # 40 near-duplicates in the tile after one
        6: np.arange(_tile0(127) - 20, _tile0(127) + 20),     # 40 across the edge into a sample tile
        7: np.arange(_tile0(128) - 20, _tile0(128) + 20),     # 40 across the edge out of it
    }
    for j, ids in plants.items():
        rows[ids] = _near(rng, q[j], len(ids))
    ix, got, st = _search(bsr_mod, rows, q)
    _filtered(st, nq, "planted")
    _same(got, _oracle(oracle_mod, rows, q), range(nq), "planted")
    for j, ids in plants.items():
        c = min(K, len(ids))
        assert set(got[0][j, :c].tolist()) <= set(ids.tolist()), (j, got[0][j], ids)
    ix.close()


# ---- ties at the threshold -------------------------------------------------------------------
def test_ties_at_the_threshold(bsr_mod, oracle_mod, gpu):
    """A small-integer corpus of period 8192 rows (64 tiles), 8.5 periods: sample tiles 31, 95, ...
    hold the same 128 rows with the same block scales (9 times), tiles 63, 127, ... likewise (8
    times), so every sample maximum occurs 8 or 9 times and tau0, the 8th best, IS a maximum that
    8 or more blocks reach exactly.  Per query the period holds two copies of the query outside the
    sample tiles (17 rows at distance 0 in the shard: the answer, in index order) and, in each of
    the two sample tiles, the query with its first 150 coordinates zeroed (score ~0.9, every other
    row ~0.1): tau0 is that row's score, and exactly the 17 copies above it and the 8, 9 or 17 rows
    AT it are emitted -- the latter by the fix-up, only if ties at the threshold pass (a certified
    answer cannot show a row at tau0, so the emitted count is what tells)."""
    rng = np.random.default_rng(99)
    period, nq = 8192, 24
    pool = rng.integers(-2, 3, (period, D)).astype(np.float32)
    q = rng.integers(-2, 3, (nq, D)).astype(np.float32)
    first = []
    for j in range(nq):
        p1, p2 = _tile0(10) + 1 + j, _tile0(40) + 33 + j      # (no multiple of 32 among them)
        pool[p1] = q[j]
        pool[p2] = q[j]
        near = q[j].copy()
        near[:150] = 0
        pool[_tile0(31) + 33 + j] = near
        pool[_tile0(63) + 65 + j] = near
        first.append(sorted([p1 + period * i for i in range(9)] + [p2 + period * i for i in range(8)])[:K])
    rows = np.tile(pool, (9, 1))[:N_FULL]
    ix, got, st = _search(bsr_mod, rows, q)
    _filtered(st, nq, "ties")
    _same(got, _oracle(oracle_mod, rows, q), range(nq), "ties")
    assert np.array_equal(got[0], np.array(first, np.uint64))
    assert np.all(got[1] == 0.0)
    assert nq * (17 + 8) <= st.n_emitted <= nq * (17 + 17), st.n_emitted
    ix.close()


# ---- masked search ---------------------------------------------------------------------------
def test_masked_search(bsr_mod, oracle_mod, gpu):
    """The masked filter path lowers the threshold to the ceil(8 n / A)-th best sample value, and
    its sample is compact -- the sample tiles are used -- only when n / 32 >= 256 times that, i.e.
    A / n >= 65536 / n: at 200,000 rows a mask must allow a third of the rows.  So: every row of
    every sample tile allowed (what the fix-up emits survives the cut), the answers planted in
    sample tiles, and random other rows up to A / n = 0.36."""
    rng = np.random.default_rng(5)
    n, nq = 200_000, 24
    rows = rng.uniform(-1, 1, (n, D)).astype(np.float32)
    q = rng.uniform(-1, 1, (nq, D)).astype(np.float32)
    tiles = np.arange(PHASE, (n + TILE - 1) // TILE // EVERY * EVERY, EVERY)
    in_sample = (np.arange(n) // TILE) % EVERY == PHASE
    in_sample &= np.arange(n) < (tiles[-1] + 1) * TILE
    mask = in_sample | (rng.random(n) < 0.34)
    for j in range(8):
        ids = _tile0(tiles[3 * j]) + 40 * (j % 3) + np.arange(12)
        rows[ids] = _near(rng, q[j], 12)
    ids = np.flatnonzero(mask)
    assert 0.34 < len(ids) / n < 0.40
    ix = bsr_mod.Index(D, max_k=16, device=0)
    ix.load(rows)
    got = ix.local_top_k(q, K, allow_mask=mask, mask_mode="filter")
    st = ix.last_stats()
    print(f"masked: fallback={st.n_fallback} exact_direct={st.n_exact_direct} emitted={st.n_emitted} "
          f"path={st.search_path}")
    assert st.search_path & bsr_mod.BSR_PATH_MASK_FILTER and not st.search_path & bsr_mod.BSR_PATH_MASK_LIST
    assert st.n_fallback == 0 and st.n_exact_direct == 0 and st.n_emitted >= nq
    wi, wd, wc = _oracle(oracle_mod, rows[ids], q)
    assert np.all(wc == K) and np.array_equal(got[2], wc)
    assert np.array_equal(got[0], ids[wi.astype(np.int64)].astype(np.uint64))
    assert np.array_equal(got[1].view(np.uint32), wd.view(np.uint32))
    ix.close()


# ---- the parallel search's global threshold --------------------------------------------------
@pytest.mark.parametrize("comm_kind", ["forced-one-rank", "loopback-2"])
def test_global_threshold(bsr_mod, oracle_mod, base, monkeypatch, comm_kind):
    """The fix-up reads the threshold at run time.  A rank's own sample keys are among the gathered
    ones, so the global threshold is never below its local tau0: a one-rank RCCL communicator with
    BSR_FORCE_COLLECTIVES=1 gives a global threshold EQUAL to the local one (every tie at tau0
    passes again), a replicating loopback communicator of two ranks one ABOVE it (the 8th best of
    two copies of the keys is the local 4th best, so sample blocks between the two no longer pass).
    Each query has 12 planted near-duplicates, some in sample tiles, so every merged list certifies."""
    rows, qs = base
    n, nq = N_FULL, 24
    rows = rows[:n].copy()
    q = qs[:nq].copy()
    rng = np.random.default_rng(3)
    for j in range(nq):
        t = 31 + 16 * j if j % 2 == 0 else 40 + 16 * j      # (even queries: a sample tile)
        assert _is_sample_tile(t) == (j % 2 == 0)
        rows[_tile0(t) + 26:_tile0(t) + 38] = _near(rng, q[j], 12)
    ix = bsr_mod.Index(D, max_k=16, device=0)
    ix.load(rows)
    if comm_kind == "forced-one-rank":
        monkeypatch.setenv("BSR_FORCE_COLLECTIVES", "1")
        comm = bsr_mod.Comm(bsr_mod.Comm.unique_id(), 0, 1, 0)
    else:
        comm = bsr_mod.Comm.loopback(0, 2, 0)
    want = _oracle(oracle_mod, rows, q)
    bits = bsr_mod.BSR_PATH_COLLECTIVE | bsr_mod.BSR_PATH_GLOBAL_TAU
    for rep in range(2):
        got = bsr_mod.parallel_top_k_similarity_search_batch(comm, ix, q, K)
        st = ix.last_stats()
        print(f"{comm_kind} rep={rep}: fallback={st.n_fallback} emitted={st.n_emitted} path={st.search_path}")
        assert st.search_path & bits == bits and not st.search_path & bsr_mod.BSR_PATH_FALLBACK, st.search_path
        assert st.n_fallback == 0 and st.n_exact_direct == 0 and st.n_emitted >= nq
        _same(got, want, range(nq), (comm_kind, rep))
    comm.close()
    ix.close()
