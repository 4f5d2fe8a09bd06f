"""Kernel-level checks of the id scoring (csrc/k_exact.hip): launch_score_ids and
launch_score_finish, each on its own through the test-only shim, against the models of
tests/kcheck_score.py -- bit for bit, every output garbage-filled before the launch."""
import numpy as np
import pytest

import kcheck_exact as kx
import kcheck_score as ks

pytestmark = pytest.mark.gpu

F = np.float32
KFILL = np.uint64(0x5A5A5A5A5A5A5A5A)
PAD = np.uint64(2 ** 64 - 1)
N, NQ = 600, 17
MS = (1, 63, 64, 65, 255, 256, 257, 700)
NQS = (1, 3, 17)
OFFSETS = (0, 2 ** 33 + 5)

_corpora = {}


def corpus(dim):
    """600 rows and 17 queries with the planted rows of kcheck_exact.Corpus, the model's distance of
    every row to every query (computed once per row length) and a fixed set of deleted rows."""
    if dim not in _corpora:
        c = kx.Corpus(N, dim, NQ, 2200 + dim)
        c.all_dist = [c.dist(q) for q in range(NQ)]
        c.dead = np.random.default_rng(dim).random(N) < 0.2
        c.dead[[c.ident[1], c.zero[1]]] = True
        c.dead[[c.ident[0], c.zero[0], c.near, c.neg, c.run, c.run + 1]] = False
        _corpora[dim] = c
    return _corpora[dim]


def make_lists(corp, rng, nq, m, offset):
    """ids [nq][m]: per query ceil(0.6 m) slots name live rows (drawn with replacement: repeats; the
    planted rows first), the others are the padding value, ids below the shard (with an offset), ids
    above it up to 2^64 - 2, and deleted rows -- shuffled.  At m = 1 every odd query's slot is absent."""
    live = np.flatnonzero(~corp.dead)
    gone = np.flatnonzero(corp.dead)
    special = [r for r in (corp.ident[0], corp.zero[0], corp.near, corp.neg, corp.run, corp.run + 1)]
    ids = np.empty((nq, m), np.uint64)
    for q in range(nq):
        n_pres = -(-6 * m // 10) if not (m == 1 and q % 2) else 0
        pres = np.concatenate([special, rng.choice(live, max(n_pres, 1))])[:n_pres]
        row = [np.uint64(offset + int(r)) for r in pres]
        kinds = rng.integers(0, 4, m - n_pres)
        for kind in kinds:
            if kind == 0:
                row.append(PAD)
            elif kind == 1:
                row.append(np.uint64(offset - 1 - int(rng.integers(0, 3))) if offset else np.uint64(2 ** 64 - 2))
            elif kind == 2:
                above = (offset + N, offset + N + int(rng.integers(1, 1 << 40)), 2 ** 64 - 2, 2 ** 63 + 17)
                row.append(np.uint64(above[int(rng.integers(0, 4))]))
            else:
                row.append(np.uint64(offset + int(rng.choice(gone))))
        row = np.array(row, np.uint64)
        rng.shuffle(row)
        ids[q] = row
    return ids


def launch(corp, ids, offset, dead=None, na=None, dist=True, keys=True, found=True):
    nq, m = ids.shape
    out = dict(dist=np.full((nq, m), np.nan, F) if dist else None,
               keys=np.full((nq, m), KFILL, np.uint64) if keys else None,
               kcnt=np.zeros(nq, np.uint32) if keys else None,
               found=np.zeros(nq, np.uint32) if found else None)
    rc = ks.score_raw(rows=corp.rows, ld=corp.ld, dim=corp.dim, n=N, offset=offset,
                      na=corp.na if na is None else na, qf32=corp.qf32[:nq].copy(), nb=corp.nb[:nq].copy(),
                      dead=ks.pack_dead(dead, corp.rows.shape[0] // 64) if dead is not None else None,
                      ids=np.ascontiguousarray(ids), m=m, nq=nq, **out)
    assert rc == 0
    return out


def check(corp, ids, offset, out, dead=None, all_dist=None):
    nq, m = ids.shape
    all_dist = corp.all_dist if all_dist is None else all_dist
    n_present = 0
    for q in range(nq):
        wd, wf, wk = ks.score_model(all_dist[q], ids[q], offset, dead)
        n_present += wf
        what = (corp.dim, offset, nq, m, q)
        if out["dist"] is not None:
            assert np.array_equal(out["dist"][q].view(np.uint32), wd.view(np.uint32)), what
        if out["found"] is not None:
            assert out["found"][q] == wf, what
        if out["keys"] is not None:
            assert out["kcnt"][q] == wf, what
            assert np.array_equal(np.sort(out["keys"][q, :wf]), wk), what
            assert (out["keys"][q, wf:] == KFILL).all(), what
    return n_present


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("dim", (768, 70, 1100))
def test_score_ids(gpu, dim, offset):
    assert ks.lib().kc_score_max_ids() == ks.SCORE_MAX_IDS == 4096
    corp = corpus(dim)
    rng = np.random.default_rng(dim + (offset & 0xFFFF))
    for m in MS:
        for nq in NQS:
            ids = make_lists(corp, rng, nq, m, offset)
            for dead in (None, corp.dead):
                out = launch(corp, ids, offset, dead)
                n_present = check(corp, ids, offset, out, dead)
                assert 2 * n_present >= nq * m, (dim, offset, nq, m, n_present)
    # a query equal to stored rows, zero rows, the negated row: 0 and 1 by the reference's rules
    ids = np.array([[offset + r for r in corp.ident + corp.zero + [corp.neg, corp.near]]] * 2, np.uint64)
    out = launch(corp, ids, offset)
    check(corp, ids, offset, out)
    assert (out["dist"][0, :3] == 0).all() and (out["dist"][:, 3:5] == 1).all() and out["dist"][1, 5] > 1.99


@pytest.mark.parametrize("dim", (768, 70, 1100))
def test_score_ids_single_sinks_and_stored_norms(gpu, dim):
    corp = corpus(dim)
    offset = OFFSETS[1]
    rng = np.random.default_rng(77 + dim)
    ids = make_lists(corp, rng, 3, 257, offset)
    for sinks in (dict(keys=False, found=False), dict(dist=False, found=False), dict(dist=False), dict(keys=False)):
        out = launch(corp, ids, offset, corp.dead, **sinks)
        assert 2 * check(corp, ids, offset, out, corp.dead) >= ids.size
    # one stored magnitude doubled: exactly that row's slots change, to the model's value with the
    # doubled magnitude -- na is read, not recomputed from the row.  (An ordinary live row: the
    # identical and the zero rows score 0 and 1 whatever their magnitude.)
    fixed = set(corp.ident + corp.zero + [corp.near])
    r = next(g - offset for g in ids[0].tolist()
             if offset <= g < offset + N and g - offset not in fixed and not corp.dead[g - offset])
    ids[1, 5] = ids[2, 200] = np.uint64(offset + r)
    full = launch(corp, ids, offset, corp.dead)
    na2 = corp.na.copy()
    na2[r] *= F(2)
    out = launch(corp, ids, offset, corp.dead, na=na2)
    check(corp, ids, offset, out, corp.dead, all_dist=[corp.dist(q, na=na2) for q in range(3)])
    changed = out["dist"].view(np.uint32) != full["dist"].view(np.uint32)
    assert np.array_equal(changed, ids == np.uint64(offset + r)) and changed.sum() >= 3


def test_score_ids_refusals(gpu):
    corp = corpus(70)
    ids = np.zeros((1, 4), np.uint64)
    base = dict(rows=corp.rows, ld=corp.ld, dim=corp.dim, n=N, offset=0, na=corp.na, qf32=corp.qf32[:1].copy(),
                nb=corp.nb[:1].copy(), ids=ids, nq=1)
    d, k, c = np.zeros((1, 4), F), np.zeros((1, 4), np.uint64), np.zeros(1, np.uint32)
    assert ks.score_raw(m=0, dist=d, **base) == 1
    assert ks.score_raw(m=4, **base) == 1, "no sink"
    assert ks.score_raw(m=4, keys=k, **base) == 1, "keys without their counter"
    assert ks.score_raw(m=4, keys=k, kcnt=c, **base) == 0


# ----------------------------------------------------------------------------------------
# launch_score_finish
# ----------------------------------------------------------------------------------------
def check_finish(keys, kcnt, k, offset):
    rc, idx, dist, cnt = ks.score_finish(keys, kcnt, k, offset)
    assert rc == 0
    for q in range(len(kcnt)):
        wi, wd, wc = ks.finish_model(keys[q], int(kcnt[q]), k, offset)
        what = (keys.shape, k, q, int(kcnt[q]))
        assert cnt[q] == wc, what
        assert np.array_equal(idx[q], wi), what
        assert np.array_equal(dist[q].view(np.uint32), wd.view(np.uint32)), what
    return cnt


@pytest.mark.parametrize("m", (1, 65, 700, 4096))
def test_score_finish(gpu, m):
    rng = np.random.default_rng(m)
    offset = 10 ** 10 + 7
    counts = sorted({0, 1, min(m, 63), min(m, 64), min(m, 65), m // 2, max(m - 1, 0), m})
    for dup in (False, True):
        keys = np.full((len(counts) + 2, m), KFILL, np.uint64)
        for q, c in enumerate(counts):
            d = rng.choice(F([0.0, 0.25, 0.5, 2.0]), c) if dup else rng.uniform(0, 2, c).astype(F)
            # dup: few distinct distances and rows drawn with replacement -- ties and equal keys
            rows = rng.integers(0, max(c // 2, 1), c) if dup else rng.choice(1 << 24, c, replace=False)
            keys[q, :c] = kx.dist_key(d, rows.astype(np.uint64))
        # m distinct keys in descending order, and m equal keys
        keys[-2] = kx.dist_key(np.linspace(2, 0, m).astype(F), np.arange(m, dtype=np.uint64))
        keys[-1] = kx.dist_key(F(0.375), np.uint64(41))
        kcnt = np.array(counts + [m, m], np.uint32)
        for k in sorted({1, max(m // 2, 1), m}):
            cnt = check_finish(keys, kcnt, k, offset)
            assert cnt[-2] == k and cnt[-1] == 1
    assert m < 4096 or len(np.unique(keys[-2])) == 4096


def test_score_finish_refusals(gpu):
    keys = np.zeros((1, 8), np.uint64)
    one = np.ones(1, np.uint32)
    assert ks.score_finish(keys, one, 0, 0)[0] == 1
    assert ks.score_finish(keys, one, 9, 0)[0] == 1
    assert ks.score_finish(np.zeros((1, 4097), np.uint64), one, 1, 0)[0] == 1
    assert ks.score_finish(keys, one, 8, 0)[0] == 0
