"""Kernel-level checks of the range search (csrc/k_exact.hip): launch_range_tau,
launch_range_rescore, launch_range_scan and launch_range_finish, each on its own through the
test-only shim, against the models of tests/kcheck_range.py -- bit for bit."""
import numpy as np
import pytest

import kcheck as kc
import kcheck_exact as kx
import kcheck_range as kr
from kcheck_exact import KEY_NONE, NEG_INF, POS_INF

pytestmark = pytest.mark.gpu

F = np.float32
KFILL = np.uint64(0x5A5A5A5A5A5A5A5A)
FILL = 0xA5A5A5A5


def ulps_up(x, k):
    for _ in range(k):
        x = np.nextafter(F(x), POS_INF)
    return F(x)


def test_constants(gpu):
    c = kr.consts()
    assert c.scan_qf == 8 and c.max_results == kr.RANGE_MAX_RESULTS == 4096
    assert c.query_no_approx == 2 and c.nan_radius == 0x100
    for cap in (1, 64, 512, 513, 1000, 2048, 4095, 4096):
        assert kr.range_cap(cap) == kr.range_cap_model(cap), cap


# ----------------------------------------------------------------------------------------
# launch_range_tau
# ----------------------------------------------------------------------------------------
def tau_grid():
    rs = (-1.0, 0.0, 1e-7, 0.1, 0.999, 1.0, 2.0, np.inf)
    es = (0.0, 0.01, 0.999, 1.0)
    nbs = (1.0, 1e-6)
    g = np.array([(r, e, b) for r in rs for e in es for b in nbs], F)
    radius, ebound, nb = g[:, 0].copy(), g[:, 1].copy(), g[:, 2].copy()
    flags = np.zeros(len(g), np.uint32)
    # a few more: the filter cannot serve the query (flag; a NaN bound), radii next to each other
    extra = [(0.1, 0.01, 1.0, 2), (-0.5, 0.01, 1.0, 2), (0.1, np.nan, 1.0, 0), (0.25, 0.004, 27.7, 0),
             (np.nextafter(F(0.25), POS_INF), 0.004, 27.7, 0), (0.05, 0.0078, 16.0, 1)]
    for r, e, b, f in extra:
        radius, ebound, nb, flags = (np.append(radius, F(r)), np.append(ebound, F(e)), np.append(nb, F(b)),
                                     np.append(flags, np.uint32(f)))
    return radius.astype(F), ebound.astype(F), nb.astype(F), flags.astype(np.uint32)


@pytest.mark.parametrize("with_nan", [False, True])
def test_range_tau(gpu, with_nan):
    c = kr.consts()
    radius, ebound, nb, flags = tau_grid()
    if with_nan:
        radius[5] = np.nan
    nq, qpad = len(radius), 256
    out = kr.range_tau(radius, ebound, nb, flags, qpad, fill=FILL)
    tau, st = out["tau"], out["status"]
    want_tau, want_scan, want_nan = kr.range_tau_model(radius, ebound, nb, flags, c.query_no_approx)
    assert want_nan == with_nan
    n_filtered = 0
    for q in range(nq):
        what = (q, radius[q], ebound[q], nb[q], flags[q], tau[q], want_tau[q])
        if not (want_tau[q] < POS_INF):
            assert tau[q] == POS_INF, what
            continue
        n_filtered += 1
        assert 0 < tau[q] < POS_INF, what
        # safety (mandatory): every row the filter leaves out at tau lies outside the radius
        assert kx.exclusion_bound(tau[q], ebound[q], nb[q]) > radius[q], what
        # tightness: four ulps further the bound no longer clears the radius
        assert not (kx.exclusion_bound(ulps_up(tau[q], 4), ebound[q], nb[q]) > radius[q]), what
    assert n_filtered >= 16
    print(f"tau: {n_filtered} filtered queries, {int((tau[:nq] != want_tau).sum())} differ from the model's bits")
    assert np.isposinf(tau[nq:]).all(), "padding queries emit nothing"
    n_scan = int(want_scan.sum())
    assert st[c.st_fail] == n_scan and st[c.st_fail2] == n_scan and st[c.st_emitted] == 0
    assert st[c.st_query_flags] == (c.nan_radius if with_nan else 0)
    lst = out["scan_list"]
    assert sorted(lst[:n_scan]) == list(np.flatnonzero(want_scan)), "the scan list is exactly the model's set"
    assert (lst[n_scan:] == FILL).all()
    assert not out["cnt"].any(), "cnt[0 .. qpad), the tail counters and the gang words are zeroed"
    assert len(out["cnt"]) == qpad + c.tail_words and c.tail_words == 8 * 64 + 512
    assert not out["rcnt"].any()


# ----------------------------------------------------------------------------------------
# launch_range_rescore
# ----------------------------------------------------------------------------------------
CAP = 1024


@pytest.mark.parametrize("dim", (64, 130, 768, 1100))
def test_range_rescore(gpu, dim):
    c = kr.consts()
    corp = kx.Corpus(1500, dim, 4, 900 + dim)
    rng = np.random.default_rng(dim)
    n = corp.n
    special = corp.ident + [corp.near] + corp.zero + [corp.neg] + list(range(corp.run, corp.run + 20))
    others = np.setdiff1d(np.arange(n), special)
    short = np.concatenate([special, rng.choice(others, 300, replace=False)])
    rng.shuffle(short)
    full = rng.permutation(n)[:CAP]
    over = rng.permutation(n)[:CAP]  # (its count says cap + 1: the list itself is never read)
    planted = int(short[np.isin(short, others)][17])  # (an ordinary row of the list)
    d_planted = corp.dist(0, [planted])[0]
    assert d_planted > 0
    d_full = corp.dist(2, full)
    # slot: (query, list, radius, listed count)
    slots = [(0, short, d_planted, len(short)),                                # the planted row: included
             (0, short, np.nextafter(d_planted, NEG_INF), len(short)),         # one f32 below: excluded
             (0, short, F(0), len(short)),                                     # identical rows: distance 0
             (1, short, F(1), len(short)),                                     # zero rows: distance 1
             (2, full, np.sort(d_full)[CAP // 2], CAP),                        # a list of exactly cap keys
             (3, over, F(2), CAP + 1),                                         # cap + 1: the scan's
             (1, short[:1], F(2), 1), (1, short, F(-1), 0)]                    # one key; an empty list
    nq = len(slots)
    qsel = [s[0] for s in slots]
    qf32, nb = corp.qf32[qsel].copy(), corp.nb[qsel].copy()
    radius = np.array([s[2] for s in slots], F)
    cand = np.full((nq, CAP), KEY_NONE, np.uint64)
    cnt = np.zeros(nq, np.uint32)
    for i, (_, lst, _, m) in enumerate(slots):
        cand[i, :len(lst)] = kc.score_key(rng.uniform(0, 1, len(lst)).astype(F), lst.astype(np.uint32))
        cnt[i] = m
    dead = np.zeros(n, bool)
    dead[[corp.ident[0], corp.zero[0], int(short[40]), int(full[3])]] = True
    for na, dead_on, tag in ((corp.na, False, "plain"), (corp.na, True, "dead"), (corp.na * F(2), False, "2na")):
        keys = np.full((nq, CAP), KFILL, np.uint64)
        rcnt = np.full(nq, FILL, np.uint32)
        lst_out = np.full(nq + 5, FILL, np.uint32)
        st = np.full(c.st_words, 0, np.uint32)
        st[c.st_fail] = 5  # (the threshold kernel listed five queries before)
        st[c.st_fail2] = 5
        rc = kr.range_raw(0, rows=corp.rows, ld=corp.ld, dim=corp.dim, n=n, na=na, qf32=qf32, nb=nb, radius=radius,
                          dead=kr.pack_dead(dead, corp.rows.shape[0] // 64) if dead_on else None, keys=keys, rcnt=rcnt,
                          cap=CAP, nq=nq, cand=cand, cnt=cnt, scan_list=lst_out, status=st)
        assert rc == 0
        for i, (qi, lst, r, m) in enumerate(slots):
            if m > CAP:
                assert rcnt[i] == FILL and (keys[i] == KFILL).all(), "an overflowed query writes nothing"
                continue
            rows = np.asarray(lst[:m], np.int64)
            want = kr.in_range_keys(corp.dist(qi, rows, na=na), rows, r, dead if dead_on else None)
            assert rcnt[i] == len(want), (tag, i, rcnt[i], len(want))
            assert np.array_equal(np.sort(keys[i, :len(want)]), want), (tag, i)
            assert (keys[i, len(want):] == KFILL).all(), (tag, i)
        assert st[c.st_fail] == 6 and lst_out[5] == 5 and (lst_out[:5] == FILL).all() and (lst_out[6:] == FILL).all()
        assert st[c.st_fail2] == 5 and st[c.st_emitted] == int(cnt.sum())
        if tag == "plain":
            k0 = set(kx.key_row(keys[0, :rcnt[0]]).tolist())
            k1 = set(kx.key_row(keys[1, :rcnt[1]]).tolist())
            assert planted in k0 and planted not in k1, "the radius is inclusive, to the bit"
            z = keys[2, :rcnt[2]]
            assert set(kx.key_row(z).tolist()) >= set(corp.ident) and (kx.key_dist(z) == 0).all()
            d3 = dict(zip(kx.key_row(keys[3, :rcnt[3]]).tolist(), kx.key_dist(keys[3, :rcnt[3]]).tolist()))
            assert all(d3[r] == 1.0 for r in corp.zero)
            assert rcnt[6] == 1 and rcnt[7] == 0 and 0 < rcnt[4] < CAP
        if tag == "dead":
            assert corp.ident[0] not in set(kx.key_row(keys[2, :rcnt[2]]).tolist())
        if tag == "2na":
            # (doubled magnitudes halve every cosine: the stored na is read, not recomputed)
            plain = kr.in_range_keys(corp.dist(0, np.asarray(short, np.int64)), short, d_planted)
            assert rcnt[0] != len(plain)


# ----------------------------------------------------------------------------------------
# launch_range_scan
# ----------------------------------------------------------------------------------------
_corpora = {}


def scan_corpus(dim):
    if dim not in _corpora:
        c = kx.Corpus(1000, dim, 12, 700 + dim)
        c.all_dist = [c.dist(q) for q in range(c.nq)]
        _corpora[dim] = c
    return _corpora[dim]


@pytest.mark.parametrize("dim", (130, 768))
@pytest.mark.parametrize("nqf", (1, 3, 8))
def test_range_scan(gpu, dim, nqf):
    corp = scan_corpus(dim)
    rng = np.random.default_rng(dim + nqf)
    cap = 256
    qf = 1 if nqf <= 1 else 2 if nqf <= 2 else 4 if nqf <= 4 else 8
    ids = [int(x) for x in rng.permutation(corp.nq)[:nqf]]
    qids = np.array(ids + [ids[-1]] * (qf - nqf), np.int32)
    for n in (1, 255, 256, 257, 1000):
        # radii: the first query takes every row (at n = 1000 its count exceeds cap), the others a
        # quantile of their own distances, planted at a row's exact distance
        radius = np.full(corp.nq, np.nan, F)
        for j, q in enumerate(ids):
            radius[q] = POS_INF if j == 0 else np.sort(corp.all_dist[q][:n])[min(n - 1, (j * n) // 40)]
        dead = rng.random(corp.n) < 0.3
        dead[corp.ident[1]] = True
        for dead_on in (False, True):
            for grid in sorted({kx.scan_grid_for(n), 3}):
                keys = np.full((corp.nq, cap), KFILL, np.uint64)
                rcnt = np.full(corp.nq, FILL, np.uint32)
                rcnt[ids] = 0
                rc = kr.range_raw(1, rows=corp.rows, ld=corp.ld, dim=corp.dim, n=n, na=corp.na, qf32=corp.qf32,
                                  nb=corp.nb, radius=radius,
                                  dead=kr.pack_dead(dead, corp.rows.shape[0] // 64) if dead_on else None,
                                  keys=keys, rcnt=rcnt, cap=cap, nq=corp.nq, qids=qids, nqf=nqf, grid=grid)
                assert rc == 0
                for q in range(corp.nq):
                    what = (n, dead_on, grid, q)
                    if q not in ids:
                        assert rcnt[q] == FILL and (keys[q] == KFILL).all(), what
                        continue
                    want = kr.in_range_keys(corp.all_dist[q][:n], np.arange(n), radius[q], dead if dead_on else None)
                    assert rcnt[q] == len(want), what + (rcnt[q], len(want))
                    if len(want) <= cap:
                        assert np.array_equal(np.sort(keys[q, :len(want)]), want), what
                        assert (keys[q, len(want):] == KFILL).all(), what
                    else:
                        got = keys[q]
                        assert len(set(got.tolist())) == cap and np.isin(got, want).all(), what
                if n == 1000 and not dead_on:
                    assert rcnt[ids[0]] == 1000 > cap


def test_range_scan_refusals(gpu):
    corp = scan_corpus(130)
    base = dict(rows=corp.rows, ld=corp.ld, dim=corp.dim, n=10, na=corp.na, qf32=corp.qf32, nb=corp.nb,
                radius=np.zeros(corp.nq, F), keys=np.zeros((corp.nq, 64), np.uint64),
                rcnt=np.zeros(corp.nq, np.uint32), cap=64, nq=corp.nq, qids=np.zeros(16, np.int32))
    assert kr.range_raw(1, nqf=0, grid=1, **base) == 1
    assert kr.range_raw(1, nqf=9, grid=1, **base) == 1
    assert kr.range_raw(1, nqf=1, grid=0, **base) == 1


# ----------------------------------------------------------------------------------------
# launch_range_finish
# ----------------------------------------------------------------------------------------
def finish_lists(rng, counts, cap, dup=False):
    """keys [len(counts)][cap]: list q holds min(counts[q], cap) distinct keys in random order (dup:
    only four distinct distances, so the row decides), garbage behind them."""
    keys = np.full((len(counts), cap), KFILL, np.uint64)
    for q, m in enumerate(counts):
        m = min(m, cap)
        d = rng.choice(F([0.0, 0.25, 0.5, 2.0]), m) if dup else rng.uniform(0, 2, m).astype(F)
        rows = rng.choice(1 << 24, m, replace=False).astype(np.uint64)
        keys[q, :m] = kx.dist_key(d, rows)
    return keys


@pytest.mark.parametrize("capacity, cap, counts", [
    (100, 1024, (0, 1, 63, 64, 65, 99, 100, 101, 1024, 3000)),
    (64, 1024, (64, 65, 2, 33)),
    (1, 1024, (0, 1, 2)),
    (4096, 8192, (4096, 4097, 2049, 2048, 129, 100000)),
])
@pytest.mark.parametrize("dup", [False, True])
def test_range_finish(gpu, capacity, cap, counts, dup):
    rng = np.random.default_rng(capacity + dup)
    keys = finish_lists(rng, counts, cap, dup)
    rcnt = np.array(counts, np.uint32)
    offset = 10 ** 10 + 7
    rc, idx, dist, cnt = kr.range_finish(keys, rcnt, capacity, offset)
    assert rc == 0
    for q, m in enumerate(counts):
        wi, wd, wc = kr.finish_model(keys[q], m, capacity, offset)
        assert cnt[q] == wc == m, (q, m)
        assert np.array_equal(idx[q], wi), (q, m)
        assert np.array_equal(dist[q].view(np.uint32), wd.view(np.uint32)), (q, m)
        if m <= capacity:
            order = kx.dist_key(dist[q, :m], idx[q, :m] - np.uint64(offset))
            assert (np.diff(order.astype(object)) > 0).all(), "ascending (distance, index), no duplicates"


def test_range_finish_refusals(gpu):
    keys = np.zeros((1, 1024), np.uint64)
    for capacity, cap in ((0, 1024), (4097, 8192), (2048, 1024)):
        k = np.zeros((1, cap), np.uint64)
        assert kr.range_finish(k, np.zeros(1, np.uint32), capacity, 0)[0] == 1, (capacity, cap)
    assert kr.range_finish(keys, np.zeros(1, np.uint32), 1024, 0)[0] == 0
