"""Kernel-level checks of the masked range search: launch_range_scan_list_groups and
launch_range_route (csrc/k_exact.hip) and launch_mask_groups_scatter_seg (csrc/k_prep.hip), each on
its own through the test-only shim, against the models of tests/kcheck_range_list.py and
tests/kcheck_range.py -- bit for bit."""
import numpy as np
import pytest

import kcheck_exact as kx
import kcheck_range as kr
import kcheck_range_list as kl
from kcheck_exact import POS_INF

pytestmark = pytest.mark.gpu

F = np.float32
KFILL = np.uint64(0x5A5A5A5A5A5A5A5A)
FILL = 0xA5A5A5A5
CAP = 256
NQ = 26  # queries of a corpus: three groups of up to eight distinct ids, and two no group names

_corpora = {}


def corpus(dim):
    if dim not in _corpora:
        c = kx.Corpus(1000, dim, NQ, 4100 + dim)
        c.all_dist = [c.dist(q) for q in range(c.nq)]
        _corpora[dim] = c
    return _corpora[dim]


def make_lists(corp, rng, lengths):
    """One ascending row list per length, each holding the planted rows it has room for (rows
    identical to query 0, zero rows), concatenated: (list, offsets)."""
    special = np.array(corp.ident + corp.zero + [corp.near, corp.neg])
    lists = []
    for m in lengths:
        keep = special[:min(len(special), m // 2)]
        rest = rng.choice(np.setdiff1d(np.arange(corp.n), keep), m - len(keep), replace=False)
        lists.append(np.sort(np.concatenate([keep, rest])).astype(np.uint32))
    offs = np.concatenate([[0], np.cumsum([len(x) for x in lists])[:-1]])
    return np.concatenate(lists), offs, lists


def group_setup(corp, rng, lists, qf, nqs):
    """Group y: ids[y * qf ..], the first nqs[y] its own (distinct over the launch; query 0 the
    second of the first group that has two), the rest padding with the group's first id; a radius
    per own query."""
    free = [int(x) for x in rng.permutation(np.arange(1, corp.nq - 2))]
    ids = np.zeros((len(lists), qf), np.int32)
    radius = np.full(corp.nq, np.nan, F)  # (a query no group names is never read)
    own = []
    placed0 = False
    for y, (lst, nqg) in enumerate(zip(lists, nqs)):
        mine = [free.pop(0) for _ in range(nqg)]
        if nqg >= 2 and not placed0:
            mine[1], placed0 = 0, True
        ids[y] = mine + [mine[0]] * (qf - nqg)
        for j, q in enumerate(mine):
            d = np.sort(corp.all_dist[q][lst])
            # every listed row; an identical row's distance 0 (query 0) or a zero row's distance 1; a
            # quantile of the list planted at a row's exact distance
            radius[q] = (POS_INF, F(0) if q == 0 else F(1), d[(j * len(d)) // 9])[min(j, 2)]
        own.append(mine)
    return ids, radius, own


def check_lists(corp, lists, own, radius, keys, rcnt, ctx):
    named = set()
    for lst, mine in zip(lists, own):
        for q in mine:
            named.add(q)
            want = kr.in_range_keys(corp.all_dist[q][lst], lst, radius[q])
            assert rcnt[q] == len(want), ctx + (q, int(rcnt[q]), len(want))
            if len(want) <= CAP:
                assert np.array_equal(np.sort(keys[q, :len(want)]), want), ctx + (q,)
                assert (keys[q, len(want):] == KFILL).all(), ctx + (q, "written past the count")
            else:  # the count runs on, the keys stop at cap: cap distinct keys of the answer
                assert len(set(keys[q].tolist())) == CAP and np.isin(keys[q], want).all(), ctx + (q,)
    for q in range(corp.nq):
        if q not in named:
            assert rcnt[q] == FILL and (keys[q] == KFILL).all(), ctx + (q, "a query no group names was written")
    return named


def launch(corp, lst, grp, qids, qf, radius, keys, rcnt, grid):
    return kl.scan_list_raw(rows=corp.rows, ld=corp.ld, dim=corp.dim, na=corp.na, qf32=corp.qf32, nb=corp.nb,
                            radius=radius, list=lst, grp=grp, groups=len(grp), qf=qf, qids=qids.reshape(-1).copy(),
                            keys=keys, rcnt=rcnt, cap=CAP, grid=grid)


@pytest.mark.parametrize("dim", (64, 130, 768))
@pytest.mark.parametrize("qf", (1, 2, 4, 8))
def test_range_scan_list_groups(gpu, dim, qf):
    """Three groups of different list lengths in one launch, grp.nq below the width, grids narrower
    and wider than a group's tile count."""
    corp = corpus(dim)
    assert (corp.ld, corp.dim) == ({64: 64, 130: 192, 768: 768}[dim], dim)
    rng = np.random.default_rng(dim + qf)
    for lengths, nqs in (((513, 1, 256), (qf, max(1, qf - 1), max(1, qf // 2 + (qf > 2)))),
                         ((255, 257, 513), (max(1, qf // 2 + (qf > 2)), qf, max(1, qf - 1)))):
        lst, offs, lists = make_lists(corp, rng, lengths)
        ids, radius, own = group_setup(corp, rng, lists, qf, nqs)
        grp = np.zeros(3, kx.GROUP_DESC)
        grp["off"], grp["n_list"], grp["nq"] = offs, lengths, nqs
        for grid in sorted({kx.scan_grid_for(max(lengths)), 2, 5}):
            keys = np.full((corp.nq, CAP), KFILL, np.uint64)
            rcnt = np.full(corp.nq, FILL, np.uint32)
            rcnt[[q for mine in own for q in mine]] = 0
            assert launch(corp, lst, grp, ids, qf, radius, keys, rcnt, grid) == 0
            named = check_lists(corp, lists, own, radius, keys, rcnt, (dim, qf, lengths, grid))
            # the first query of a 513-row list takes every row: its count runs past cap
            q_all = own[lengths.index(513)][0]
            assert rcnt[q_all] == 513 > CAP and q_all in named
            if 0 in named:  # the rows identical to query 0, found through the shortcut at distance 0
                lst0 = lists[[0 in mine for mine in own].index(True)]
                want0 = sorted(set(corp.ident) & set(lst0.tolist()))
                if radius[0] == 0:  # (the row 2e-10 off query 0 may round to distance 0 as well)
                    got0 = keys[0, :rcnt[0]]
                    assert len(want0) >= 1 and set(want0) <= set(kx.key_row(got0).tolist()) <= set(want0 + [corp.near])
                    assert (kx.key_dist(got0) == 0).all()


@pytest.mark.parametrize("dim", (130, 768))
def test_a_list_split_over_two_launches_accumulates(gpu, dim):
    corp = corpus(dim)
    rng = np.random.default_rng(7 + dim)
    qf, nqg = 4, 3
    lst, _, lists = make_lists(corp, rng, (513,))
    ids, radius, own = group_setup(corp, rng, lists, qf, (nqg,))
    radius[own[0][0]] = np.sort(corp.all_dist[own[0][0]][lst])[199]  # 200 rows <= cap, from both halves
    keys = np.full((corp.nq, CAP), KFILL, np.uint64)
    rcnt = np.full(corp.nq, FILL, np.uint32)
    rcnt[own[0]] = 0
    for lo, hi in ((0, 300), (300, 513)):
        grp = np.zeros(1, kx.GROUP_DESC)
        grp["off"], grp["n_list"], grp["nq"] = lo, hi - lo, nqg
        assert launch(corp, lst, grp, ids, qf, radius, keys, rcnt, kx.scan_grid_for(hi - lo)) == 0
    check_lists(corp, lists, own, radius, keys, rcnt, (dim, "split"))
    q = own[0][0]
    got = kx.key_row(keys[q, :rcnt[q]])
    assert rcnt[q] >= 200 and (np.isin(got, lst[:300])).any() and (np.isin(got, lst[300:])).any()


def test_zero_magnitude_rows_and_stored_norms(gpu):
    """na is read, never recomputed: a row whose stored magnitude is 0 lies at distance 1 whatever it holds."""
    corp = corpus(130)
    lst = np.arange(0, 300, dtype=np.uint32)
    na = corp.na.copy()
    zeroed = [20, 21, 299]
    na[zeroed] = 0
    q = 3
    radius = np.full(corp.nq, np.nan, F)
    d = kx.exact_distance(corp.a[lst], corp.q[q], na[lst], corp.nb[q])
    assert (d[zeroed] == 1).all()
    radius[q] = F(1)
    grp = np.zeros(1, kx.GROUP_DESC)
    grp["off"], grp["n_list"], grp["nq"] = 0, len(lst), 1
    keys = np.full((corp.nq, 512), KFILL, np.uint64)
    rcnt = np.zeros(corp.nq, np.uint32)
    rc = kl.scan_list_raw(rows=corp.rows, ld=corp.ld, dim=corp.dim, na=na, qf32=corp.qf32, nb=corp.nb, radius=radius,
                          list=lst, grp=grp, groups=1, qf=1, qids=np.array([q], np.int32), keys=keys, rcnt=rcnt,
                          cap=512, grid=2)
    assert rc == 0
    want = kr.in_range_keys(d, lst, F(1))
    assert rcnt[q] == len(want) and np.array_equal(np.sort(keys[q, :len(want)]), want)
    assert set(zeroed + corp.zero[:1]) <= set(kx.key_row(want).tolist())


def test_range_scan_list_refusals(gpu):
    corp = corpus(64)
    grp = np.zeros(1, kx.GROUP_DESC)
    grp["n_list"], grp["nq"] = 4, 1
    base = dict(rows=corp.rows, ld=corp.ld, dim=corp.dim, na=corp.na, qf32=corp.qf32, nb=corp.nb,
                radius=np.zeros(corp.nq, F), list=np.arange(4, dtype=np.uint32), grp=grp,
                qids=np.zeros(8, np.int32), keys=np.zeros((corp.nq, 64), np.uint64), rcnt=np.zeros(corp.nq, np.uint32))
    assert kl.scan_list_raw(groups=0, qf=1, cap=64, grid=1, **base) == 1
    assert kl.scan_list_raw(groups=1, qf=3, cap=64, grid=1, **base) == 1
    assert kl.scan_list_raw(groups=1, qf=1, cap=64, grid=0, **base) == 1
    assert kl.scan_list_raw(groups=1, qf=1, cap=0, grid=1, **base) == 1
    assert kl.scan_list_raw(groups=1, qf=1, cap=64, grid=1, **base) == 0


# ----------------------------------------------------------------------------------------
# launch_range_route
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["none", "some", "all"])
def test_range_route(gpu, which):
    c = kr.consts()
    rng = np.random.default_rng(11)
    # launch_range_tau's own grid of cases: filtered queries, unfilterable ones, radius < 0, a NaN
    rs = (-1.0, 0.0, 1e-7, 0.1, 0.999, 1.0, 2.0, np.inf, np.nan)
    g = np.array([(r, e, f) for r in rs for e in (0.0, 0.01, 1.0) for f in (0, 2) for _ in range(45)], F)
    nq = len(g)
    assert nq > 1024, "more queries than the workgroup has threads"
    radius, ebound, flags = g[:, 0].copy(), g[:, 1].copy(), g[:, 2].astype(np.uint32)
    nb = np.ones(nq, F)
    before = kr.range_tau(radius, ebound, nb, flags, 2560, fill=FILL)
    n0 = int(before["status"][c.st_fail])
    listed0 = set(before["scan_list"][:n0].tolist())
    assert 0 < n0 < nq and before["status"][c.st_fail2] == n0
    assert np.isfinite(before["tau"][:nq]).any()
    to_list = {"none": np.zeros(nq, np.uint32), "all": np.ones(nq, np.uint32),
               "some": (rng.random(nq) < 0.5).astype(np.uint32) * 7}[which]
    tau = before["tau"][:nq].copy()
    lst = np.full(nq + 3, FILL, np.uint32)
    lst[:n0] = before["scan_list"][:n0]
    st = before["status"].copy()
    assert kl.route(to_list, radius, tau, lst, st) == 0
    w_tau, w_set, w_fail, w_fail2 = kl.route_model(to_list, radius, before["tau"][:nq], listed0, n0)
    assert np.array_equal(tau.view(np.uint32), w_tau.view(np.uint32))
    assert st[c.st_fail] == w_fail and st[c.st_fail2] == w_fail2
    assert st[c.st_emitted] == before["status"][c.st_emitted] and st[c.st_query_flags] == before["status"][c.st_query_flags]
    got = lst[:w_fail].tolist()
    assert len(set(got)) == len(got) == len(w_set) and set(got) == w_set, "every query on the list exactly once"
    assert np.array_equal(lst[:n0], before["scan_list"][:n0]) and (lst[w_fail:] == FILL).all()
    on = np.zeros(nq, bool)
    on[got] = True
    with np.errstate(invalid="ignore"):
        assert not on[np.isnan(radius) | (radius < 0)].any(), "radius < 0 and NaN stay off the list"
        if which == "all":
            assert on[radius >= 0].all() and np.isposinf(tau).all()
    if which == "none":
        assert w_fail == n0


# ----------------------------------------------------------------------------------------
# launch_mask_groups_scatter_seg
# ----------------------------------------------------------------------------------------
def test_mask_scatter_segments(gpu):
    rng = np.random.default_rng(5)
    n = 40003  # 626 words: three blocks of 256 words, the last one partial
    masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 1 / 16, np.ones(n, bool), np.zeros(n, bool)])
    dead = rng.random(n) < 0.1
    words = (n + 63) // 64
    allow = np.stack([kr.pack_dead(m, words) for m in masks])
    allow[:, -1] |= np.uint64(0xFFFFFFFF) << np.uint64(32)  # (bits at positions >= n are ignored)
    A = [int((m & ~dead).sum()) for m in masks]
    # mask 0 in three segments at odd boundaries, mask 1 whole, a middle piece of mask 2, one id, an
    # empty segment, a segment that asks for more ids than the mask has left
    pieces = [(0, 0, 1000), (0, 1000, 16001 - 1000), (0, 16001, A[0] - 16001), (1, 0, A[1]), (2, 12345, 3000),
              (2, A[2] - 1, 1), (1, 5, 0), (1, A[1] - 10, 25)]
    segs = np.zeros(len(pieces), kl.SEG_DESC)
    off = 3
    for i, (g, first, m) in enumerate(pieces):
        segs[i] = (off, g, first, m, 0)
        off += m + 2  # (a gap between the segments shows a write past a segment's end)
    for dead_on in (False, True):
        d = dead if dead_on else np.zeros(n, bool)
        lst, a_out = kl.scatter_seg(allow, n, kr.pack_dead(dead, words) if dead_on else None, segs, off, fill=FILL)
        assert list(a_out) == [int((m & ~d).sum()) for m in masks]
        written = np.zeros(off, bool)
        for s in segs:
            want = kl.seg_model(masks[s["mask"]], d, int(s["first"]), int(s["n_list"]))
            o = int(s["off"])
            assert np.array_equal(lst[o:o + len(want)], want), (dead_on, s)
            written[o:o + len(want)] = True
        assert (lst[~written] == FILL).all(), "nothing outside the segments"
