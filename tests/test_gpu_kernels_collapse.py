"""Kernel-level checks of the collapsed search (csrc/k_exact.hip): launch_group_check,
launch_collapse_walk, and one round of the group scan (launch_collapse_scan, launch_collapse_select,
launch_merge_parts, launch_collapse_finish), through the test-only shim, against the model of
tests/kcheck_collapse.py -- bit for bit."""
import numpy as np
import pytest

import kcheck_collapse as kl
import kcheck_exact as kx
import kcheck_range as kr
from kcheck_exact import IDX_NONE, KEY_NONE

pytestmark = pytest.mark.gpu

F = np.float32
OFFSET = 5_000_000_000
FILL = 0x5A5A5A5A


# ----------------------------------------------------------------------------------------
# launch_group_check
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1000, 300_000])  # (300000: more rows than one pass of the grid)
def test_group_check(gpu, n):
    rng = np.random.default_rng(n)
    n_groups = 37
    rg = rng.integers(0, n_groups, n).astype(np.uint32)
    assert kl.group_check(rg, n, n_groups) == 0
    assert kl.group_check(rg, n, 2 ** 32 - 1) == 0
    for pos in (0, n - 1, n // 2):
        bad = rg.copy()
        bad[pos] = n_groups
        assert kl.group_check(bad, n, n_groups) == 1, pos
        bad[pos] = 0xFFFFFFFF
        assert kl.group_check(bad, n, n_groups) == 1, pos
        assert kl.group_check(bad, n, n_groups + 1) == (1 if n_groups + 1 <= bad[pos] else 0)
    # (an entry past n is not the check's business)
    assert kl.group_check(np.append(rg, np.uint32(n_groups)), n, n_groups) == 0


# ----------------------------------------------------------------------------------------
# launch_collapse_walk
# ----------------------------------------------------------------------------------------
def walk_model(ids, dist, cnt, fetch_k, k, n, offset, row_group):
    """First occurrences of the groups in list order, the first k of them."""
    m = min(int(cnt), fetch_k)
    oi, od, og, seen = [], [], [], set()
    for p in range(m):
        g_id = int(ids[p])
        if g_id < offset or g_id - offset >= n:
            continue  # no candidate
        g = int(row_group[g_id - offset])
        if g in seen:
            continue
        seen.add(g)
        if len(oi) < k:
            oi.append(g_id), od.append(dist[p]), og.append(g)
    c = len(oi)
    idx = np.full(k, IDX_NONE, np.uint64)
    dd = np.full(k, np.inf, F)
    gg = np.full(k, kl.GROUP_NONE, np.uint32)
    idx[:c], dd[:c], gg[:c] = oi, od, og
    return idx, dd, gg, c, (len(seen) < k and cnt >= fetch_k)


class WalkCases:
    """Crafted candidate lists, each over rows of its own (so its groups are its own): the slots of a
    list hold ascending rows at ascending distances (adjacent pairs tie), the slots past the count
    valid ids of groups seen nowhere else (a walk that reads past the count finds them)."""

    ROWS = 2 * kl.MAX_FETCH

    def __init__(self, fetch_k, k):
        self.fetch_k, self.k = fetch_k, k
        self.ids, self.dist, self.cnt, self.groups, self.tags = [], [], [], [], []
        self.past_end = []  # (case, position): slots that get the id just past the shard

    def add(self, tag, cnt, pos_groups, outside=()):
        """pos_groups: the group of list position p, for p < cnt (ids local to the case)."""
        q = len(self.ids)
        base = q * self.ROWS
        fk = self.fetch_k
        rows = base + 2 * np.arange(fk)  # (ascending; every second row of the case's range)
        rg = np.arange(base, base + self.ROWS, dtype=np.int64) + 1_000_000  # unique groups by default
        g = np.asarray(pos_groups, np.int64)
        assert len(g) == cnt <= fk
        rg[rows[:cnt] - base] = g + q * 1000  # (the case's own group ids)
        ids = (rows + OFFSET).astype(np.uint64)
        for p, bad in outside:
            if bad is None:
                self.past_end.append((q, p))
            else:
                ids[p] = bad
        self.ids.append(ids)
        self.dist.append((np.arange(fk) // 2 * F(0.001)).astype(F))
        self.cnt.append(cnt)
        self.groups.append(rg)
        self.tags.append(tag)

    def arrays(self, sel):
        n = len(self.ids) * self.ROWS
        rg = np.concatenate(self.groups).astype(np.uint32)
        return (np.stack([self.ids[i] for i in sel]), np.stack([self.dist[i] for i in sel]),
                np.array([self.cnt[i] for i in sel], np.uint32), n, rg)


def build_walk_cases(fetch_k, k):
    c = WalkCases(fetch_k, k)
    rng = np.random.default_rng(fetch_k * 1000 + k)
    for cnt in sorted({0, 1, fetch_k - 1, fetch_k}):
        c.add(("one group", cnt), cnt, np.full(cnt, 3))
        c.add(("own groups", cnt), cnt, np.arange(cnt))
        c.add(("random groups", cnt), cnt, rng.integers(0, max(1, k + 2), cnt))
        if cnt >= 1:
            # the k-th new group at the last position (cnt >= k), else cnt - 1 < k groups cycled
            first = np.arange(cnt - 1) % max(1, min(k - 1, cnt - 1)) if k > 1 else np.zeros(cnt - 1, np.int64)
            c.add(("k-th group last", cnt), cnt, np.append(first, 500))
        if cnt >= 2:
            # ids outside the shard: below the offset at position 0, past its end in the middle; their
            # would-be rows carry a group of their own
            g = np.arange(cnt) % max(1, k)
            c.add(("outside ids", cnt), cnt, g, outside=[(0, np.uint64(OFFSET - 1)), (cnt // 2, None)])
    # (the id just past the shard is known only once every case exists)
    n = len(c.ids) * c.ROWS
    for q, p in c.past_end:
        c.ids[q][p] = np.uint64(OFFSET + n)
    return c


@pytest.mark.parametrize("fetch_k", [1, 5, 64, 65, 256])
def test_walk(gpu, fetch_k):
    for k in sorted({1, fetch_k}):
        c = build_walk_cases(fetch_k, k)
        total = len(c.ids)
        n_fail_seen = 0
        # every case in one launch (a partly filled last workgroup unless total % 4 == 0), then
        # launches of 1, 4 and 5 queries
        for sel in (list(range(total)), [total - 1], list(range(4)), list(range(2, 7))):
            ids, dist, cnt, n, rg = c.arrays(sel)
            rc, oi, od, oc, og, fail, nfail = kl.walk(ids, dist, cnt, k, n, OFFSET, rg)
            assert rc == 0
            want_fail = set()
            for j, i in enumerate(sel):
                wi, wd, wg, wc, wf = walk_model(ids[j], dist[j], cnt[j], fetch_k, k, n, OFFSET, rg)
                what = (fetch_k, k, c.tags[i])
                assert oc[j] == wc, (what, oc[j], wc)
                assert np.array_equal(oi[j], wi), (what, oi[j], wi)
                assert np.array_equal(od[j].view(np.uint32), wd.view(np.uint32)), what
                assert np.array_equal(og[j], wg), (what, og[j], wg)
                if wf:
                    want_fail.add(j)
                # the list is in (distance, id) order, so the contract's model agrees with the walk
                loc = ids[j][:cnt[j]].astype(np.int64) - OFFSET
                inside = (loc >= 0) & (loc < n)
                listed = np.zeros(n, bool)
                listed[loc[inside]] = True
                dvec = np.full(n, np.inf, F)
                dvec[loc[inside]] = dist[j][:cnt[j]][inside]
                mi, md, mg, mc = kl.collapse_model(dvec, rg, k, allowed=listed, offset=OFFSET)
                assert mc == wc and np.array_equal(mi, wi) and np.array_equal(mg, wg), what
            assert nfail == len(want_fail) and set(fail[:nfail].tolist()) == want_fail, (fetch_k, k, sel, fail[:nfail])
            assert (fail[nfail:] == FILL).all()
            n_fail_seen += nfail
            # without out_group: the same rows
            rc, oi2, od2, oc2, og2, _, nfail2 = kl.walk(ids, dist, cnt, k, n, OFFSET, rg, with_group=False)
            assert rc == 0 and og2 is None and np.array_equal(oi2, oi) and np.array_equal(oc2, oc) and nfail2 == nfail
        if k > 1:
            assert n_fail_seen >= 2, "a full list of one group must fail"
        # all candidates in one group: exactly the queries whose list is full fail
        sel = [i for i, t in enumerate(c.tags) if t[0] == "one group"]
        ids, dist, cnt, n, rg = c.arrays(sel)
        rc, oi, od, oc, og, fail, nfail = kl.walk(ids, dist, cnt, k, n, OFFSET, rg)
        full = {j for j in range(len(sel)) if cnt[j] >= fetch_k and k > 1}
        assert rc == 0 and set(fail[:nfail].tolist()) == full and nfail == len(full)
        assert all(oc[j] == min(1, cnt[j]) for j in range(len(sel)))


def test_walk_refusals(gpu):
    ids = np.zeros((1, 4), np.uint64)
    d = np.zeros((1, 4), F)
    cnt = np.zeros(1, np.uint32)
    rg = np.zeros(8, np.uint32)
    assert kl.walk(ids, d, cnt, 0, 8, 0, rg)[0] == 1       # k = 0
    assert kl.walk(ids, d, cnt, 5, 8, 0, rg)[0] == 1       # k > fetch_k
    big = np.zeros((1, kl.MAX_FETCH + 1), np.uint64)
    assert kl.walk(big, big.astype(F), cnt, 2, 8, 0, rg)[0] == 1  # fetch_k > 256


# ----------------------------------------------------------------------------------------
# the group scan, its selection and finish
# ----------------------------------------------------------------------------------------
_corpora = {}


def scan_corpus(dim):
    if dim not in _corpora:
        c = kx.Corpus(1000, dim, 12, 1900 + dim)
        c.all_dist = [c.dist(q) for q in range(c.nq)]
        _corpora[dim] = c
    return _corpora[dim]


def groups_of(kind, n):
    i = np.arange(n)
    return {"1": (np.zeros(n, np.int64), 1), "3": (i % 3, 3), "n": (i, n), "7": (i // 7, (n + 6) // 7)}[kind]


def best_model(dist, n, rg, n_groups, ok):
    t = np.full(n_groups, KEY_NONE, np.uint64)
    keys = kx.dist_key(dist[:n], np.arange(n))
    rows = np.flatnonzero(ok[:n])
    np.minimum.at(t, rg[rows], keys[rows])
    return t


def tombstones_and_masks(rng, corp, ids, n, rg, ng, k):
    """The masked set-up of a launch over the first n rows for the queries ids: (live [corp.n], masks
    [3][n], allow words, mask id by query id)."""
    # tombstones: a third of the rows, the unmasked heads of the first query among
    # them, and the whole of group 1 (or of the first head's group)
    live = rng.random(corp.n) >= 0.3
    h0 = kl.collapse_model(corp.all_dist[ids[0]][:n], rg, k)[0]
    heads0 = h0[h0 != IDX_NONE].astype(np.int64)
    live[heads0[::2]] = False
    if ng > 1:
        live[:n][rg == rg[min(1, n - 1)]] = False
    # three masks: a random half; everything but the heads of the launch's last query
    # and one whole group; everything
    masks = np.ones((3, n), bool)
    masks[0] = rng.random(n) < 0.5
    hl = kl.collapse_model(corp.all_dist[ids[-1]][:n], rg, k, live=live[:n])[0]
    headsl = hl[hl != IDX_NONE].astype(np.int64)
    masks[1, headsl] = False
    if len(headsl) > 1:
        masks[1, rg == rg[headsl[1]]] = False
    allow = np.stack([kr.pack_dead(m) for m in masks])
    # (the mask ids by query id: two queries of one launch differ in their masks)
    qm = np.arange(corp.nq, dtype=np.uint32) % 3
    qm[ids[-1]] = 1
    if len(ids) >= 2:
        qm[ids[0]] = 0
    return live, masks, allow, qm


SCAN_CASES = [(100, nqf) for nqf in range(1, 9)] + [(d, nqf) for d in (8, 768) for nqf in (1, 5, 8)]


@pytest.mark.parametrize("dim,nqf", SCAN_CASES)
def test_scan_select_finish(gpu, dim, nqf):
    corp = scan_corpus(dim)
    rng = np.random.default_rng(dim * 10 + nqf)
    width = 1 if nqf <= 1 else 2 if nqf <= 2 else 4 if nqf <= 4 else 8
    ids = [int(x) for x in rng.permutation(corp.nq)[:nqf]]
    if nqf >= 2 and 0 not in ids:
        ids[0] = 0  # (query 0: the rows identical to it, at distance 0 through the 1e-10 rule)
    qids = np.array(ids + [ids[0]] * (width - nqf), np.int32)
    launches = 0
    for n in (1, 255, 256, 257, 1000):
        for kind, k in (("1", 1), ("n", 1), ("1", 10), ("3", 10), ("n", 10), ("7", 10), ("3", 256), ("n", 256)):
            rg, ng = groups_of(kind, n)
            for masked in (False, True):
                live = np.ones(corp.n, bool)
                allow = None
                qm = None
                masks = None
                if masked:
                    live, masks, allow, qm = tombstones_and_masks(rng, corp, ids, n, rg, ng, k)
                dead = kr.pack_dead(~live, corp.rows.shape[0] // 64) if masked else None
                rc, oi, od, oc, og, best = kl.scan(corp.rows, corp.dim, n, OFFSET, corp.na, corp.qf32, corp.nb, rg, ng,
                                                   qids, nqf, k, dead=dead, allow=allow, query_mask=qm)
                assert rc == 0
                launches += 1
                for j, q in enumerate(ids):
                    what = (dim, nqf, n, kind, k, masked, j, q)
                    ok = live[:n] & (masks[qm[q]] if masked else True)
                    wi, wd, wg, wc = kl.collapse_model(corp.all_dist[q][:n], rg, k, live=live[:n],
                                                       allowed=masks[qm[q]] if masked else None, offset=OFFSET)
                    assert np.array_equal(best[j], best_model(corp.all_dist[q], n, rg, ng, ok)), (what, "table")
                    assert oc[q] == wc, (what, oc[q], wc)
                    assert np.array_equal(oi[q], wi), (what, oi[q][:12], wi[:12])
                    assert np.array_equal(od[q].view(np.uint32), wd.view(np.uint32)), what
                    assert np.array_equal(og[q], wg), what
                    assert wc == min(k, len(set(rg[ok].tolist()))), what
                # the queries outside the launch (the padding ids among them write nothing new)
                others = np.setdiff1d(np.arange(corp.nq), ids)
                assert (oi[others] == 0x1234).all() and (oc[others] == FILL).all() and (og[others] == FILL).all()
    assert launches == 80
    # query 0's identical rows head their groups at distance exactly 0; duplicate rows (the run of
    # 100) within one group and across groups resolve to the smallest row
    if 0 in ids:
        rg, ng = groups_of("7", 1000)
        rc, oi, od, oc, og, best = kl.scan(corp.rows, corp.dim, 1000, 0, corp.na, corp.qf32, corp.nb, rg, ng, qids, nqf, 10)
        # (row 7 differs from query 0 by 2e-10 in one element: not identical; its distance is 0 or a
        # rounding above it, by the dimension, so it comes between or right behind the identical rows)
        assert rc == 0 and np.array_equal(oi[0], kl.collapse_model(corp.all_dist[0], rg, 10)[0])
        zero = oi[0][od[0] == 0].tolist()
        assert set(corp.ident) <= set(zero) and set(zero) <= set(corp.ident + [corp.near]) and zero == sorted(zero)
        assert set(oi[0][:4].tolist()) == set(corp.ident + [corp.near])
    q = ids[-1]
    run = np.arange(corp.run, corp.run + 100)
    d_run = corp.all_dist[q][run]
    assert (d_run == d_run[0]).all()
    for kind in ("3", "7"):
        rg, ng = groups_of(kind, 1000)
        allow = kr.pack_dead(np.isin(np.arange(1000), run))[None, :]  # only the run is allowed
        rc, oi, od, oc, og, best = kl.scan(corp.rows, corp.dim, 1000, 0, corp.na, corp.qf32, corp.nb, rg, ng, qids, nqf,
                                           256, allow=allow)
        groups = sorted(set(rg[run].tolist()))
        firsts = sorted(int(run[rg[run] == g][0]) for g in groups)
        assert rc == 0 and oc[q] == len(groups) and list(oi[q][:oc[q]]) == firsts


def test_scan_grids(gpu):
    """launch_collapse_scan on other grids than scan_grid_for(n), which gives every workgroup one tile
    here: on 2 workgroups one of them walks a second tile at n = 600 and both do at n = 1000 (the first
    chunk of the next tile is prefetched during the last chunk of this one), and one has no tile at
    n = 1; on 5 there are more workgroups than tiles.  The same tables and outputs."""
    corp = scan_corpus(100)
    k = 10
    launches = 0
    for nqf in (1, 3, 8):
        rng = np.random.default_rng(7000 + nqf)
        width = 1 if nqf <= 1 else 2 if nqf <= 2 else 4 if nqf <= 4 else 8
        ids = [int(x) for x in rng.permutation(corp.nq)[:nqf]]
        qids = np.array(ids + [ids[0]] * (width - nqf), np.int32)
        for n in (1, 600, 1000):
            rg, ng = groups_of("7", n)
            for masked in (False, True):
                live, masks, allow, qm, dead = np.ones(corp.n, bool), None, None, None, None
                if masked:
                    live, masks, allow, qm = tombstones_and_masks(rng, corp, ids, n, rg, ng, k)
                    dead = kr.pack_dead(~live, corp.rows.shape[0] // 64)
                want = []
                for q in ids:
                    allowed = masks[qm[q]] if masked else None
                    ok = live[:n] & (allowed if masked else True)
                    want.append((best_model(corp.all_dist[q], n, rg, ng, ok),
                                 kl.collapse_model(corp.all_dist[q][:n], rg, k, live=live[:n], allowed=allowed,
                                                   offset=OFFSET)))
                for grid in (2, 5):
                    rc, oi, od, oc, og, best = kl.scan(corp.rows, corp.dim, n, OFFSET, corp.na, corp.qf32, corp.nb, rg,
                                                       ng, qids, nqf, k, dead=dead, allow=allow, query_mask=qm, grid=grid)
                    assert rc == 0
                    launches += 1
                    for j, q in enumerate(ids):
                        what = (nqf, n, masked, grid, j, q)
                        table, (wi, wd, wg, wc) = want[j]
                        assert np.array_equal(best[j], table), (what, "table")
                        assert oc[q] == wc, (what, oc[q], wc)
                        assert np.array_equal(oi[q], wi), (what, oi[q], wi)
                        assert np.array_equal(od[q].view(np.uint32), wd.view(np.uint32)), what
                        assert np.array_equal(og[q], wg), what
                    others = np.setdiff1d(np.arange(corp.nq), ids)
                    assert (oi[others] == 0x1234).all() and (oc[others] == FILL).all() and (og[others] == FILL).all()
    assert launches == 36


def test_scan_refusals(gpu):
    corp = scan_corpus(8)
    rg = np.zeros(10, np.uint32)
    qids = np.zeros(8, np.int32)
    args = (corp.rows, corp.dim, 10, 0, corp.na, corp.qf32, corp.nb, rg)
    assert kl.scan(*args, 1, qids, 0, 4)[0] == 1          # nqf = 0
    assert kl.scan(*args, 1, qids, 1, 257)[0] == 1        # k > 256
