"""Kernel-level checks of the capped search (csrc/k_exact.hip): launch_cap_walk, and one round of the
capped group scan (launch_cap_scan, launch_collapse_select, launch_merge_parts,
launch_collapse_finish), through the test-only shim, against the model of tests/kcheck_cap.py -- bit
for bit; with per_group = 1, byte for byte against the collapsed search's launchers."""
import numpy as np
import pytest

import kcheck_cap as kp
import kcheck_exact as kx
import kcheck_range as kr
from kcheck_exact import IDX_NONE, KEY_NONE

pytestmark = pytest.mark.gpu

F = np.float32
OFFSET = 5_000_000_000
FILL = 0x5A5A5A5A


# ----------------------------------------------------------------------------------------
# launch_cap_walk
# ----------------------------------------------------------------------------------------
def walk_model(ids, dist, cnt, fetch_k, k, m, n, offset, row_group):
    """The rows of the list with fewer than m earlier list rows of their group, in list order, the
    first k of them; (idx, dist, group, count, fails)."""
    oi, od, og, have, kept = [], [], [], {}, 0
    for p in range(min(int(cnt), fetch_k)):
        g_id = int(ids[p])
        if g_id < offset or g_id - offset >= n:
            continue  # no candidate
        g = int(row_group[g_id - offset])
        have[g] = have.get(g, 0) + 1
        if have[g] > m:
            continue
        kept += 1
        if len(oi) < k:
            oi.append(g_id), od.append(dist[p]), og.append(g)
    c = len(oi)
    idx = np.full(k, IDX_NONE, np.uint64)
    dd = np.full(k, np.inf, F)
    gg = np.full(k, kp.GROUP_NONE, np.uint32)
    idx[:c], dd[:c], gg[:c] = oi, od, og
    return idx, dd, gg, c, (kept < k and cnt >= fetch_k)


class WalkCases:
    """Crafted candidate lists, each over rows of its own (so its groups are its own): the slots of a
    list hold ascending rows at ascending distances (adjacent pairs tie), the slots past the count
    valid ids of groups seen nowhere else (a walk that reads past the count finds them)."""

    ROWS = 2 * kp.MAX_FETCH

    def __init__(self, fetch_k):
        self.fetch_k = fetch_k
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


def build_walk_cases(fetch_k, k, m):
    c = WalkCases(fetch_k)
    rng = np.random.default_rng(fetch_k * 1000 + k * 17 + m)
    for cnt in sorted({0, 1, fetch_k - 1, fetch_k}):
        c.add(("one group", cnt), cnt, np.full(cnt, 3))
        c.add(("own groups", cnt), cnt, np.arange(cnt))
        c.add(("three groups", cnt), cnt, rng.integers(0, 3, cnt))
        if cnt >= 1:
            # k - 1 kept rows (groups filled m at a time), then rows of the first, full group (dropped
            # where it is full), then a new group at the last position: the k-th kept row where the
            # list is long enough
            first = np.arange(cnt - 1) // m
            first[k - 1:] = 0
            c.add(("k-th kept row last", cnt), cnt, np.append(first, 500))
        if cnt >= 2:
            # ids outside the shard: below the offset at position 0, past its end in the middle; their
            # would-be rows carry a group of their own
            g = np.arange(cnt) % max(1, (k + m - 1) // m)
            c.add(("outside ids", cnt), cnt, g, outside=[(0, np.uint64(OFFSET - 1)), (cnt // 2, None)])
    # (the id just past the shard is known only once every case exists)
    n = len(c.ids) * c.ROWS
    for q, p in c.past_end:
        c.ids[q][p] = np.uint64(OFFSET + n)
    return c


@pytest.mark.parametrize("fetch_k", [1, 5, 64, 65, 256])
def test_walk(gpu, fetch_k):
    fails_seen = one_group_checked = 0
    for k in sorted({1, (fetch_k + 1) // 2, fetch_k}):
        for m in (1, 2, 3, 16):
            c = build_walk_cases(fetch_k, k, m)
            total = len(c.ids)
            # every case in one launch (a partly filled last workgroup unless total % 4 == 0), then
            # launches of 1, 4 and 5 queries
            for sel in (list(range(total)), [total - 1], list(range(4)), list(range(2, 7))):
                sel = [i for i in sel if i < total]
                ids, dist, cnt, n, rg = c.arrays(sel)
                rc, oi, od, oc, og, fail, nfail = kp.walk(ids, dist, cnt, k, m, n, OFFSET, rg)
                assert rc == 0
                want_fail = set()
                for j, i in enumerate(sel):
                    wi, wd, wg, wc, wf = walk_model(ids[j], dist[j], cnt[j], fetch_k, k, m, n, OFFSET, rg)
                    what = (fetch_k, k, m, c.tags[i])
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
                    mi, md, mg, mc = kp.cap_model(dvec, rg, k, m, allowed=listed, offset=OFFSET)
                    assert mc == wc and np.array_equal(mi, wi) and np.array_equal(mg, wg), what
                    if c.tags[i][0] == "one group":
                        assert oc[j] == min(m, k, cnt[j]), what
                        one_group_checked += 1
                assert nfail == len(want_fail) and set(fail[:nfail].tolist()) == want_fail, (fetch_k, k, m, sel)
                assert (fail[nfail:] == FILL).all()
                fails_seen += nfail
                # without out_group: the same rows
                rc, oi2, od2, oc2, og2, _, nfail2 = kp.walk(ids, dist, cnt, k, m, n, OFFSET, rg, with_group=False)
                assert rc == 0 and og2 is None and np.array_equal(oi2, oi) and np.array_equal(oc2, oc)
                assert nfail2 == nfail
                if m == 1:
                    # the collapsed search's walk on the same input: the same bytes
                    rc, ci, cd, cc, cg, cfail, cn = kp.walk(ids, dist, cnt, k, m, n, OFFSET, rg, collapse=True)
                    assert rc == 0 and cn == nfail and set(cfail[:cn].tolist()) == set(fail[:nfail].tolist())
                    for a, b in ((ci, oi), (cd, od), (cc, oc), (cg, og)):
                        assert a.tobytes() == b.tobytes(), (fetch_k, k, "m = 1 against launch_collapse_walk")
    assert one_group_checked
    if fetch_k > 1:
        assert fails_seen >= 2, "a full list of one group must fail for k > m"


def test_walk_cap_above_k_keeps_the_list_head(gpu):
    """per_group >= k: the first k candidates, whatever their groups, and no failure."""
    rng = np.random.default_rng(9)
    nq, fetch_k, n = 7, 40, 500
    ids = np.stack([np.sort(rng.choice(n, fetch_k, replace=False)) for _ in range(nq)]).astype(np.uint64) + np.uint64(OFFSET)
    dist = np.sort(rng.random((nq, fetch_k)).astype(F), axis=1)
    cnt = np.array([40, 40, 39, 12, 0, 40, 5], np.uint32)
    rg = np.zeros(n, np.uint32)  # (one group)
    for k, m in ((12, 12), (12, 16), (5, 16), (16, 16)):
        rc, oi, od, oc, og, fail, nfail = kp.walk(ids, dist, cnt, k, m, n, OFFSET, rg)
        assert rc == 0 and nfail == 0
        for q in range(nq):
            c = min(k, int(cnt[q]))
            assert oc[q] == c and np.array_equal(oi[q][:c], ids[q][:c]) and (oi[q][c:] == IDX_NONE).all()
            assert np.array_equal(od[q][:c].view(np.uint32), dist[q][:c].view(np.uint32)) and np.isposinf(od[q][c:]).all()


def test_walk_refusals(gpu):
    ids = np.zeros((1, 4), np.uint64)
    d = np.zeros((1, 4), F)
    cnt = np.zeros(1, np.uint32)
    rg = np.zeros(8, np.uint32)
    assert kp.walk(ids, d, cnt, 0, 2, 8, 0, rg)[0] == 1       # k = 0
    assert kp.walk(ids, d, cnt, 5, 2, 8, 0, rg)[0] == 1       # k > fetch_k
    assert kp.walk(ids, d, cnt, 2, 0, 8, 0, rg)[0] == 1       # per_group = 0
    big = np.zeros((1, kp.MAX_FETCH + 1), np.uint64)
    assert kp.walk(big, big.astype(F), cnt, 2, 2, 8, 0, rg)[0] == 1  # fetch_k > 256


# ----------------------------------------------------------------------------------------
# the capped group scan, its selection and finish
# ----------------------------------------------------------------------------------------
_corpora = {}
NQ = 12


def scan_corpus(n, dim):
    if (n, dim) not in _corpora:
        c = kx.Corpus(n, dim, NQ, 2000 + n + dim)
        c.all_dist = [c.dist(q) for q in range(c.nq)]
        c.all_keys = [kx.dist_key(c.all_dist[q], np.arange(n)) for q in range(c.nq)]
        _corpora[(n, dim)] = c
    return _corpora[(n, dim)]


def table_model(keys, rg, n_groups, m, ok):
    """[n_groups][m]: the m smallest keys of every group's rows in ok, ascending, KEY_NONE behind."""
    t = np.full((n_groups, m), KEY_NONE, np.uint64)
    for g in range(n_groups):
        ks = np.sort(keys[ok & (rg == g)])[:m]
        t[g, :len(ks)] = ks
    return t


def tombstones_and_masks(rng, corp, ids, n, rg, k, m):
    """The masked set-up of a launch over the first n rows for the queries ids: (live [n], masks
    [3][n], allow words, mask id by query id, dead words)."""
    # tombstones: a third of the rows, with every second row the first query keeps;
    # three masks: a random half; everything but the rows the launch's last query
    # keeps; everything
    live = rng.random(n) >= 0.3
    k0 = kp.cap_model(corp.all_dist[ids[0]][:n], rg, k, m)[0]
    live[k0[k0 != IDX_NONE].astype(np.int64)[::2]] = False
    masks = np.ones((3, n), bool)
    masks[0] = rng.random(n) < 0.5
    kl_ = kp.cap_model(corp.all_dist[ids[-1]][:n], rg, k, m, live=live)[0]
    masks[1, kl_[kl_ != IDX_NONE].astype(np.int64)] = False
    allow = np.stack([kr.pack_dead(x) for x in masks])
    # (the mask ids by query id: two queries of one launch differ in their masks)
    qm = np.arange(corp.nq, dtype=np.uint32) % 3
    qm[ids[-1]] = 1
    if len(ids) >= 2:
        qm[ids[0]] = 0
    return live, masks, allow, qm, kr.pack_dead(~live, corp.rows.shape[0] // 64)


@pytest.mark.parametrize("nqf", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("n,dim", [(130, 768), (600, 768), (600, 200)])
def test_scan_select_finish(gpu, n, dim, nqf):
    corp = scan_corpus(n, dim)
    rng = np.random.default_rng(n * 10 + dim + nqf)
    width = 1 if nqf <= 1 else 2 if nqf <= 2 else 4 if nqf <= 4 else 8
    perm = [int(x) for x in rng.permutation(corp.nq)]
    ids, pad = perm[:nqf], perm[nqf:nqf + width - nqf]  # (the padding ids: queries outside the launch)
    qids = np.array(ids + pad, np.int32)
    launches = 0
    i = np.arange(n)
    for rg, ng in ((np.zeros(n, np.int64), 1), (i % 3, 3), (i // 7, n // 7 + 1)):
        for m in (1, 2, 3, 8, 16):
            k = 256 if m == 16 else 10
            for masked in (False, True):
                live = np.ones(n, bool)
                dead = allow = qm = masks = None
                if masked:
                    live, masks, allow, qm, dead = tombstones_and_masks(rng, corp, ids, n, rg, k, m)
                rc, oi, od, oc, og, best = kp.scan(corp.rows, corp.dim, n, OFFSET, corp.na, corp.qf32, corp.nb, rg, ng,
                                                   qids, nqf, k, m, dead=dead, allow=allow, query_mask=qm)
                assert rc == 0
                launches += 1
                for j, q in enumerate(ids):
                    what = (n, dim, nqf, ng, m, masked, j, q)
                    allowed = masks[qm[q]] if masked else None
                    ok = live & (allowed if masked else True)
                    # the table per (query, group): the m smallest keys, in any order
                    assert np.array_equal(np.sort(best[j], axis=1), table_model(corp.all_keys[q], rg, ng, m, ok)), \
                        (what, "table")
                    wi, wd, wg, wc = kp.cap_model(corp.all_dist[q], rg, k, m, live=live, allowed=allowed, offset=OFFSET)
                    assert oc[q] == wc, (what, oc[q], wc)
                    assert np.array_equal(oi[q], wi), (what, oi[q][:12], wi[:12])
                    assert np.array_equal(od[q].view(np.uint32), wd.view(np.uint32)), what
                    assert np.array_equal(og[q], wg), what
                    assert wc == min(k, sum(min(m, int(c)) for c in np.bincount(rg[ok], minlength=1))), what
                # the padding slots' tables stay empty; the queries outside the launch (the padding
                # ids among them) get nothing written
                assert (best[nqf:] == KEY_NONE).all()
                others = np.setdiff1d(np.arange(corp.nq), ids)
                assert (oi[others] == 0x1234).all() and (oc[others] == FILL).all() and (og[others] == FILL).all()
                if m == 1:
                    # the collapsed search's scan on the same input: the same table, the same outputs
                    rc, ci, cd, cc, cg, cbest = kp.scan(corp.rows, corp.dim, n, OFFSET, corp.na, corp.qf32, corp.nb, rg,
                                                        ng, qids, nqf, k, 1, dead=dead, allow=allow, query_mask=qm,
                                                        collapse=True)
                    assert rc == 0 and cbest.tobytes() == best.tobytes()
                    for a, b in ((ci, oi), (cd, od), (cc, oc), (cg, og)):
                        assert a.tobytes() == b.tobytes()
    assert launches == 30
    # the run of 100 identical rows under a mask that allows only them: equal distances within and
    # across groups, so every group keeps its m smallest row ids
    q = ids[-1]
    run = np.arange(corp.run, corp.run + 100) if n >= corp.run + 100 else None
    if run is not None:
        d_run = corp.all_dist[q][run]
        assert (d_run == d_run[0]).all()
        allow = kr.pack_dead(np.isin(i, run))[None, :]
        for rg, ng, m in ((i % 3, 3, 3), (i // 7, n // 7 + 1, 2), (np.zeros(n, np.int64), 1, 16)):
            rc, oi, od, oc, og, best = kp.scan(corp.rows, corp.dim, n, 0, corp.na, corp.qf32, corp.nb, rg, ng, qids, nqf,
                                               256, m, allow=allow)
            firsts = sorted(int(r) for g in set(rg[run].tolist()) for r in run[rg[run] == g][:m])
            assert rc == 0 and oc[q] == len(firsts) and list(oi[q][:oc[q]]) == firsts, (ng, m)


def test_scan_grids(gpu):
    """launch_cap_scan on other grids than scan_grid_for(n), which gives every workgroup one tile here:
    on 2 workgroups one of them walks a second tile at n = 600 and both do at n = 1000 (the first chunk
    of the next tile is prefetched during the last chunk of this one), and one has no tile at n = 1; on
    5 there are more workgroups than tiles.  The same tables and outputs."""
    corp = scan_corpus(1000, 200)
    k = 10
    launches = 0
    for nqf in (1, 3, 8):
        rng = np.random.default_rng(7100 + nqf)
        width = 1 if nqf <= 1 else 2 if nqf <= 2 else 4 if nqf <= 4 else 8
        perm = [int(x) for x in rng.permutation(corp.nq)]
        ids = perm[:nqf]
        qids = np.array(perm[:width], np.int32)  # (the padding ids: queries outside the launch)
        for n in (1, 600, 1000):
            rg, ng = np.arange(n) // 7, n // 7 + 1
            for m in (1, 3):
                for masked in (False, True):
                    live = np.ones(n, bool)
                    dead = allow = qm = masks = None
                    if masked:
                        live, masks, allow, qm, dead = tombstones_and_masks(rng, corp, ids, n, rg, k, m)
                    want = []
                    for q in ids:
                        allowed = masks[qm[q]] if masked else None
                        ok = live & (allowed if masked else True)
                        want.append((table_model(corp.all_keys[q][:n], rg, ng, m, ok),
                                     kp.cap_model(corp.all_dist[q][:n], rg, k, m, live=live, allowed=allowed,
                                                  offset=OFFSET)))
                    for grid in (2, 5):
                        rc, oi, od, oc, og, best = kp.scan(corp.rows, corp.dim, n, OFFSET, corp.na, corp.qf32, corp.nb,
                                                           rg, ng, qids, nqf, k, m, dead=dead, allow=allow,
                                                           query_mask=qm, grid=grid)
                        assert rc == 0
                        launches += 1
                        for j, q in enumerate(ids):
                            what = (nqf, n, m, masked, grid, j, q)
                            table, (wi, wd, wg, wc) = want[j]
                            assert np.array_equal(np.sort(best[j], axis=1), table), (what, "table")
                            assert oc[q] == wc, (what, oc[q], wc)
                            assert np.array_equal(oi[q], wi), (what, oi[q], wi)
                            assert np.array_equal(od[q].view(np.uint32), wd.view(np.uint32)), what
                            assert np.array_equal(og[q], wg), what
                        assert (best[nqf:] == KEY_NONE).all()
                        others = np.setdiff1d(np.arange(corp.nq), ids)
                        assert (oi[others] == 0x1234).all() and (oc[others] == FILL).all() and (og[others] == FILL).all()
    assert launches == 72


def test_scan_refusals(gpu):
    corp = scan_corpus(130, 768)
    rg = np.zeros(10, np.uint32)
    qids = np.zeros(8, np.int32)
    args = (corp.rows, corp.dim, 10, 0, corp.na, corp.qf32, corp.nb, rg)
    assert kp.scan(*args, 1, qids, 0, 4, 2)[0] == 1          # nqf = 0
    assert kp.scan(*args, 1, qids, 1, 257, 2)[0] == 1        # k > 256
    assert kp.scan(*args, 1, qids, 1, 4, 0)[0] == 1          # m = 0
    assert kp.scan(*args, 1, qids, 1, 4, 17)[0] == 1         # m > 16
