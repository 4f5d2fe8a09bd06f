"""Kernel-level checks of the exact scans and their merges (csrc/k_exact.hip): launch_scan_exact,
launch_scan_list, launch_scan_list_groups, launch_merge_parts, launch_merge_parts_groups,
launch_finalize -- and launch_row_norms (csrc/k_prep.hip), whose magnitudes are the exact stage's
input -- against the models of tests/kcheck_exact.py, bit for bit.
"""
import numpy as np
import pytest

import kcheck as kc
import kcheck_exact as kx
from kcheck_exact import KEY_NONE, POS_INF

pytestmark = pytest.mark.gpu

KFILL = np.uint64(0x5A5A5A5A5A5A5A5A)
INVALID = 1  # hipErrorInvalidValue
NS = (1, 255, 256, 257, 773, 2561)


@pytest.fixture(autouse=True, scope="module")
def _switches_unset():
    kx.assert_no_switches()


_corpora = {}


def corpus(dim):
    """2,561 rows and 24 queries; every distance of the model, computed once."""
    if dim not in _corpora:
        c = kx.Corpus(2561, dim, 24, 300 + dim)
        c.all_keys = [kx.dist_key(c.dist(q), np.arange(c.n, dtype=np.uint64)) for q in range(c.nq)]
        _corpora[dim] = c
    return _corpora[dim]


def qf_for(nqf):
    return 1 if nqf <= 1 else 2 if nqf <= 2 else 4 if nqf <= 4 else 8


def padded_ids(ids, qf):
    """The scan's id list: the ids past nqf repeat the last one."""
    return np.array(list(ids) + [ids[-1]] * (qf - len(ids)), np.int32)


def scan_args(c):
    return dict(rows=c.rows, ld=c.ld, dim=c.dim, na=c.na, qf32=c.qf32, nb=c.nb)


def check_part(c, part, qids, k, tiles_rows, grid):
    """part [grid][qf][k]: block b's list for slot j = the k best keys over the rows of its tiles."""
    for b in range(grid):
        mine = tiles_rows[b::grid]
        rows = np.concatenate(mine) if mine else np.zeros(0, np.int64)
        for j, qid in enumerate(qids):
            want = kx.topk_keys(c.all_keys[qid][rows], k)
            assert np.array_equal(part[b, j], want), (b, j, qid)


@pytest.mark.parametrize("dim", (64, 130, 768, 1100))
def test_scan_exact_and_merge_parts(gpu, dim):
    c = corpus(dim)
    for (nqf, k), ids in zip(((1, 1), (2, 65), (3, 130), (4, 256), (5, 10), (8, 100)),
                             ([7], [3, 0], [11, 2, 5], [1, 4, 9, 6], [10, 8, 0, 2, 7], [5, 11, 3, 9, 1, 6, 4, 0])):
        qf = qf_for(nqf)
        qids = padded_ids(ids, qf)
        for n in NS:
            tiles = [np.arange(t, min(t + 256, n)) for t in range(0, n, 256)]
            for grid in sorted({kx.scan_grid_for(n), 3}):
                part = np.full((grid, qf, k), KFILL, np.uint64)
                assert kx.scan_raw(0, n=n, nqf=nqf, k=k, grid=grid, qids=qids, part=part, **scan_args(c)) == 0
                check_part(c, part, qids, k, tiles, grid)
                out = np.full((c.nq, k), KFILL, np.uint64)
                assert kx.merge_parts(part, grid, qids, nqf, k, out) == 0
                for q in range(c.nq):
                    if q in ids:
                        assert np.array_equal(out[q], kx.topk_keys(c.all_keys[q][:n], k)), (nqf, k, n, grid, q)
                    else:
                        assert (out[q] == KFILL).all(), "rows of other queries keep their pattern"
    assert kx.scan_grid_for(1) == 1 and kx.scan_grid_for(2561) == 11 and kx.scan_grid_for(10 ** 9) == 512
    assert kx.consts().scan_qf == 8


def row_list(c, rng, m):
    """m ascending ids, the last slab rows among them."""
    tail = [c.n - 1, c.n - 2, c.n - 3][:m]
    rest = rng.choice(c.n - 3, m - len(tail), replace=False)
    return np.sort(np.concatenate([rest, tail])).astype(np.uint32)


@pytest.mark.parametrize("dim", (130, 768, 1100))
def test_scan_list(gpu, dim):
    c = corpus(dim)
    rng = np.random.default_rng(dim)
    for (nqf, groups, k) in ((1, 1, 10), (3, 1, 65), (8, 1, 130), (8, 3, 10), (8, 3, 256)):
        qf = qf_for(nqf)
        ids = [int(x) for x in rng.permutation(c.nq)[:nqf]]
        qids = np.concatenate([padded_ids([(i + g) % c.nq for i in ids], qf) for g in range(groups)])
        for m in (1, 256, 257, 1500):
            lst = row_list(c, rng, m)
            assert lst[-1] == c.n - 1 and len(lst) == m and (np.diff(lst.astype(np.int64)) > 0).all()
            grid = kx.scan_grid_for(m)
            tiles = [lst[t:t + 256].astype(np.int64) for t in range(0, m, 256)]
            part = np.full((groups, grid, qf, k), KFILL, np.uint64)
            assert kx.scan_raw(1, list=lst, n_list=m, nqf=nqf, groups=groups, k=k, grid=grid, qids=qids, part=part,
                               **scan_args(c)) == 0
            for g in range(groups):
                gq = qids[g * qf:(g + 1) * qf]
                check_part(c, part[g], gq, k, tiles, grid)
                out = np.full((c.nq, k), KFILL, np.uint64)
                assert kx.merge_parts(np.ascontiguousarray(part[g]), grid, gq, nqf, k, out) == 0
                for q in set(gq[:nqf].tolist()):
                    assert np.array_equal(out[q], kx.topk_keys(c.all_keys[q][lst.astype(np.int64)], k)), (m, g, q)
    # rejected before any launch: an empty list, several groups of fewer than kScanQF queries
    part = np.full((3, 1, 8, 10), KFILL, np.uint64)
    qids = np.zeros(24, np.int32)
    lst = np.arange(5, dtype=np.uint32)
    assert kx.scan_raw(1, list=lst, n_list=0, nqf=8, groups=1, k=10, grid=1, qids=qids, part=part, **scan_args(c)) == INVALID
    assert kx.scan_raw(1, list=lst, n_list=5, nqf=4, groups=3, k=10, grid=1, qids=qids, part=part, **scan_args(c)) == INVALID
    assert (part == KFILL).all()


@pytest.mark.parametrize("qf", (1, 2, 4, 8))
def test_scan_list_groups_and_merge(gpu, qf):
    """One list per query group, of very different lengths: the grid comes from the longest, so the
    other groups' later workgroups have no tile and write empty lists; ids past a group's own count
    are padding and get no output row."""
    for dim, k in ((130, 10), (768, 65), (1100, 256)):
        c = corpus(dim)
        rng = np.random.default_rng(10 * dim + qf)
        lens = (1500, 3, 300, 257)
        own = (qf, max(qf - 1, 1), 1, max(qf // 2, 1))
        groups = len(lens)
        lists = [row_list(c, rng, m) for m in lens]
        grp = np.zeros(groups, kx.GROUP_DESC)
        grp["off"] = np.concatenate([[0], np.cumsum(lens)[:-1]])
        grp["n_list"], grp["nq"] = lens, own
        # the groups' own queries are distinct; the padding id belongs to no group
        pad = c.nq - 1
        free = [int(x) for x in rng.permutation(pad)]
        qids = np.full(groups * qf, pad, np.int32)
        for y in range(groups):
            for j in range(own[y]):
                qids[y * qf + j] = free.pop()
        own_ids = [qids[y * qf:y * qf + own[y]].tolist() for y in range(groups)]
        lst = np.concatenate(lists[:groups])
        grid = kx.scan_grid_for(max(lens))
        part = np.full((groups, grid, qf, k), KFILL, np.uint64)
        assert kx.scan_raw(2, list=lst, grp=grp, nqf=qf, groups=groups, k=k, grid=grid, qids=qids, part=part,
                           **scan_args(c)) == 0
        for y in range(groups):
            tiles = [lists[y][t:t + 256].astype(np.int64) for t in range(0, lens[y], 256)]
            check_part(c, part[y], qids[y * qf:(y + 1) * qf], k, tiles, grid)
        assert (part[1, 1:] == KEY_NONE).all(), "workgroups without a tile write empty lists"
        out = np.full((c.nq, k), KFILL, np.uint64)
        assert kx.merge_parts_groups(part, grid, qids, qf, grp, k, out) == 0
        written = set()
        for y in range(groups):
            for q in own_ids[y]:
                assert np.array_equal(out[q], kx.topk_keys(c.all_keys[q][lists[y].astype(np.int64)], k)), (dim, y, q)
                written.add(q)
        for q in set(range(c.nq)) - written:
            assert (out[q] == KFILL).all(), "padding ids produce no output row"
    # rejected: no group, a width that is no template
    assert kx.scan_raw(2, list=lst, grp=grp, nqf=3, groups=groups, k=k, grid=grid, qids=qids, part=part,
                       **scan_args(c)) == INVALID
    assert kx.merge_parts_groups(part, grid, qids, 3, grp, k, out) == INVALID


def test_finalize(gpu):
    st = kx.consts()
    rng = np.random.default_rng(4)
    offset = (1 << 32) + (1 << 35) + 9
    for k, n in ((10, 1000), (10, 4), (10, 0), (1, 1), (130, 100), (256, 5000)):
        nq = 7
        d = np.sort(rng.uniform(0, 2, (nq, k)).astype(np.float32), axis=1)
        keys = kx.dist_key(d, rng.integers(0, max(n, 1), (nq, k)).astype(np.uint64))
        keys[1, k // 2:] = KEY_NONE          # a short list
        keys[2, 0] = KEY_NONE                # KEY_NONE inside the first places
        if k > 2:
            keys[3, 1] = KEY_NONE
        emit = rng.integers(0, 9000, nq).astype(np.uint32)
        n_q = np.array([n, 0, 1, k, k + 1, max(k - 1, 0), 3], np.uint32)
        for per_q, em in ((None, None), (n_q, emit), (None, emit)):
            idx, dist, cnt, status, cur = kx.finalize(keys, n, offset, emit_cnt=em, n_q=per_q)
            for q in range(nq):
                c = min(k, int(per_q[q]) if per_q is not None else n)
                assert cnt[q] == c
                has = (np.arange(k) < c) & (keys[q] != KEY_NONE)
                want_i = np.where(has, np.uint64(offset) + kc.key_row(keys[q]).astype(np.uint64), kx.IDX_NONE)
                want_d = np.where(has, kx.key_dist(keys[q]), POS_INF).astype(np.float32)
                assert np.array_equal(idx[q], want_i), (k, n, q)
                assert np.array_equal(dist[q].view(np.uint32), want_d.view(np.uint32)), (k, n, q)
            assert not status.any(), "the next search's status words"
            want_cur = np.full(st.st_words, 0x5A5A5A5A, np.uint32)
            if em is not None:
                want_cur[st.st_emitted] = emit.sum(dtype=np.uint32)
            assert np.array_equal(cur, want_cur)


def norm_flags(a):
    """The flags launch_row_norms ORs in, from the rows and the model's magnitudes."""
    st = kx.consts()
    m = kc.seq_norm_f32(a)
    f = 0
    if not np.isfinite(a).all():
        f |= st.row_non_finite
    if not np.isfinite(m).all():
        f |= st.row_norm_ovf
    with np.errstate(invalid="ignore"):
        if ((m != 0) & ((m < np.float32(1e-18)) | (m > np.float32(1e18)))).any():
            f |= st.row_norm_range
    return m, f


@pytest.mark.parametrize("dim", (40, 768, 1100))
def test_row_norms(gpu, dim):
    st = kx.consts()
    for n in (1, 255, 257, 1000):
        rng = np.random.default_rng(17 * dim + n)
        a = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
        if n > 4:
            a[2] = 0
        variants = {"clean": a}
        for name, row in (("nan", None), ("ovf", np.full(dim, 1e30)), ("tiny", np.full(dim, 1e-19 / np.sqrt(dim))),
                          ("huge", np.full(dim, 1e19 / np.sqrt(dim)))):
            b = a.copy()
            r = n - 1 if name in ("nan", "huge") else n // 2
            if row is None:
                b[r, dim // 3] = np.nan
            else:
                b[r] = row.astype(np.float32)
            variants[name] = b
        for name, b in variants.items():
            s = kc.slab(b)
            want, flags = norm_flags(b)
            for preset in (0, 8):
                na, got = kx.row_norms(s, n, dim, preset)
                assert np.array_equal(na[:n].view(np.uint32), want.view(np.uint32)), (name, n)
                assert np.isnan(na[n:]).all(), "padding rows are untouched"
                assert got == preset | flags, (name, n, got, flags)
            want_flag = {"clean": 0, "nan": st.row_non_finite | st.row_norm_ovf,
                         "ovf": st.row_norm_ovf | st.row_norm_range, "tiny": st.row_norm_range,
                         "huge": st.row_norm_range}[name]
            assert flags == want_flag, (name, flags)
