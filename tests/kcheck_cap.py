"""Kernel-level checks of the capped search: the ctypes loader of the test-only shim
(tests/kcheck/kcheck_cap.cpp -> lib/libbsr_kcheck_cap.so) and the exact model of the contract of
bsr_local_top_k_capped and bsr_global_top_k_capped (include/bsr.h).

The model needs no tolerance: from the full distance vector of a query over the stored rows (the
reference's bits, oracle.np_cosine_distances) it drops the deleted and the disallowed rows, sorts
by (distance, index), keeps a row while its group's kept count is below m and takes the first k.
cap_model_ranked is the same contract said another way (rank within the group below m, then the k
smallest); the model tests compare the two.

tests/test_cap_models.py pins the model with hand-worked cases (CPU); tests/test_cap_host.py uses it
for the host merge; tests/test_gpu_kernels_cap.py compares the kernels with it, tests/test_gpu_cap.py
whole calls."""
import ctypes
import os

import numpy as np

from kcheck_exact import IDX_NONE, POS_INF, _fill, _rc, _struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "better-search-rag-rust_amd", "lib", "libbsr_kcheck_cap.so")

MAX_FETCH = 256     # kCollapseMaxFetch = BSR_MAX_K
SCAN_QF = 8         # kScanQF
MAX_PER_GROUP = 16  # kCapMaxPerGroup = BSR_CAP_MAX_PER_GROUP
GROUP_NONE = np.uint32(0xFFFFFFFF)
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)

# (the order of struct KcCapWalk / KcCapScan in kcheck_cap.cpp)
_WALK_SPEC = (
    ("cand_idx", "buf"), ("cand_dist", "buf"), ("cand_cnt", "buf"), ("nq", "u32"), ("fetch_k", "u32"), ("k", "u32"),
    ("per_group", "u32"), ("n", "u64"), ("offset", "u64"), ("row_group", "buf"), ("out_idx", "buf"),
    ("out_dist", "buf"), ("out_group", "buf"), ("out_count", "buf"), ("fail", "buf"), ("fail_cnt", "buf"))
_SCAN_SPEC = (
    ("rows", "buf"), ("ld", "u32"), ("dim", "u32"), ("n", "u64"), ("offset", "u64"), ("na", "buf"), ("qf32", "buf"),
    ("nb", "buf"), ("dead", "buf"), ("row_group", "buf"), ("n_groups", "u32"), ("nqf", "u32"), ("allow", "buf"),
    ("allow_words", "u64"), ("query_mask", "buf"), ("qids", "buf"), ("k", "u32"), ("grid", "u32"),
    ("sel_grid", "u32"), ("m", "u32"), ("best", "buf"), ("part", "buf"), ("keys", "buf"), ("out_idx", "buf"),
    ("out_dist", "buf"), ("out_group", "buf"), ("out_count", "buf"))
_Walk, _Scan = _struct(_WALK_SPEC), _struct(_SCAN_SPEC)
_lib = None


def lib() -> ctypes.CDLL:
    """libbsr_kcheck_cap.so (raises if it has not been built).  Load it after the `gpu` fixture."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built (run __graft_entry__.build())")
        _lib = ctypes.CDLL(LIB_PATH)
        for f in ("kc_cap_max_fetch", "kc_cap_scan_qf", "kc_cap_max_per_group", "kc_cap_select_grid",
                  "kc_cap_scan_grid"):
            getattr(_lib, f).restype = ctypes.c_uint32
        _lib.kc_cap_select_grid.argtypes = [ctypes.c_uint32]
        _lib.kc_cap_scan_grid.argtypes = [ctypes.c_uint64]
        _lib.kc_cap_walk.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        _lib.kc_cap_scan.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        sizes = (ctypes.c_uint32 * 2)()
        _lib.kc_cap_sizes(sizes)
        assert list(sizes) == [ctypes.sizeof(_Walk), ctypes.sizeof(_Scan)], "struct layouts differ from the shim's"
        assert _lib.kc_cap_max_fetch() == MAX_FETCH and _lib.kc_cap_scan_qf() == SCAN_QF
        assert _lib.kc_cap_max_per_group() == MAX_PER_GROUP
    return _lib


def walk(cand_idx, cand_dist, cand_cnt, k, per_group, n, offset, row_group, with_group=True, collapse=False):
    """launch_cap_walk (collapse: launch_collapse_walk, per_group unused) over the lists cand_idx /
    cand_dist [nq][fetch_k], cand_cnt [nq]; the outputs and the fail list start as a pattern, the
    fail count as 0.  Returns (rc, idx [nq][k], dist, count, group or None, fail list [nq], fail
    count)."""
    cand_idx = np.ascontiguousarray(cand_idx, np.uint64)
    cand_dist = np.ascontiguousarray(cand_dist, np.float32)
    cand_cnt = np.ascontiguousarray(cand_cnt, np.uint32)
    row_group = np.ascontiguousarray(row_group, np.uint32)
    nq, fetch_k = cand_idx.shape
    assert cand_dist.shape == (nq, fetch_k) and cand_cnt.shape == (nq,) and row_group.shape == (n,)
    idx = np.full((nq, max(k, 1)), 0x1234, np.uint64)
    dist = np.full((nq, max(k, 1)), np.nan, np.float32)
    grp = np.full((nq, max(k, 1)), 0x5A5A5A5A, np.uint32) if with_group else None
    cnt = np.full(nq, 0x5A5A5A5A, np.uint32)
    fail = np.full(nq, 0x5A5A5A5A, np.uint32)
    fail_cnt = np.zeros(1, np.uint32)
    s = _Walk()
    keep = _fill(s, _WALK_SPEC, dict(cand_idx=cand_idx, cand_dist=cand_dist, cand_cnt=cand_cnt, nq=nq, fetch_k=fetch_k,
                                     k=k, per_group=per_group, n=n, offset=offset, row_group=row_group, out_idx=idx,
                                     out_dist=dist, out_group=grp, out_count=cnt, fail=fail, fail_cnt=fail_cnt))
    rc = lib().kc_cap_walk(ctypes.byref(s), 1 if collapse else 0)
    del keep
    return _rc(rc), idx, dist, cnt, grp, fail, int(fail_cnt[0])


def scan(rows, dim, n, offset, na, qf32, nb, row_group, n_groups, qids, nqf, k, m, dead=None, allow=None,
         query_mask=None, collapse=False, grid=None):
    """One round of the capped group scan over the slab rows [n_pad][ld] for the launch's nqf queries
    (qids padded to the template width): the tables, launch_cap_scan (collapse: launch_collapse_scan,
    m = 1; on `grid` workgroups, None: scan_grid_for(n)), launch_collapse_select over m * n_groups
    entries, launch_merge_parts,
    launch_collapse_finish.  The outputs [nq_all][k] (nq_all = len(qf32)) are indexed by query id and
    start as a pattern.  Returns (rc, idx, dist, count, group, best [width][n_groups][m])."""
    L = lib()
    qids = np.ascontiguousarray(qids, np.int32)
    row_group = np.ascontiguousarray(row_group, np.uint32)
    assert rows.dtype == np.float32 and rows.flags.c_contiguous and rows.shape[0] >= n and row_group.shape == (n,)
    assert rows.shape[0] % 256 == 0 and (n == 0 or int(row_group.max()) < n_groups)  # (what the kernel indexes)
    nq_all = qf32.shape[0]
    width = 1 if nqf <= 1 else 2 if nqf <= 2 else 4 if nqf <= 4 else 8
    assert len(qids) >= width and qids.max() < nq_all and qids.min() >= 0
    sel_grid = L.kc_cap_select_grid(m * n_groups)
    idx = np.full((nq_all, k), 0x1234, np.uint64)
    dist = np.full((nq_all, k), np.nan, np.float32)
    grp = np.full((nq_all, k), 0x5A5A5A5A, np.uint32)
    cnt = np.full(nq_all, 0x5A5A5A5A, np.uint32)
    best = np.full((width, n_groups, max(m, 1)), KEY_NONE, np.uint64)  # (the padding slots too: they stay empty)
    part = np.full(sel_grid * width * k, 0x77, np.uint64)
    keys = np.full((nq_all, k), 0x77, np.uint64)
    words = 0
    if allow is not None:
        allow = np.ascontiguousarray(allow, np.uint64)
        words = allow.shape[-1]
        assert words * 64 >= n
    s = _Scan()
    keep = _fill(s, _SCAN_SPEC, dict(
        rows=rows, ld=rows.shape[1], dim=dim, n=n, offset=offset, na=np.ascontiguousarray(na, np.float32),
        qf32=np.ascontiguousarray(qf32, np.float32), nb=np.ascontiguousarray(nb, np.float32), dead=dead,
        row_group=row_group, n_groups=n_groups, nqf=nqf, allow=allow, allow_words=words,
        query_mask=None if query_mask is None else np.ascontiguousarray(query_mask, np.uint32), qids=qids, k=k,
        grid=L.kc_cap_scan_grid(n) if grid is None else grid, sel_grid=sel_grid, m=m, best=best, part=part, keys=keys,
        out_idx=idx, out_dist=dist, out_group=grp, out_count=cnt))
    rc = L.kc_cap_scan(ctypes.byref(s), 1 if collapse else 0)
    del keep
    return _rc(rc), idx, dist, cnt, grp, best


# ----------------------------------------------------------------------------------------
# The model
# ----------------------------------------------------------------------------------------
def _ordered_rows(dist, n, live, allowed):
    ok = np.ones(n, bool)
    if live is not None:
        ok &= np.asarray(live, bool)
    if allowed is not None:
        ok &= np.asarray(allowed, bool)
    rows = np.flatnonzero(ok)
    return rows[np.lexsort((rows, dist[rows]))]  # (distance asc, index asc)


def _result(kept, dist, row_group, k, offset):
    idx = np.full(k, IDX_NONE, np.uint64)
    od = np.full(k, POS_INF, np.float32)
    og = np.full(k, GROUP_NONE, np.uint32)
    c = len(kept)
    h = np.asarray(kept, np.int64)
    idx[:c] = (h + offset).astype(np.uint64)
    od[:c] = dist[h]
    og[:c] = row_group[h]
    return idx, od, og, c


def cap_model(dist, row_group, k, m, live=None, allowed=None, offset=0):
    """The contract for one query: dist [n] the reference's distances of the stored rows, row_group
    [n] their groups, live / allowed [n] bool (None: every row).  The live allowed rows in (distance
    asc, index asc) order; a row is kept while fewer than m rows of its group were kept before it;
    the first k kept.  Returns (idx [k] u64, dist [k] f32, group [k] u32, count) with the (~0, +inf,
    ~0u) tail."""
    dist = np.asarray(dist, np.float32)
    row_group = np.asarray(row_group, np.int64)
    n = len(dist)
    assert row_group.shape == (n,) and m >= 1 and k >= 1
    kept, have = [], {}
    for r in _ordered_rows(dist, n, live, allowed):
        g = int(row_group[r])
        if have.get(g, 0) < m:
            have[g] = have.get(g, 0) + 1
            kept.append(int(r))
            if len(kept) == k:
                break
    return _result(kept, dist, row_group, k, offset)


def cap_model_ranked(dist, row_group, k, m, live=None, allowed=None, offset=0):
    """The same contract, the other way round: the rank of a row within its group (by (distance,
    index) among the live allowed rows) is below m; of those rows the k smallest."""
    dist = np.asarray(dist, np.float32)
    row_group = np.asarray(row_group, np.int64)
    n = len(dist)
    order = _ordered_rows(dist, n, live, allowed)
    cand = []
    for g in np.unique(row_group[order]):
        cand.extend(order[row_group[order] == g][:m].tolist())  # (order is sorted: the group's m first)
    cand = np.asarray(sorted(cand, key=lambda r: (dist[r], r))[:k], np.int64)
    return _result(cand, dist, row_group, k, offset)


def cap_batch(dists, row_group, k, m, live=None, allowed=None, offset=0):
    """cap_model for every query: dists [nq][n]; allowed None, [n], or one array per query.
    Returns (idx [nq][k], dist, count [nq], group)."""
    nq = len(dists)
    per_query = allowed is not None and (isinstance(allowed, list) or np.asarray(allowed).ndim == 2)
    out = [cap_model(dists[q], row_group, k, m, live, allowed[q] if per_query else allowed, offset) for q in range(nq)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]),
            np.array([o[3] for o in out], np.uint32), np.stack([o[2] for o in out]))


def merge_model(idx, dist, group, count, k, m):
    """bsr_global_top_k_capped for one query: idx / dist / group [L][k_in], count [L].  The listed
    entries ordered by (distance, index), deduplicated by index, capped at m per group, the first k.
    Returns (idx [k], dist [k], group [k], count)."""
    ent = {}
    for l in range(len(count)):
        for i in range(min(int(count[l]), idx.shape[1])):
            key = (np.float32(dist[l, i]), int(idx[l, i]))
            ent.setdefault(key, int(group[l, i]))
    oi = np.full(k, IDX_NONE, np.uint64)
    od = np.full(k, POS_INF, np.float32)
    og = np.full(k, GROUP_NONE, np.uint32)
    c, have, seen = 0, {}, set()
    for (d, i) in sorted(ent):
        g = ent[(d, i)]
        if i in seen or have.get(g, 0) >= m:
            continue
        seen.add(i)
        have[g] = have.get(g, 0) + 1
        oi[c], od[c], og[c] = i, d, g
        c += 1
        if c == k:
            break
    return oi, od, og, c


def cascade_sim(keys, m, rng):
    """The capped scan's insert (cap_insert in k_exact.hip) for every key, each atomic min one
    indivisible step, the steps of different inserts interleaved at random; the plain reads ahead of
    the cascade see the table of that moment or of any earlier one (a stale read).  Returns the
    final entries, sorted."""
    none = int(KEY_NONE)
    e = [none] * m
    past = [list(e)]  # every state the table went through
    # an insert's state: [value carried, next entry]; not started: None
    pending = [[int(x), None] for x in keys]
    while pending:
        j = int(rng.integers(len(pending)))
        st = pending[j]
        if st[1] is None:
            seen = past[int(rng.integers(len(past)))]
            if not any(st[0] < x for x in seen):  # (the plain reads: below no entry -> skipped)
                pending.pop(j)
                continue
            st[1] = 0
            continue
        s = st[1]
        old = e[s]
        e[s] = min(old, st[0])  # atomicMin
        past.append(list(e))
        if old == none or s + 1 == m:
            pending.pop(j)
            continue
        st[0] = max(old, st[0])
        st[1] = s + 1
    return sorted(e)
