"""Kernel-level checks of the id scoring: the ctypes loader of the test-only shim
(tests/kcheck/kcheck_score.cpp -> lib/libbsr_kcheck_score.so) and exact models of the contracts of
its two launchers in csrc/k_exact.hip: which slots of an id list are present, their aligned
distances and keys, and the rerank's order.

None of the models needs a tolerance: presence is integer arithmetic on the ids, the distance is
the exact model's (kcheck_exact.exact_distance, or the oracle's), the order plain u64 order of the
distance keys with equal keys dropped.

tests/test_score_models.py pins the models with hand-derived cases (CPU);
tests/test_gpu_kernels_score.py compares the kernels with them.
"""
import ctypes
import os

import numpy as np

from kcheck import KEY_NONE, _check, key_row  # noqa: F401
from kcheck_exact import IDX_NONE, POS_INF, _fill, _rc, _struct, _vp, dist_key, key_dist  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "better-search-rag-rust_amd", "lib", "libbsr_kcheck_score.so")

SCORE_MAX_IDS = 4096  # BSR_SCORE_MAX_IDS (include/bsr.h)

# (the order of struct KcScore in kcheck_score.cpp)
_SCORE_SPEC = (
    ("rows", "buf"), ("ld", "u32"), ("dim", "u32"), ("n", "u64"), ("offset", "u64"), ("na", "buf"), ("qf32", "buf"),
    ("nb", "buf"), ("dead", "buf"), ("ids", "buf"), ("m", "u32"), ("nq", "u32"), ("dist", "buf"), ("keys", "buf"),
    ("kcnt", "buf"), ("found", "buf"))
_Score = _struct(_SCORE_SPEC)

_lib = None


# ----------------------------------------------------------------------------------------
# Loader
# ----------------------------------------------------------------------------------------
def lib() -> ctypes.CDLL:
    """libbsr_kcheck_score.so (raises if it has not been built).  Load it after the `gpu` fixture."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built (run __graft_entry__.build())")
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.kc_score_max_ids.restype = ctypes.c_uint32
        _lib.kc_score_sizeof.restype = ctypes.c_uint32
        assert _lib.kc_score_sizeof() == ctypes.sizeof(_Score), "struct layout differs from the shim's"
    return _lib


def score_raw(**kw):
    """launch_score_ids through kc_score_ids; returns the hipError_t (0 = success)."""
    s = _Score()
    keep = _fill(s, _SCORE_SPEC, kw)
    rc = lib().kc_score_ids(ctypes.byref(s))
    del keep
    return _rc(rc)


def score_finish(keys, kcnt, k, offset):
    """launch_score_finish over keys [nq][m]: (rc, idx, dist, count), pattern-filled before."""
    nq, m = keys.shape
    idx = np.full((nq, max(k, 1)), 0x1234, np.uint64)
    dist = np.full((nq, max(k, 1)), np.nan, np.float32)
    cnt = np.full(nq, 0x5A5A5A5A, np.uint32)
    u32 = ctypes.c_uint32
    rc = lib().kc_score_finish(_vp(np.ascontiguousarray(keys, np.uint64)), _vp(np.ascontiguousarray(kcnt, np.uint32)),
                               u32(m), u32(nq), u32(k), ctypes.c_uint64(offset), _vp(idx), _vp(dist), _vp(cnt))
    return _rc(rc), idx, dist, cnt


# ----------------------------------------------------------------------------------------
# Models
# ----------------------------------------------------------------------------------------
def present_rows(ids, offset, n, dead=None):
    """(present [m] bool, row [m] int64) of a list of GLOBAL ids: present = offset <= id < offset + n
    and the row not deleted (dead: a bool array over the rows); row = id - offset where the id lies
    in the shard, 0 elsewhere.  Python integers: ids up to 2^64 - 1 neither wrap nor overflow."""
    ids = np.asarray(ids, np.uint64).ravel()
    present = np.zeros(len(ids), bool)
    row = np.zeros(len(ids), np.int64)
    for j, g in enumerate(ids.tolist()):
        if offset <= g < offset + n:
            row[j] = g - offset
            present[j] = dead is None or not bool(dead[g - offset])
    return present, row


def score_model(dist_rows, ids, offset, dead=None):
    """launch_score_ids for one query: dist_rows [n] = the exact distance of every row of the shard
    to the query.  Returns (dist [m]: dist_rows[id - offset] for a present slot, +inf otherwise;
    found: the present slots, a repeated id counted each time; keys: the present slots' distance
    keys, ascending -- one per slot, so a repeated id gives its key as often)."""
    dist_rows = np.asarray(dist_rows, np.float32)
    present, row = present_rows(ids, offset, len(dist_rows), dead)
    dist = np.full(len(row), np.inf, np.float32)
    dist[present] = dist_rows[row[present]]
    keys = np.sort(dist_key(dist[present], row[present].astype(np.uint64)))
    return dist, int(present.sum()), keys


def finish_model(keys, count, k, offset):
    """launch_score_finish for one query: the first `count` keys sorted as u64 -- (distance, row)
    order -- with equal keys dropped; the first k as (offset + row, distance), then (~0, +inf); the
    count = min(k, distinct keys)."""
    idx = np.full(k, IDX_NONE, np.uint64)
    dist = np.full(k, np.inf, np.float32)
    u = np.unique(np.asarray(keys, np.uint64)[:count])[:k]
    idx[:len(u)] = np.uint64(offset) + key_row(u).astype(np.uint64)
    dist[:len(u)] = key_dist(u)
    return idx, dist, len(u)


def rerank_model(ids, dist, k):
    """bsr_local_rerank_ids for one query from bsr_local_score_ids' own output: the slots with a
    finite distance (the present ones: a distance is at most 2), one per distinct id, in (distance
    asc, id asc) order; the first k, then (~0, +inf); the count."""
    ids = np.asarray(ids, np.uint64).ravel()
    dist = np.asarray(dist, np.float32).ravel()
    pairs = sorted({(float(d), int(g)) for d, g in zip(dist.tolist(), ids.tolist()) if d != np.inf})[:k]
    oi = np.full(k, IDX_NONE, np.uint64)
    od = np.full(k, np.inf, np.float32)
    for i, (d, g) in enumerate(pairs):
        oi[i] = g
        od[i] = np.float32(d)
    return oi, od, len(pairs)


def pack_dead(dead, n_words=None):
    """A bool array over the rows as the index's bitset: bit (i & 63) of word (i >> 6)."""
    dead = np.asarray(dead, bool)
    words = n_words or (len(dead) + 63) // 64
    bits = np.zeros(words * 64, np.uint8)
    bits[:len(dead)] = dead
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()
