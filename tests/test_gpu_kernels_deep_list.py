"""launch_deep_scan_list (csrc/k_exact.hip) through its test-only shim (tests/kcheck/kcheck_deep_list.cpp
-> lib/libbsr_kcheck_deep_list.so): one query group over one list segment, or over two segments of one
list with the carry between them, bit for bit against the model -- kcheck_exact's distances of the
listed rows, ordered by (distance, row), the first k."""
import ctypes
import os

import numpy as np
import pytest

import kcheck_exact as kx

pytestmark = pytest.mark.gpu

F, U64 = np.float32, np.uint64
OFFSET = 1 << 33
LIB = os.path.join(kx.ROOT, "better-search-rag-rust_amd", "lib", "libbsr_kcheck_deep_list.so")
NQ = 6

_corpora = {}


def corpus(dim):
    if dim not in _corpora:
        c = kx.Corpus(5300, dim, NQ, 2500 + dim)
        c.all_dist = [c.dist(q) for q in range(c.nq)]
        _corpora[dim] = c
    return _corpora[dim]


def scan(corp, lst, segs, qids, nq_own, k, grid):
    lib = ctypes.CDLL(LIB)
    lib.kc_deep_scan_buf.restype = ctypes.c_uint32
    assert lib.kc_deep_scan_buf() == 2 * 1024 + 256
    nq = corp.nq
    carry = np.full((nq, k), kx.KEY_NONE, U64)
    idx, dist, cnt = np.full((nq, k), 0x1234, U64), np.full((nq, k), -3.0, F), np.full(nq, 0x5A5A, np.uint32)
    off = np.array([s[0] for s in segs], U64)
    ln = np.array([s[1] for s in segs], np.uint32)
    qids = np.ascontiguousarray(qids, np.int32)
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, kx._vp
    rc = lib.kc_deep_scan_list(vp(corp.rows), u64(corp.rows.shape[0]), u32(corp.ld), u32(corp.dim), vp(corp.na),
                               vp(corp.qf32), vp(corp.nb), u32(nq), vp(lst), u64(len(lst)), vp(off), vp(ln),
                               u32(len(segs)), vp(qids), u32(len(qids)), u32(nq_own), u32(k), u32(grid), u64(OFFSET),
                               vp(carry), vp(idx), vp(dist), vp(cnt))
    assert rc == 0, f"hipError_t {rc}"
    return carry, idx, dist, cnt


@pytest.mark.parametrize("dim", (64, 130))
@pytest.mark.parametrize("qf,nq_own", ((1, 1), (2, 2), (4, 3), (4, 4)))
@pytest.mark.parametrize("k", (1, 1024))
@pytest.mark.parametrize("length", (1, 255, 257, 5000))
def test_deep_scan_list(gpu, dim, qf, nq_own, k, length):
    corp = corpus(dim)
    rng = np.random.default_rng(length + k + qf)
    special = np.array(corp.special_rows())[:length // 2]  # (identical rows, zero rows, the run of ties)
    rest = rng.choice(np.setdiff1d(np.arange(corp.n), special), length - len(special), replace=False)
    rows = np.sort(np.concatenate([special, rest])).astype(np.uint32)
    own = [0] + [int(x) for x in rng.permutation(np.arange(1, NQ))[:nq_own - 1]]
    qids = own + [own[0]] * (qf - nq_own)
    cut = length // 3
    # grid 0: one workgroup a tile; 2 (the long list): ten tiles a workgroup, so that a full buffer is cut
    for segs, grid in [([(0, length)], 0)] + ([([(0, cut), (cut, length - cut)], 0)] if cut else []) + \
            ([([(0, length)], 2)] if length == 5000 else []):
        carry, idx, dist, cnt = scan(corp, rows, segs, qids, nq_own, k, grid)
        for q in range(NQ):
            want = kx.topk_keys(kx.dist_key(corp.all_dist[q][rows], rows), k) if q in own else np.full(k, kx.KEY_NONE, U64)
            m = int((want != kx.KEY_NONE).sum())
            assert np.array_equal(carry[q], want), (len(segs), q)
            assert cnt[q] == m == (min(k, length) if q in own else 0)
            assert np.array_equal(idx[q, :m], U64(OFFSET) + (want[:m] & U64(0xFFFFFFFF))) and (idx[q, m:] == kx.IDX_NONE).all()
            assert np.array_equal(dist[q, :m].view(np.uint32), kx.key_dist(want[:m]).view(np.uint32))
            assert np.isposinf(dist[q, m:]).all()
