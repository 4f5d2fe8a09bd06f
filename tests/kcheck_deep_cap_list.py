"""Kernel-level checks of the deep capped list scan: the ctypes loader of the test-only shim
(tests/kcheck/kcheck_deep_cap_list.cpp -> lib/libbsr_kcheck_deep_cap_list.so).  The model is
kcheck_cap's cap_model over kcheck_exact's distances of the listed rows."""
import ctypes
import os

import numpy as np

import kcheck_exact as kx

LIB_PATH = os.path.join(kx.ROOT, "better-search-rag-rust_amd", "lib", "libbsr_kcheck_deep_cap_list.so")
SCAN_QF = 2  # kDeepCapScanQF
_lib = None


def lib() -> ctypes.CDLL:
    """libbsr_kcheck_deep_cap_list.so (raises if it has not been built).  Load it after the `gpu` fixture."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built (run __graft_entry__.build())")
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.kc_deep_cap_scan_qf.restype = ctypes.c_uint32
        assert _lib.kc_deep_cap_scan_qf() == SCAN_QF
    return _lib


def scan(corp, row_group, lst, segs, qids, nq_own, k, m, grid, offset, carry=None):
    """One query group (qids, the first nq_own its own) over the segments [(off, len)] of the row list
    lst: launch_deep_cap_scan_list on `grid` workgroups (0: scan_grid_for of the segment) and the
    capped merge into the carry per segment, launch_deep_cap_finish at the end.  carry [nq][k] starts
    as given (None: empty).  The outputs start as a pattern.  Returns (carry, idx, dist, count, group)."""
    nq = corp.nq
    carry = np.full((nq, k), kx.KEY_NONE, np.uint64) if carry is None else np.ascontiguousarray(carry, np.uint64)
    idx, dist = np.full((nq, k), 0x1234, np.uint64), np.full((nq, k), -3.0, np.float32)
    grp, cnt = np.full((nq, k), 0x5A5A5A5A, np.uint32), np.full(nq, 0x5A5A, np.uint32)
    off = np.array([s[0] for s in segs], np.uint64)
    ln = np.array([s[1] for s in segs], np.uint32)
    qids = np.ascontiguousarray(qids, np.int32)
    lst = np.ascontiguousarray(lst if len(lst) else [0], np.uint32)  # (an empty list: a valid pointer all the same)
    rg = np.zeros(corp.rows.shape[0], np.uint32)
    rg[:corp.n] = row_group
    assert lst.max() < corp.n and all(o + n <= len(lst) for o, n in segs)  # (what the kernel indexes)
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, kx._vp
    rc = lib().kc_deep_cap_scan_list(vp(corp.rows), u64(corp.rows.shape[0]), u32(corp.ld), u32(corp.dim), vp(corp.na),
                                     vp(rg), vp(corp.qf32), vp(corp.nb), u32(nq), vp(lst), u64(len(lst)), vp(off),
                                     vp(ln), u32(len(segs)), vp(qids), u32(len(qids)), u32(nq_own), u32(k), u32(m),
                                     u32(grid), u64(offset), vp(carry), vp(idx), vp(dist), vp(grp), vp(cnt))
    assert rc == 0, f"hipError_t {rc}"
    return carry, idx, dist, cnt, grp
