"""Kernel-level checks of the deep MMR selection: the ctypes loader of the test-only shim
(tests/kcheck/kcheck_deep_mmr.cpp -> lib/libbsr_kcheck_deep_mmr.so).  The model is kcheck_mmr's
(mmr_model, mmr_outputs): the contract is bsr_local_top_k_mmr's, generic in the list length."""
import ctypes
import os

import numpy as np

import kcheck_mmr as km
from kcheck_exact import _fill, _rc, _struct

LIB_PATH = os.path.join(km.ROOT, "better-search-rag-rust_amd", "lib", "libbsr_kcheck_deep_mmr.so")
MAX_FETCH, MAX_PICKS = 1024, 256  # kMmrDeepMaxFetch = BSR_DEEP_MAX_K, kMmrDeepMaxPicks = BSR_DEEP_MMR_MAX_PICKS

# struct KcDeepMmr in kcheck_deep_mmr.cpp: KcMmr's fields, then the pair counter
_SPEC = km._MMR_SPEC + (("pairs", "buf"),)
_DeepMmr = type("KcDeepMmr", (ctypes.Structure,),
                {"_fields_": list(km._Mmr._fields_) + list(_struct((("pairs", "buf"),))._fields_)})
_lib = None


def lib() -> ctypes.CDLL:
    """libbsr_kcheck_deep_mmr.so (raises if it has not been built).  Load it after the `gpu` fixture."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built (run __graft_entry__.build())")
        _lib = ctypes.CDLL(LIB_PATH)
        for f in (_lib.kc_deep_mmr_sizeof, _lib.kc_deep_mmr_max_fetch, _lib.kc_deep_mmr_max_picks):
            f.restype = ctypes.c_uint32
        assert _lib.kc_deep_mmr_sizeof() == ctypes.sizeof(_DeepMmr), "struct layout differs from the shim's"
        assert _lib.kc_deep_mmr_max_fetch() == MAX_FETCH and _lib.kc_deep_mmr_max_picks() == MAX_PICKS
    return _lib


def deep_mmr_select(rows, dim, n, offset, na, cand_idx, cand_dist, cand_cnt, k, lam, with_rank=True):
    """launch_mmr_deep_select over the slab rows [n_pad][ld] and the lists cand_idx / cand_dist
    [nq][fetch_k], cand_cnt [nq]; the outputs start as a pattern, the pair counter as 0.  Returns (rc,
    idx [nq][k], dist, rank or None, count, pairs)."""
    cand_idx = np.ascontiguousarray(cand_idx, np.uint64)
    nq, fetch_k = cand_idx.shape
    assert rows.dtype == np.float32 and rows.flags.c_contiguous and rows.shape[0] >= n and na.shape[0] >= n
    idx = np.full((nq, max(k, 1)), 0x1234, np.uint64)
    dist = np.full((nq, max(k, 1)), np.nan, np.float32)
    rank = np.full((nq, max(k, 1)), 0x5A5A5A5A, np.uint32) if with_rank else None
    cnt = np.full(nq, 0x5A5A5A5A, np.uint32)
    pairs = np.zeros(1, np.uint64)
    s = _DeepMmr()
    kw = dict(rows=rows, ld=rows.shape[1], dim=dim, n=n, offset=offset, na=np.ascontiguousarray(na, np.float32),
              cand_idx=cand_idx, cand_dist=np.ascontiguousarray(cand_dist, np.float32).reshape(nq, fetch_k),
              cand_cnt=np.ascontiguousarray(cand_cnt, np.uint32).reshape(nq), nq=nq, fetch_k=fetch_k, k=k,
              out_idx=idx, out_dist=dist, out_rank=rank, out_count=cnt, pairs=pairs)
    keep = _fill(s, tuple(x for x in _SPEC if x[0] != "lam"), kw)
    s.lam = float(lam)
    rc = lib().kc_deep_mmr_select(ctypes.byref(s))
    del keep
    return _rc(rc), idx, dist, rank, cnt, int(pairs[0])
