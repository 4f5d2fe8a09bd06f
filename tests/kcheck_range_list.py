"""Kernel-level checks of the masked range search: the ctypes loader of the test-only shim
(tests/kcheck/kcheck_range_list.cpp -> lib/libbsr_kcheck_range_list.so) and exact models of its
launchers: the range over row lists (csrc/k_exact.hip, launch_range_scan_list_groups), the routing
behind the threshold kernel (launch_range_route) and the segment scatter of a mask's row list
(csrc/k_prep.hip, launch_mask_groups_scatter_seg).

No model needs a tolerance: the in-range selection is kcheck_range.in_range_keys over the model's
exact distances, the routing and the scatter are integer bookkeeping.

tests/test_gpu_kernels_range_list.py compares the kernels with them.
"""
import ctypes
import os

import numpy as np

from kcheck_exact import GROUP_DESC, _fill, _rc, _struct, _vp  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "better-search-rag-rust_amd", "lib", "libbsr_kcheck_range_list.so")

# (the order of struct KcRangeList in kcheck_range_list.cpp)
_LIST_SPEC = (
    ("rows", "buf"), ("ld", "u32"), ("dim", "u32"), ("na", "buf"), ("qf32", "buf"), ("nb", "buf"), ("radius", "buf"),
    ("list", "buf"), ("grp", "buf"), ("groups", "u32"), ("qf", "u32"), ("qids", "buf"), ("keys", "buf"),
    ("rcnt", "buf"), ("cap", "u32"), ("grid", "u32"))
_List = _struct(_LIST_SPEC)

# struct MaskSegDesc { uint64_t off; uint32_t mask, first, n_list, pad_; }
SEG_DESC = np.dtype([("off", "<u8"), ("mask", "<u4"), ("first", "<u4"), ("n_list", "<u4"), ("pad_", "<u4")])

_lib = None


def lib() -> ctypes.CDLL:
    """libbsr_kcheck_range_list.so (raises if it has not been built).  Load it after the `gpu` fixture."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built (run __graft_entry__.build())")
        _lib = ctypes.CDLL(LIB_PATH)
        for f in ("kc_range_list_sizeof", "kc_seg_desc_sizeof"):
            getattr(_lib, f).restype = ctypes.c_uint32
        assert _lib.kc_range_list_sizeof() == ctypes.sizeof(_List), "struct layout differs from the shim's"
        assert _lib.kc_seg_desc_sizeof() == SEG_DESC.itemsize, "MaskSegDesc differs from the shim's"
    return _lib


def scan_list_raw(**kw):
    """launch_range_scan_list_groups; returns the hipError_t (0 = success)."""
    s = _List()
    keep = _fill(s, _LIST_SPEC, kw)
    rc = lib().kc_range_scan_list_groups(ctypes.byref(s))
    del keep
    return _rc(rc)


def route(to_list, radius, tau, scan_list, status):
    """launch_range_route in place over tau [nq], scan_list and status; returns the hipError_t."""
    nq = len(radius)
    to_list = np.ascontiguousarray(to_list, np.uint32)
    radius = np.ascontiguousarray(radius, np.float32)
    return _rc(lib().kc_range_route(_vp(to_list), _vp(radius), ctypes.c_uint32(nq), _vp(tau), _vp(scan_list),
                                    ctypes.c_uint64(scan_list.size), _vp(status)))


def scatter_seg(allow, n, dead, segs, list_words, fill=0xA5A5A5A5):
    """launch_mask_groups_count + launch_mask_groups_scatter_seg over allow [G][words]: (list
    [list_words], pattern-filled before; A [G])."""
    allow = np.ascontiguousarray(allow, np.uint64)
    n_masks, words = allow.shape
    lst = np.full(list_words, fill, np.uint32)
    a_out = np.zeros(n_masks, np.uint32)
    segs = np.ascontiguousarray(segs, SEG_DESC)
    rc = _rc(lib().kc_mask_scatter_seg(_vp(allow), ctypes.c_uint64(words), ctypes.c_uint32(n_masks), ctypes.c_uint64(n),
                                       _vp(dead), _vp(segs), ctypes.c_uint32(len(segs)), _vp(lst),
                                       ctypes.c_uint64(list_words), _vp(a_out)))
    assert rc == 0
    return lst, a_out


# ----------------------------------------------------------------------------------------
# Models
# ----------------------------------------------------------------------------------------
def route_model(to_list, radius, tau, listed, no_filter_count):
    """launch_range_route after launch_range_tau left (tau, listed = its scan list as a set,
    no_filter_count = its kStFail2): (tau, the set on the list, kStFail, kStFail2).  A routed query
    gets tau = +inf and joins the list unless it is there already or its radius is < 0 or NaN."""
    tau = np.array(tau, np.float32)
    out = set(listed)
    added = 0
    for q in range(len(radius)):
        if not to_list[q]:
            continue
        r = np.float32(radius[q])
        if r >= 0 and tau[q] < np.inf:  # (NaN compares false)
            assert q not in out
            out.add(q)
            added += 1
        tau[q] = np.inf
    return tau, out, len(listed) + added, no_filter_count + added


def seg_model(mask_bits, dead_bits, first, n_list):
    """The ids of rank first .. first + n_list - 1 among the allowed live rows, ascending."""
    live = np.flatnonzero(np.asarray(mask_bits, bool) & ~np.asarray(dead_bits, bool))
    return live[first:first + n_list].astype(np.uint32)
