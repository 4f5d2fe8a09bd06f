"""The grouped masked search's host side, without a GPU: the exported symbol, the argument check
that needs no device, the path constant, and pack_allow_masks against pack_allow_mask."""
import os
import re

import numpy as np
import pytest


def test_symbol_is_exported(bsr_mod):
    assert hasattr(bsr_mod.lib(), "bsr_local_top_k_masked_groups")


def test_null_index_is_invalid(bsr_mod):
    """A null index returns BSR_E_INVALID with a message, before any device is touched."""
    L = bsr_mod.lib()
    q = np.zeros((1, 8), np.float32)
    w = np.ones((1, 1), np.uint64)
    qm = np.zeros(1, np.uint32)
    oi, od, oc = np.zeros((1, 1), np.uint64), np.zeros((1, 1), np.float32), np.zeros(1, np.uint32)
    st = L.bsr_local_top_k_masked_groups(None, q.ctypes.data, 1, 1, w.ctypes.data, 1, 1, qm.ctypes.data,
                                         bsr_mod.BSR_MASK_AUTO, oi.ctypes.data, od.ctypes.data, oc.ctypes.data)
    assert st == -1
    assert b"null index" in L.bsr_last_error()


def test_path_constant_mirrors_header(bsr_mod):
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "bsr.h")).read()
    m = re.search(r"#define\s+BSR_PATH_MASK_GROUPS\s+(\d+)u", src)
    assert m and int(m.group(1)) == bsr_mod.BSR_PATH_MASK_GROUPS == 512


@pytest.mark.parametrize("n", [1, 64, 65, 130, 3001])
def test_pack_masks_agrees_row_by_row(bsr_mod, n):
    rng = np.random.default_rng(n)
    masks = rng.random((5, n)) < rng.random((5, 1))
    masks[3] = False
    a = bsr_mod.pack_allow_masks(n, masks=masks)
    b = bsr_mod.pack_allow_masks(n, ids=[rng.permutation(np.flatnonzero(m)) for m in masks])
    assert a.dtype == np.uint64 and a.shape == (5, (n + 63) // 64) and a.flags.c_contiguous
    assert np.array_equal(a, b)
    for g in range(5):
        assert np.array_equal(a[g], bsr_mod.pack_allow_mask(n, mask=masks[g])), g


def test_pack_masks_no_masks_and_empty_shard(bsr_mod):
    assert bsr_mod.pack_allow_masks(100, ids=[]).shape == (0, 2)
    assert bsr_mod.pack_allow_masks(0, masks=np.zeros((3, 0), bool)).shape == (3, 0)


def test_pack_masks_argument_errors(bsr_mod):
    ok = np.ones((2, 10), bool)
    for kw in ({}, {"masks": ok, "ids": [[1], [2]]}, {"masks": np.ones((2, 9), bool)}, {"masks": np.ones(10, bool)},
               {"masks": ok.astype(np.uint8)}, {"ids": [[1], [10]]}, {"ids": [[-1]]}):
        with pytest.raises(bsr_mod.BsrError) as e:
            bsr_mod.pack_allow_masks(10, **kw)
        assert e.value.status == -1, kw
