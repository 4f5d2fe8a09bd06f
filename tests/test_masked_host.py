"""The masked search's host side, without a GPU: pack_allow_mask (the bool and the id forms, bit
order, tails, errors) and the argument checks of bsr_local_top_k_masked that need no device."""
import ctypes

import numpy as np
import pytest


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100, 128, 3001])
def test_pack_bool_and_id_forms_agree(bsr_mod, n):
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.3
    ids = np.flatnonzero(mask)
    a = bsr_mod.pack_allow_mask(n, mask=mask)
    b = bsr_mod.pack_allow_mask(n, ids=rng.permutation(ids))
    assert a.dtype == np.uint64 and a.shape == ((n + 63) // 64,)
    assert np.array_equal(a, b)
    # little-endian bit order: bit (i & 63) of word (i >> 6), tail bits zero
    want = np.zeros(((n + 63) // 64) * 8, np.uint8)
    want[:(n + 7) // 8] = np.packbits(mask, bitorder="little")
    assert np.array_equal(a.view(np.uint8), want)
    for i in range(n):
        assert bool((int(a[i >> 6]) >> (i & 63)) & 1) == bool(mask[i])
    if n % 64:
        assert int(a[-1]) >> (n % 64) == 0


def test_pack_empty_shard_and_empty_ids(bsr_mod):
    assert bsr_mod.pack_allow_mask(0, mask=np.zeros(0, bool)).shape == (0,)
    assert bsr_mod.pack_allow_mask(0, ids=[]).shape == (0,)
    w = bsr_mod.pack_allow_mask(130, ids=[])
    assert w.shape == (3,) and not w.any()


def test_pack_duplicate_ids(bsr_mod):
    w = bsr_mod.pack_allow_mask(200, ids=[5, 5, 199, 64, 5, 64])
    assert [int(x) for x in w] == [1 << 5, 1, 0, 1 << (199 - 192)]
    full = bsr_mod.pack_allow_mask(70, mask=np.ones(70, bool))
    assert [int(x) for x in full] == [2 ** 64 - 1, (1 << 6) - 1]


@pytest.mark.parametrize("ids", [[10], [-1], [3, 4, 10 ** 12]])
def test_pack_out_of_range_id_raises(bsr_mod, ids):
    with pytest.raises(bsr_mod.BsrError) as e:
        bsr_mod.pack_allow_mask(10, ids=ids)
    assert e.value.status == -1


def test_pack_argument_errors(bsr_mod):
    with pytest.raises(bsr_mod.BsrError):
        bsr_mod.pack_allow_mask(10)
    with pytest.raises(bsr_mod.BsrError):
        bsr_mod.pack_allow_mask(10, mask=np.ones(10, bool), ids=[1])
    with pytest.raises(bsr_mod.BsrError):
        bsr_mod.pack_allow_mask(10, mask=np.ones(9, bool))


def test_masked_search_null_index_is_invalid(bsr_mod):
    """A null index returns BSR_E_INVALID before any device is touched."""
    L = bsr_mod.lib()
    q = np.zeros((1, 8), np.float32)
    w = np.ones(1, np.uint64)
    oi, od, oc = np.zeros((1, 1), np.uint64), np.zeros((1, 1), np.float32), np.zeros(1, np.uint32)
    st = L.bsr_local_top_k_masked(None, q.ctypes.data, 1, 1, w.ctypes.data, 1, bsr_mod.BSR_MASK_AUTO,
                                  oi.ctypes.data, od.ctypes.data, oc.ctypes.data)
    assert st == -1
    assert b"null index" in L.bsr_last_error()


def test_masked_constants_mirror_header(bsr_mod):
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "bsr.h")).read()
    for name in ("BSR_MASK_AUTO", "BSR_MASK_LIST", "BSR_MASK_FILTER", "BSR_PATH_MASK_LIST", "BSR_PATH_MASK_FILTER"):
        m = re.search(r"#define\s+%s\s+(\d+)u" % name, src)
        assert m and int(m.group(1)) == getattr(bsr_mod, name), name
    assert isinstance(ctypes.c_uint64(1).value, int)
