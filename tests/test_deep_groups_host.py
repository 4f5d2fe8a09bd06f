"""The deep group search's host side, without a GPU: the argument checks of bsr_local_top_groups_deep
that return before any device is touched, in the header's order (the checks behind "not loaded" need
a loaded index: tests/test_gpu_deep_groups.py), and the Python wrapper's own checks."""
import ctypes

import numpy as np
import pytest

Q = np.zeros((1, 8), np.float32)
RG = np.zeros(4, np.uint32)
W = np.zeros(1, np.uint64)
QM = np.zeros(1, np.uint32)


def _p(a):
    return None if a is None else a.ctypes.data


def _call(L, ix, k, m=3, q=Q, nq=1, n_groups=4, allow=None, n_masks=0, qm=None, mode=0, outs=None):
    oi, od, og, orows, oc = outs
    return L.bsr_local_top_groups_deep(ix, _p(q), nq, k, m, _p(RG), 4, n_groups, _p(allow), 1, n_masks, _p(qm), mode,
                                       _p(oi), _p(od), _p(og), _p(orows), _p(oc))


@pytest.fixture()
def fake_index():
    """A non-null index pointer for the checks that return before the index is looked at (zeroed
    memory: `loaded` reads false, so a check that let the call through would end in BSR_E_STATE)."""
    buf = ctypes.create_string_buffer(1 << 16)
    return ctypes.c_void_p(ctypes.addressof(buf)), buf


def test_symbol_exported(bsr_mod):
    assert hasattr(bsr_mod.lib(), "bsr_local_top_groups_deep") and bsr_mod.BSR_DEEP_GROUPS_MAX_SLOTS == 8192


@pytest.mark.parametrize("kw,msg", [
    (dict(ix=None, k=5), b"null index"),
    (dict(k=5, m=0), b"group_size=0 outside"),
    (dict(k=5, m=65), b"group_size=65 outside"),
    (dict(k=1024, m=9), b"k * group_size = 1024 * 9 exceeds 8192"),
    (dict(k=129, m=64), b"exceeds 8192"),
    (dict(k=0), b"k=0 outside"),
    (dict(k=1025, m=1), b"k=1025 outside"),
    (dict(k=5, n_groups=0), b"n_groups = 0"),
    (dict(k=5, n_masks=1), b"without allow masks"),
    (dict(k=5, qm=QM), b"without allow masks"),
    (dict(k=5, allow=W), b"n_masks = 0 with allow masks"),
    (dict(k=5, allow=W, n_masks=2), b"null query_mask with n_masks = 2"),
    (dict(k=5, mode=3), b"unknown mask mode 3"),
    (dict(k=5, q=None), b"null queries"),
    (dict(k=5, outs=0), b"null output"),
    (dict(k=5, outs=1), b"null output"),
    (dict(k=5, outs=4), b"null output"),
])
def test_checks_before_any_device(bsr_mod, fake_index, kw, msg):
    L = bsr_mod.lib()
    outs = [np.full((1, 8192), 7, np.uint64), np.full((1, 8192), 7, np.float32), np.full((1, 1024), 7, np.uint32),
            np.full((1, 1024), 7, np.uint32), np.full(1, 7, np.uint32)]
    passed = list(outs)
    if "outs" in kw:
        passed[kw.pop("outs")] = None
    kw.setdefault("ix", fake_index[0])
    assert _call(L, outs=passed, **kw) == -1 and msg in L.bsr_last_error()
    assert all((a == 7).all() for a in outs)
    # past every check above (out_group and out_rows are nullable; both slot limits met exactly, with
    # and without masks): the index is looked at (not loaded), still before any device
    if kw["ix"] is not None:
        passed = [outs[0], outs[1], None, None, outs[4]]
        assert _call(L, fake_index[0], 1024, m=8, outs=passed) == -7
        assert _call(L, fake_index[0], 128, m=64, allow=W, n_masks=2, qm=QM, mode=2, outs=passed) == -7
        assert _call(L, fake_index[0], 1024, m=1, nq=0, q=None, outs=[None] * 5) == -7
        assert all((a == 7).all() for a in outs)


def test_wrapper_checks(bsr_mod):
    ix = bsr_mod.Index.__new__(bsr_mod.Index)
    ix.dim = 8
    for kw in (dict(k=0), dict(k=1025, group_size=1), dict(k=5, group_size=0), dict(k=5, group_size=65),
               dict(k=1024, group_size=9), dict(k=5, n_groups=0), dict(k=5, row_group=np.array([0.5])),
               dict(k=5, allow_mask=np.ones(4, bool), query_mask=[0]), dict(k=5, allow_masks=np.ones((1, 4), bool))):
        kw.setdefault("row_group", RG)
        kw.setdefault("group_size", 3)
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.deep_group_search(Q, **kw)
        assert e.value.status == -1
