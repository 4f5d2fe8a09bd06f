"""The masked deep search's host side, without a GPU: the argument checks of
bsr_local_top_k_deep_masked that return before any device is touched, in the header's order, and the
Python wrapper's handling of the mask arguments."""
import ctypes

import numpy as np
import pytest

Q = np.zeros((1, 8), np.float32)
W = np.zeros((2, 1), np.uint64)
QM = np.zeros(1, np.uint32)


def _p(a):
    return None if a is None else a.ctypes.data


def _call(L, ix, k, q=Q, nq=1, allow=W, n_masks=1, qmask=None, mode=0, outs=None):
    oi, od, oc = outs
    return L.bsr_local_top_k_deep_masked(ix, _p(q), nq, k, _p(allow), 1, n_masks, _p(qmask), mode, _p(oi), _p(od), _p(oc))


@pytest.fixture()
def fake_index():
    """A non-null index pointer for the checks that return before the index is looked at (zeroed
    memory: `loaded` reads false, so a check that let the call through would end in BSR_E_STATE)."""
    buf = ctypes.create_string_buffer(1 << 16)
    return ctypes.c_void_p(ctypes.addressof(buf)), buf


@pytest.mark.parametrize("kw,msg", [
    (dict(ix=None, k=5), b"null index"),
    (dict(k=0), b"k=0 outside"),
    (dict(k=1025), b"k=1025 outside"),
    (dict(k=5, n_masks=0), b"n_masks = 0"),
    (dict(k=5, mode=3), b"unknown mask mode"),
    (dict(k=5, q=None), b"null queries"),
    (dict(k=5, outs=2), b"null output"),
    (dict(k=5, allow=None), b"null allow"),
    (dict(k=5, n_masks=2), b"null query_mask"),
])
def test_checks_before_any_device(bsr_mod, fake_index, kw, msg):
    L = bsr_mod.lib()
    outs = [np.full((1, 1025), 7, np.uint64), np.full((1, 1025), 7, np.float32), np.full(1, 7, np.uint32)]
    passed = list(outs)
    if "outs" in kw:
        passed[kw.pop("outs")] = None
    kw.setdefault("ix", fake_index[0])
    assert _call(L, outs=passed, **kw) == -1 and msg in L.bsr_last_error()
    assert all((a == 7).all() for a in outs)
    # past every check above: the index is looked at (not loaded), still before any device
    if kw["ix"] is not None:
        assert _call(L, fake_index[0], 1024, qmask=QM, n_masks=2, outs=outs) == -7


def test_wrapper_mask_arguments(bsr_mod):
    ix = bsr_mod.Index.__new__(bsr_mod.Index)
    ix.dim = 8
    for kw in (dict(allow_mask=np.ones(4, bool), allow_masks=np.ones((1, 4), bool), query_mask=QM),
               dict(allow_masks=np.ones((1, 4), bool)), dict(query_mask=QM)):
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.deep_search(Q, 5, **kw)
        assert e.value.status == -1
    with pytest.raises(bsr_mod.BsrError):
        ix.deep_search_device(Q, 1, 5, None, None, None, query_mask=QM)
