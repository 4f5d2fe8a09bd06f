"""The deep capped search's host side, without a GPU: the argument checks of
bsr_local_top_k_deep_capped that return before any device is touched, in the header's order (the
checks behind "not loaded" -- row_group_len, a null row_group, n_queries = 0 -- need a loaded index:
tests/test_gpu_deep_cap.py), and the Python wrapper's own checks."""
import ctypes

import numpy as np
import pytest

Q = np.zeros((1, 8), np.float32)
RG = np.zeros(4, np.uint32)


def _p(a):
    return None if a is None else a.ctypes.data


def _call(L, ix, k, per_group=3, q=Q, nq=1, rg=RG, n_groups=4, outs=None):
    oi, od, og, oc = outs
    return L.bsr_local_top_k_deep_capped(ix, _p(q), nq, k, per_group, _p(rg), 4, n_groups, _p(oi), _p(od), _p(og),
                                         _p(oc))


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
    (dict(k=5, per_group=0), b"per_group=0 outside"),
    (dict(k=5, per_group=17), b"per_group=17 outside"),
    (dict(k=5, n_groups=0), b"n_groups = 0"),
    (dict(k=1024, per_group=16, n_groups=2 ** 28), b"exceeds 2^32 - 1"),
    (dict(k=5, q=None), b"null queries"),
    (dict(k=5, outs=0), b"null output"),
    (dict(k=5, outs=1), b"null output"),
    (dict(k=5, outs=3), b"null output"),
])
def test_checks_before_any_device(bsr_mod, fake_index, kw, msg):
    L = bsr_mod.lib()
    outs = [np.full((1, 1025), 7, np.uint64), np.full((1, 1025), 7, np.float32), np.full((1, 1025), 7, np.uint32),
            np.full(1, 7, np.uint32)]
    passed = list(outs)
    if "outs" in kw:
        passed[kw.pop("outs")] = None
    kw.setdefault("ix", fake_index[0])
    assert _call(L, outs=passed, **kw) == -1 and msg in L.bsr_last_error()
    assert all((a == 7).all() for a in outs)
    # past every check above (out_group is nullable; k = 3, per_group = 16: min(3, 16) * 2^30 fits): the
    # index is looked at (not loaded), still before any device
    if kw["ix"] is not None:
        passed = [outs[0], outs[1], None, outs[3]]
        assert _call(L, fake_index[0], 3, per_group=16, n_groups=2 ** 30, outs=passed) == -7
        assert _call(L, fake_index[0], 1024, nq=0, q=None, outs=[None] * 4) == -7
        assert all((a == 7).all() for a in outs)


def test_wrapper_checks(bsr_mod):
    ix = bsr_mod.Index.__new__(bsr_mod.Index)
    ix.dim = 8
    for kw in (dict(k=0), dict(k=1025), dict(k=5, per_group=0), dict(k=5, per_group=17), dict(k=5, n_groups=0),
               dict(k=5, row_group=np.array([0.5]))):
        kw.setdefault("row_group", RG)
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.deep_capped_search(Q, **kw)
        assert e.value.status == -1
