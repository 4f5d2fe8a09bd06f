"""The masked deep capped search's host side, without a GPU: the argument checks of
bsr_local_top_k_deep_capped_masked that return before any device is touched, in the header's order
(the checks behind "not loaded" need a loaded index: tests/test_gpu_deep_cap_masked.py), and the
Python wrapper's own checks."""
import ctypes

import numpy as np
import pytest

Q = np.zeros((1, 8), np.float32)
RG = np.zeros(4, np.uint32)
ALLOW = np.full(1, 15, np.uint64)
QM = np.zeros(1, np.uint32)


def _p(a):
    return None if a is None else a.ctypes.data


def _call(L, ix, k, per_group=3, q=Q, nq=1, rg=RG, n_groups=4, allow=ALLOW, n_masks=1, qm=QM, mode=0, outs=None):
    oi, od, og, oc = outs
    return L.bsr_local_top_k_deep_capped_masked(ix, _p(q), nq, k, per_group, _p(rg), 4, n_groups, _p(allow), 1, n_masks,
                                                _p(qm), mode, _p(oi), _p(od), _p(og), _p(oc))


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
    (dict(k=5, n_masks=0), b"n_masks = 0"),
    (dict(k=5, mode=3), b"unknown mask mode 3"),
    (dict(k=5, n_masks=2, qm=None), b"null query_mask with n_masks = 2"),
    (dict(k=5, q=None), b"null queries"),
    (dict(k=5, outs=0), b"null output"),
    (dict(k=5, outs=1), b"null output"),
    (dict(k=5, outs=3), b"null output"),
    (dict(k=5, allow=None), b"null allow masks"),
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
    # past every check above (out_group and, with one mask, query_mask are nullable): the index is
    # looked at (not loaded: BSR_E_STATE), still before any device -- with n_queries = 0 too
    if kw["ix"] is not None:
        passed = [outs[0], outs[1], None, outs[3]]
        assert _call(L, fake_index[0], 3, per_group=16, n_groups=2 ** 30, qm=None, mode=2, outs=passed) == -7
        assert _call(L, fake_index[0], 1024, nq=0, q=None, allow=None, outs=[None] * 4) == -7
        assert all((a == 7).all() for a in outs)


def test_wrapper_checks(bsr_mod):
    ix = bsr_mod.Index.__new__(bsr_mod.Index)
    ix.dim = 8
    m = np.ones(4, bool)
    for kw in (dict(k=0, allow_mask=m), dict(k=1025, allow_mask=m), dict(k=5, per_group=0, allow_mask=m),
               dict(k=5, per_group=17, allow_ids=[1]), dict(k=5, allow_mask=m, allow_masks=m[None], query_mask=[0]),
               dict(k=5, allow_masks=m[None]), dict(k=5, query_mask=[0]), dict(k=5, allow_ids=[1], query_mask=[0])):
        with pytest.raises(bsr_mod.BsrError) as e:
            ix.deep_capped_search(Q, row_group=RG, **kw)
        assert e.value.status == -1
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.deep_capped_search_device(Q, 1, 5, 3, RG, 4, None, None, None, query_mask=QM)
    assert e.value.status == -1
