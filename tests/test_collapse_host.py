"""The collapsed search's host side, without a GPU: the argument checks of bsr_local_top_k_collapsed
that need no device (step 1 of the header's list, in its order, and the step-2 state check), the
Python wrapper's shapes, its defaults and argument exclusions, and the two constants."""
import ctypes
import os
import re

import numpy as np
import pytest


def _outs(nq=1, k=4):
    return (np.full((nq, k), 7, np.uint64), np.full((nq, k), 7, np.float32), np.full((nq, k), 7, np.uint32),
            np.full(nq, 7, np.uint32))


def _untouched(outs):
    return all((o == 7).all() for o in outs)


def _call(L, ix, q, nq, k, fetch_k, rg, rg_len, n_groups, allow, words, n_masks, qm, mode, oi, od, og, oc):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return L.bsr_local_top_k_collapsed(ix, p(q), nq, k, fetch_k, p(rg), rg_len, n_groups, p(allow), words, n_masks,
                                       p(qm), mode, p(oi), p(od), p(og), p(oc))


@pytest.fixture()
def fake_index(bsr_mod):
    """A non-null index pointer for the checks that return before the index is used: zeroed memory
    (`loaded` reads false, so a call that passes every check of step 1 ends in BSR_E_STATE) whose
    leading bsr_config carries max_k = 64."""
    buf = ctypes.create_string_buffer(1 << 16)
    bsr_mod._Config.from_buffer(buf).max_k = 64
    return ctypes.c_void_p(ctypes.addressof(buf)), buf


Q = np.zeros((1, 8), np.float32)
RG = np.zeros(16, np.uint32)
ALLOW = np.zeros(4, np.uint64)
QM = np.zeros(1, np.uint32)


def test_null_index_is_invalid(bsr_mod):
    L = bsr_mod.lib()
    outs = _outs()
    assert _call(L, None, Q, 1, 2, 4, RG, 16, 3, None, 0, 0, None, 0, *outs) == -1
    assert b"null index" in L.bsr_last_error()
    assert _untouched(outs)


@pytest.mark.parametrize("k,fetch_k", [(0, 4), (5, 4), (1, 65), (0, 0), (2 ** 32 - 1, 2 ** 32 - 1)])
def test_k_and_fetch_k_out_of_range(bsr_mod, fake_index, k, fetch_k):
    L = bsr_mod.lib()
    outs = _outs()
    for nq in (0, 1):
        assert _call(L, fake_index[0], Q, nq, k, fetch_k, RG, 16, 3, None, 0, 0, None, 0, *outs) == -1
        assert b"fetch_k" in L.bsr_last_error() and b"max_k=64" in L.bsr_last_error()
    assert _untouched(outs)


def test_zero_groups(bsr_mod, fake_index):
    L = bsr_mod.lib()
    outs = _outs()
    for nq in (0, 1):
        assert _call(L, fake_index[0], Q, nq, 2, 4, RG, 16, 0, None, 0, 0, None, 0, *outs) == -1
        assert b"n_groups = 0" in L.bsr_last_error()
    assert _untouched(outs)


def test_inconsistent_mask_arguments(bsr_mod, fake_index):
    L = bsr_mod.lib()
    outs = _outs()
    ix = fake_index[0]
    err = L.bsr_last_error
    # no allow masks: n_masks must be 0 and query_mask null
    assert _call(L, ix, Q, 1, 2, 4, RG, 16, 3, None, 0, 1, None, 0, *outs) == -1 and b"without allow masks" in err()
    assert _call(L, ix, Q, 1, 2, 4, RG, 16, 3, None, 0, 0, QM, 0, *outs) == -1 and b"without allow masks" in err()
    # allow masks: at least one, and a query_mask for more than one
    assert _call(L, ix, Q, 1, 2, 4, RG, 16, 3, ALLOW, 4, 0, None, 0, *outs) == -1 and b"n_masks = 0" in err()
    assert _call(L, ix, Q, 1, 2, 4, RG, 16, 3, ALLOW, 2, 2, None, 0, *outs) == -1 and b"null query_mask" in err()
    assert _untouched(outs)


def test_unknown_mode(bsr_mod, fake_index):
    L = bsr_mod.lib()
    outs = _outs()
    assert _call(L, fake_index[0], Q, 1, 2, 4, RG, 16, 3, ALLOW, 4, 1, None, 3, *outs) == -1
    assert b"unknown mask mode 3" in L.bsr_last_error()
    assert _call(L, fake_index[0], Q, 1, 2, 4, RG, 16, 3, None, 0, 0, None, 7, *outs) == -1
    assert b"unknown mask mode 7" in L.bsr_last_error()
    assert _untouched(outs)


def test_null_pointers_and_state(bsr_mod, fake_index):
    L = bsr_mod.lib()
    oi, od, og, oc = outs = _outs()
    ix = fake_index[0]
    assert _call(L, ix, None, 1, 2, 4, RG, 16, 3, None, 0, 0, None, 0, *outs) == -1
    assert b"null queries" in L.bsr_last_error()
    for o in ((None, od, og, oc), (oi, None, og, oc), (oi, od, og, None)):
        assert _call(L, ix, Q, 1, 2, 4, RG, 16, 3, None, 0, 0, None, 0, *o) == -1
        assert b"null output" in L.bsr_last_error()
    # every check of step 1 passed (out_group is optional; with n_queries = 0 so are the others; the
    # row_group checks of step 3 come after the state check): the index is not loaded
    for args in ((Q, 1, 2, 4, RG, 16, 3, None, 0, 0, None, 0, oi, od, None, oc),
                 (Q, 1, 4, 4, RG, 16, 1, ALLOW, 4, 1, None, 1, oi, od, og, oc),
                 (Q, 1, 1, 64, RG, 16, 2 ** 32 - 1, ALLOW, 2, 2, QM, 2, oi, od, og, oc),
                 (Q, 1, 2, 4, None, 0, 3, None, 0, 0, None, 0, oi, od, og, oc),
                 (Q, 1, 2, 4, RG, 5, 3, None, 0, 0, None, 0, oi, od, og, oc),
                 (None, 0, 2, 4, None, 0, 1, None, 0, 0, None, 0, None, None, None, None)):
        assert _call(L, ix, *args) == -7 and b"not loaded" in L.bsr_last_error()
    assert _untouched(outs)


def test_check_order(bsr_mod, fake_index):
    """The header's order: k / fetch_k, n_groups, the mask set, the mode, the null pointers, the state."""
    L = bsr_mod.lib()
    ix = fake_index[0]
    bad = lambda **kw: _call(L, ix, kw.get("q"), 1, kw.get("k", 2), 4, None, 99, kw.get("ng", 3), None, 0,  # noqa: E731
                             kw.get("nm", 0), None, kw.get("mode", 0), kw.get("oi"), kw.get("oi"), None, kw.get("oi"))
    err = L.bsr_last_error
    assert bad(k=0, ng=0, nm=1, mode=9) == -1 and b"fetch_k" in err()
    assert bad(ng=0, nm=1, mode=9) == -1 and b"n_groups" in err()
    assert bad(nm=1, mode=9) == -1 and b"without allow masks" in err()
    assert bad(mode=9) == -1 and b"unknown mask mode" in err()
    assert bad() == -1 and b"null queries" in err()
    assert bad(q=Q) == -1 and b"null output" in err()
    # (a null row_group of the wrong length: the state check comes first)
    assert bad(q=Q, oi=np.zeros(8, np.uint64)) == -7 and b"not loaded" in err()


class _Stub:
    """Index.collapsed_search over a recording stand-in for the library call."""

    def __init__(self, bsr_mod, monkeypatch, dim, max_k=64, n=100, status=0):
        self.calls = []

        class NoHandle(bsr_mod.Index):  # (its handle is never the library's: nothing to destroy)
            def close(self):
                self._h = None

            __del__ = close

            def get_count(self):
                return n
        ix = object.__new__(NoHandle)
        ix._h = ctypes.c_void_p(0x1000)
        ix.dim = dim
        ix.max_k = max_k
        self.ix = ix

        def fake(h, q, nq, k, fetch_k, rg, rg_len, n_groups, allow, words, n_masks, qm, mode, oi, od, og, oc):
            self.calls.append(dict(nq=nq, k=k, fetch_k=fetch_k, rg=rg, rg_len=rg_len, n_groups=n_groups, allow=allow,
                                   words=words, n_masks=n_masks, qm=qm, mode=mode, group=og))
            np.ctypeslib.as_array(ctypes.cast(oc, ctypes.POINTER(ctypes.c_uint32)), (nq,))[:] = np.arange(nq)
            return status

        class L:
            bsr_local_top_k_collapsed = staticmethod(fake)
            bsr_last_error = staticmethod(lambda: b"stub")
            bsr_status_string = staticmethod(lambda s: b"BSR_E")
        monkeypatch.setattr(bsr_mod, "lib", lambda: L)


RG100 = np.arange(100) // 7  # groups 0 .. 14


def test_wrapper_shapes_and_defaults(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.arange(24, dtype=np.float64).reshape(3, 8)
    idx, dist, cnt = s.ix.collapsed_search(q, 5, RG100)
    assert idx.shape == (3, 5) and idx.dtype == np.uint64
    assert dist.shape == (3, 5) and dist.dtype == np.float32
    assert cnt.shape == (3,) and cnt.dtype == np.uint32 and list(cnt) == [0, 1, 2]
    c = s.calls[-1]
    assert (c["nq"], c["k"], c["fetch_k"]) == (3, 5, 32)                      # max(4 k, 32)
    assert (c["rg_len"], c["n_groups"]) == (100, 15) and c["rg"]              # max(row_group) + 1
    assert c["allow"] is None and c["words"] == 0 and c["n_masks"] == 0 and c["qm"] is None and c["group"] is None
    s.ix.collapsed_search(q, 10, RG100)
    assert s.calls[-1]["fetch_k"] == 40                                       # 4 k
    s.ix.collapsed_search(q, 30, RG100)
    assert s.calls[-1]["fetch_k"] == 64                                       # capped by max_k
    s.ix.collapsed_search(q[0], 3, list(RG100), n_groups=40, fetch_k=7)       # one query as a vector, a list
    c = s.calls[-1]
    assert (c["nq"], c["k"], c["fetch_k"], c["n_groups"], c["rg_len"]) == (1, 3, 7, 40, 100)
    out = s.ix.collapsed_search(q, 4, RG100, return_groups=True)
    assert len(out) == 4 and out[3].shape == (3, 4) and out[3].dtype == np.uint32 and s.calls[-1]["group"] is not None
    # an empty shard: no groups to name, a null row_group
    s.ix.collapsed_search(q, 4, np.zeros(0, np.int64))
    c = s.calls[-1]
    assert c["rg"] is None and c["rg_len"] == 0 and c["n_groups"] == 1


def test_wrapper_masks(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8, n=100)
    q = np.zeros((3, 8), np.float32)
    s.ix.collapsed_search(q, 2, RG100, allow_ids=[1, 5, 70], mask_mode="list")
    c = s.calls[-1]
    assert c["allow"] and c["words"] == 2 and c["n_masks"] == 1 and c["qm"] is None and c["mode"] == bsr_mod.BSR_MASK_LIST
    s.ix.collapsed_search(q, 2, RG100, allow_mask=np.ones(100, bool))
    assert s.calls[-1]["n_masks"] == 1 and s.calls[-1]["mode"] == bsr_mod.BSR_MASK_AUTO
    s.ix.collapsed_search(q, 2, RG100, allow_masks=np.ones((3, 100), bool), query_mask=[0, 2, 1], mask_mode="filter")
    c = s.calls[-1]
    assert c["words"] == 2 and c["n_masks"] == 3 and c["qm"] and c["mode"] == bsr_mod.BSR_MASK_FILTER


def test_wrapper_errors(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.zeros((3, 8), np.float32)
    m = np.ones(100, bool)
    with pytest.raises(bsr_mod.BsrError) as e:
        s.ix.collapsed_search(np.zeros((3, 9), np.float32), 2, RG100)
    assert e.value.status == -6
    for kw in (dict(k=0), dict(k=5, fetch_k=4), dict(k=2, fetch_k=65), dict(k=65),
               dict(k=2, n_groups=0), dict(k=2, n_groups=2 ** 32),
               dict(k=2, row_group=RG100 - 1), dict(k=2, row_group=RG100.astype(np.float64)),
               dict(k=2, allow_mask=m, allow_ids=[1]),
               dict(k=2, allow_mask=m, allow_masks=np.ones((2, 100), bool), query_mask=[0, 1, 0]),
               dict(k=2, allow_ids=[1], query_mask=[0, 0, 0]),
               dict(k=2, allow_masks=np.ones((2, 100), bool)),
               dict(k=2, query_mask=[0, 0, 0]),
               dict(k=2, allow_masks=np.ones((2, 100), bool), query_mask=[0, 1])):
        kw.setdefault("row_group", RG100)
        with pytest.raises(bsr_mod.BsrError) as e:
            s.ix.collapsed_search(q, **kw)
        assert e.value.status == -1, kw
    assert not s.calls
    with pytest.raises(bsr_mod.BsrError):
        s.ix.collapsed_search_device(q, 3, 2, 4, RG100.astype(np.uint32), 15, None, None, None,
                                     query_mask=np.zeros(3, np.uint32))
    assert not s.calls
    s2 = _Stub(bsr_mod, monkeypatch, 8, status=-2)
    with pytest.raises(bsr_mod.BsrError) as e:
        s2.ix.collapsed_search(q, 2, RG100)
    assert e.value.status == -2 and len(s2.calls) == 1


def test_device_wrapper_passes_buffers_through(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.zeros((3, 8), np.float32)
    rg = RG100.astype(np.uint32)
    oi, od, og, oc = _outs(3, 2)
    s.ix.collapsed_search_device(q, 3, 2, 6, rg, 15, oi, od, oc)
    c = s.calls[-1]
    assert (c["nq"], c["k"], c["fetch_k"], c["n_groups"], c["rg_len"]) == (3, 2, 6, 15, 100)
    assert c["rg"] == rg.ctypes.data and c["group"] is None and c["n_masks"] == 0
    s.ix.collapsed_search_device(q, 3, 2, 6, rg, 15, oi, od, oc, out_group=og, allow_words=np.zeros(2, np.uint64))
    c = s.calls[-1]
    assert c["group"] == og.ctypes.data and c["n_masks"] == 1 and c["words"] == 2 and c["qm"] is None
    s.ix.collapsed_search_device(q, 3, 2, 6, rg, 15, oi, od, oc, allow_words=np.zeros((4, 2), np.uint64),
                                 query_mask=np.zeros(3, np.uint32), mask_mode="list")
    c = s.calls[-1]
    assert c["n_masks"] == 4 and c["words"] == 2 and c["qm"] and c["mode"] == bsr_mod.BSR_MASK_LIST
    assert list(oc) == [0, 1, 2]


def test_constants_mirror_header(bsr_mod):
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "bsr.h")).read()
    m = re.search(r"#define\s+BSR_PATH_COLLAPSE\s+(\d+)u", src)
    assert m and int(m.group(1)) == 8192 == bsr_mod.BSR_PATH_COLLAPSE
    m = re.search(r"#define\s+BSR_PATH_COLLAPSE_SCAN\s+(\d+)u", src)
    assert m and int(m.group(1)) == 16384 == bsr_mod.BSR_PATH_COLLAPSE_SCAN
    assert "bsr_local_top_k_collapsed" in src
    assert bsr_mod.lib().bsr_local_top_k_collapsed.restype is ctypes.c_int
