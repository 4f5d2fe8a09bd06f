"""The range search's host side, without a GPU: the argument checks of bsr_local_range_search that
need no device, the Python wrapper's shape, dtype and broadcast handling, and the constants."""
import ctypes
import os
import re

import numpy as np
import pytest


def _outs(nq=1, cap=4):
    return (np.full((nq, cap), 7, np.uint64), np.full((nq, cap), 7, np.float32), np.full(nq, 7, np.uint32))


def _call(L, ix, q, nq, r, cap, oi, od, oc):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return L.bsr_local_range_search(ix, p(q), nq, p(r), cap, p(oi), p(od), p(oc))


def test_null_index_is_invalid(bsr_mod):
    L = bsr_mod.lib()
    oi, od, oc = _outs()
    st = _call(L, None, np.zeros((1, 8), np.float32), 1, np.zeros(1, np.float32), 4, oi, od, oc)
    assert st == -1 and b"null index" in L.bsr_last_error()
    assert (oi == 7).all() and (od == 7).all() and (oc == 7).all()


@pytest.fixture()
def fake_index():
    """A non-null index pointer for the checks that return before the index is looked at (zeroed
    memory: `loaded` reads false, so a check that let the call through would end in BSR_E_STATE)."""
    buf = ctypes.create_string_buffer(1 << 16)
    return ctypes.c_void_p(ctypes.addressof(buf)), buf


@pytest.mark.parametrize("cap", [0, 4097, 2 ** 32 - 1])
def test_capacity_out_of_range_is_invalid(bsr_mod, fake_index, cap):
    L = bsr_mod.lib()
    oi, od, oc = _outs()
    for nq in (0, 1):
        st = _call(L, fake_index[0], np.zeros((1, 8), np.float32), nq, np.zeros(1, np.float32), cap, oi, od, oc)
        assert st == -1 and b"capacity" in L.bsr_last_error(), (cap, nq)
    assert (oi == 7).all() and (oc == 7).all()


def test_null_pointers_are_invalid(bsr_mod, fake_index):
    L = bsr_mod.lib()
    q, r = np.zeros((1, 8), np.float32), np.zeros(1, np.float32)
    oi, od, oc = _outs()
    assert _call(L, fake_index[0], q, 1, None, 4, oi, od, oc) == -1 and b"null radius" in L.bsr_last_error()
    assert _call(L, fake_index[0], None, 1, r, 4, oi, od, oc) == -1 and b"null queries" in L.bsr_last_error()
    for outs in ((None, od, oc), (oi, None, oc), (oi, od, None)):
        assert _call(L, fake_index[0], q, 1, r, 4, *outs) == -1 and b"null output" in L.bsr_last_error()
    # in range and nothing null: the call reaches the index, which is not loaded
    assert _call(L, fake_index[0], q, 1, r, 4096, oi, od, oc) == -7
    assert (oi == 7).all() and (od == 7).all() and (oc == 7).all()


class _Stub:
    """Index.range_search over a recording stand-in for the library call."""

    def __init__(self, bsr_mod, monkeypatch, dim, status=0):
        self.calls = []
        class NoHandle(bsr_mod.Index):  # (its handle is never the library's: nothing to destroy)
            def close(self):
                self._h = None

            __del__ = close
        ix = object.__new__(NoHandle)
        ix._h = ctypes.c_void_p(0x1000)
        ix.dim = dim
        self.ix = ix

        def fake(h, q, nq, r, cap, oi, od, oc):
            qa = np.ctypeslib.as_array(ctypes.cast(q, ctypes.POINTER(ctypes.c_float)), (nq, dim)).copy()
            ra = np.ctypeslib.as_array(ctypes.cast(r, ctypes.POINTER(ctypes.c_float)), (nq,)).copy()
            self.calls.append((qa, ra, cap))
            np.ctypeslib.as_array(ctypes.cast(oc, ctypes.POINTER(ctypes.c_uint32)), (nq,))[:] = np.arange(nq)
            return status

        class L:
            bsr_local_range_search = staticmethod(fake)
            bsr_last_error = staticmethod(lambda: b"stub")
            bsr_status_string = staticmethod(lambda s: b"BSR_E")
        monkeypatch.setattr(bsr_mod, "lib", lambda: L)


def test_wrapper_shapes_dtypes_and_broadcast(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.arange(24, dtype=np.float64).reshape(3, 8)
    idx, dist, cnt = s.ix.range_search(q, 0.25)
    assert idx.shape == (3, 256) and idx.dtype == np.uint64
    assert dist.shape == (3, 256) and dist.dtype == np.float32
    assert cnt.shape == (3,) and cnt.dtype == np.uint32 and list(cnt) == [0, 1, 2]
    qa, ra, cap = s.calls[-1]
    assert cap == 256 and np.array_equal(qa, q.astype(np.float32))
    assert ra.dtype == np.float32 and list(ra) == [0.25] * 3           # the scalar, broadcast
    idx, dist, cnt = s.ix.range_search(q[0], [0.5], max_results=7)     # one query as a vector
    assert idx.shape == (1, 7) and s.calls[-1][2] == 7 and list(s.calls[-1][1]) == [0.5]
    s.ix.range_search(q, np.array([0.1, 0.2, 0.3], np.float64), max_results=4096)
    assert np.array_equal(s.calls[-1][1], np.array([0.1, 0.2, 0.3], np.float32))


def test_wrapper_errors(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.zeros((3, 8), np.float32)
    with pytest.raises(bsr_mod.BsrError) as e:
        s.ix.range_search(np.zeros((3, 9), np.float32), 0.1)
    assert e.value.status == -6
    for bad in ([0.1, 0.2], np.zeros((2, 2))):
        with pytest.raises(bsr_mod.BsrError) as e:
            s.ix.range_search(q, bad)
        assert e.value.status == -1
    for cap in (0, 4097):
        with pytest.raises(bsr_mod.BsrError) as e:
            s.ix.range_search(q, 0.1, max_results=cap)
        assert e.value.status == -1
    assert not s.calls
    s2 = _Stub(bsr_mod, monkeypatch, 8, status=-1)
    with pytest.raises(bsr_mod.BsrError) as e:
        s2.ix.range_search(q, 0.1)
    assert e.value.status == -1 and len(s2.calls) == 1


def test_constants_mirror_header(bsr_mod):
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "bsr.h")).read()
    for name, want in (("BSR_PATH_RANGE", 1024), ("BSR_PATH_RANGE_SCAN", 2048), ("BSR_RANGE_MAX_RESULTS", 4096)):
        m = re.search(r"#define\s+%s\s+(\d+)u" % name, src)
        assert m and int(m.group(1)) == want == getattr(bsr_mod, name), name
    assert "bsr_local_range_search" in src
    assert bsr_mod.lib().bsr_local_range_search.restype is ctypes.c_int
