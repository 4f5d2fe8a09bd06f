"""The masked range search's host side, without a GPU: the argument checks of
bsr_local_range_search_masked that return before any device is touched, the Python wrapper's mask
forms and query_mask handling over a stand-in for the library, and the header's declaration."""
import ctypes
import os
import re

import numpy as np
import pytest

MASK_AUTO, MASK_LIST, MASK_FILTER = 0, 1, 2


def _outs(nq=1, cap=4):
    return (np.full((nq, cap), 7, np.uint64), np.full((nq, cap), 7, np.float32), np.full(nq, 7, np.uint32))


def _untouched(oi, od, oc):
    return (oi == 7).all() and (od == 7).all() and (oc == 7).all()


def _call(L, ix, q, nq, r, cap, allow, words, n_masks, qm, mode, oi, od, oc):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return L.bsr_local_range_search_masked(ix, p(q), nq, p(r), cap, p(allow), words, n_masks, p(qm), mode,
                                           p(oi), p(od), p(oc))


@pytest.fixture()
def fake_index():
    """A non-null index pointer for the checks that return before the index is looked at (zeroed
    memory: `loaded` reads false, so a check that let the call through would end in BSR_E_STATE)."""
    buf = ctypes.create_string_buffer(1 << 16)
    return ctypes.c_void_p(ctypes.addressof(buf)), buf


def _args(nq=1):
    return dict(q=np.zeros((1, 8), np.float32), nq=nq, r=np.zeros(1, np.float32), cap=4,
                allow=np.zeros(1, np.uint64), words=1, n_masks=1, qm=np.zeros(1, np.uint32), mode=MASK_AUTO)


def test_null_index_is_invalid(bsr_mod):
    L = bsr_mod.lib()
    oi, od, oc = _outs()
    assert _call(L, None, **_args(), oi=oi, od=od, oc=oc) == -1 and b"null index" in L.bsr_last_error()
    assert _untouched(oi, od, oc)


@pytest.mark.parametrize("cap", [0, 4097, 2 ** 32 - 1])
def test_capacity_out_of_range_is_invalid(bsr_mod, fake_index, cap):
    L = bsr_mod.lib()
    oi, od, oc = _outs()
    for nq in (0, 1):
        a = dict(_args(nq), cap=cap)
        assert _call(L, fake_index[0], **a, oi=oi, od=od, oc=oc) == -1 and b"capacity" in L.bsr_last_error(), (cap, nq)
    assert _untouched(oi, od, oc)


def test_masks_and_mode_are_checked_before_the_index(bsr_mod, fake_index):
    L = bsr_mod.lib()
    oi, od, oc = _outs()
    for nq in (0, 1):
        assert _call(L, fake_index[0], **dict(_args(nq), n_masks=0), oi=oi, od=od, oc=oc) == -1
        assert b"n_masks" in L.bsr_last_error()
        for mode in (3, 2 ** 32 - 1):
            assert _call(L, fake_index[0], **dict(_args(nq), mode=mode), oi=oi, od=od, oc=oc) == -1
            assert b"mode" in L.bsr_last_error()
        # a null query_mask: legal with one mask only
        assert _call(L, fake_index[0], **dict(_args(nq), qm=None, n_masks=2), oi=oi, od=od, oc=oc) == -1
        assert b"query_mask" in L.bsr_last_error()
    assert _untouched(oi, od, oc)


def test_null_pointers_are_invalid(bsr_mod, fake_index):
    L = bsr_mod.lib()
    oi, od, oc = _outs()
    ix = fake_index[0]
    for name, text in (("r", b"null radius"), ("q", b"null queries"), ("allow", b"null allow")):
        assert _call(L, ix, **dict(_args(), **{name: None}), oi=oi, od=od, oc=oc) == -1, name
        assert text in L.bsr_last_error(), name
    for outs in ((None, od, oc), (oi, None, oc), (oi, od, None)):
        assert _call(L, ix, **_args(), oi=outs[0], od=outs[1], oc=outs[2]) == -1
        assert b"null output" in L.bsr_last_error()
    # nothing null, every mode, with and without a query_mask: the call reaches the index, which is
    # not loaded (BSR_E_STATE comes before the allow_words check: the index's row count is not read)
    for mode in (MASK_AUTO, MASK_LIST, MASK_FILTER):
        assert _call(L, ix, **dict(_args(), mode=mode, cap=4096), oi=oi, od=od, oc=oc) == -7
        assert _call(L, ix, **dict(_args(), mode=mode, qm=None, words=99), oi=oi, od=od, oc=oc) == -7
    # no queries: the pointers may be null, the call still reaches the index
    a = dict(_args(0), q=None, r=None, allow=None, qm=None)
    assert _call(L, ix, **a, oi=None, od=None, oc=None) == -7
    assert _untouched(oi, od, oc)


# ---- the wrapper over a recording stand-in for the library ---------------------------------------
class _Stub:
    def __init__(self, bsr_mod, monkeypatch, dim, n, status=0):
        self.plain, self.masked = [], []

        class NoHandle(bsr_mod.Index):  # (its handle is never the library's: nothing to destroy)
            def close(self):
                self._h = None

            def get_count(self):
                return n

            __del__ = close
        ix = object.__new__(NoHandle)
        ix._h = ctypes.c_void_p(0x1000)
        ix.dim = dim
        self.ix = ix

        def arr(p, ct, shape):
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ct)), shape).copy()

        def fake_plain(*args):
            assert len(args) == 8, "bsr_local_range_search keeps its eight arguments"
            h, q, nq, r, cap, oi, od, oc = args
            self.plain.append((arr(q, ctypes.c_float, (nq, dim)), arr(r, ctypes.c_float, (nq,)), cap))
            return status

        def fake_masked(h, q, nq, r, cap, allow, words, n_masks, qm, mode, oi, od, oc):
            self.masked.append(dict(
                q=arr(q, ctypes.c_float, (nq, dim)), r=arr(r, ctypes.c_float, (nq,)), cap=cap,
                allow=arr(allow, ctypes.c_uint64, (n_masks, words)), n_masks=n_masks,
                qm=None if qm is None else arr(qm, ctypes.c_uint32, (nq,)), mode=mode))
            np.ctypeslib.as_array(ctypes.cast(oc, ctypes.POINTER(ctypes.c_uint32)), (nq,))[:] = np.arange(nq)
            return status

        class L:
            bsr_local_range_search = staticmethod(fake_plain)
            bsr_local_range_search_masked = staticmethod(fake_masked)
            bsr_last_error = staticmethod(lambda: b"stub")
            bsr_status_string = staticmethod(lambda s: b"BSR_E")
        monkeypatch.setattr(bsr_mod, "lib", lambda: L)


def test_unmasked_call_is_unchanged(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8, 100)
    q = np.arange(24, dtype=np.float64).reshape(3, 8)
    idx, dist, cnt = s.ix.range_search(q, 0.25)
    assert idx.shape == (3, 256) and not s.masked and len(s.plain) == 1
    qa, ra, cap = s.plain[0]
    assert cap == 256 and np.array_equal(qa, q.astype(np.float32)) and list(ra) == [0.25] * 3
    s.ix.range_search(q, 0.25, mask_mode="list")  # (a mode without a mask: still the plain call)
    assert len(s.plain) == 2 and not s.masked


def test_wrapper_mask_forms(bsr_mod, monkeypatch):
    n = 100
    s = _Stub(bsr_mod, monkeypatch, 8, n)
    q = np.zeros((3, 8), np.float32)
    mask = np.zeros(n, bool)
    mask[[0, 63, 64, 99]] = True
    want = bsr_mod.pack_allow_mask(n, mask=mask)
    assert want.shape == (2,) and want[0] == (1 | 1 << 63) and want[1] == (1 | 1 << 35)
    # one mask: a bool array, row ids, packed words -- the same words, one mask, no query_mask
    for kw in (dict(allow_mask=mask), dict(allow_ids=[0, 63, 64, 99]), dict(allow_mask=want)):
        idx, dist, cnt = s.ix.range_search(q, [0.1, 0.2, 0.3], max_results=5, mask_mode="filter", **kw)
        c = s.masked[-1]
        assert idx.shape == (3, 5) and list(cnt) == [0, 1, 2]
        assert c["n_masks"] == 1 and c["qm"] is None and c["mode"] == MASK_FILTER and c["cap"] == 5
        assert np.array_equal(c["allow"], want[None, :]) and np.array_equal(c["r"], np.float32([0.1, 0.2, 0.3]))
    # groups: bool [G][n] or packed [G][words], query_mask of any integer type
    masks = np.zeros((3, n), bool)
    masks[0, :10] = masks[1, 50:] = True
    packed = bsr_mod.pack_allow_masks(n, masks=masks)
    for am in (masks, packed):
        for qm in ([2, 0, 1], np.array([2, 0, 1], np.int64), np.array([2, 0, 1], np.uint8)):
            s.ix.range_search(q, 0.5, allow_masks=am, query_mask=qm, mask_mode="list")
            c = s.masked[-1]
            assert c["n_masks"] == 3 and list(c["qm"]) == [2, 0, 1] and c["qm"].dtype == np.uint32
            assert c["mode"] == MASK_LIST and np.array_equal(c["allow"], packed) and c["cap"] == 256
    s.ix.range_search(q, 0.5, allow_mask=mask)
    assert s.masked[-1]["mode"] == MASK_AUTO
    assert not s.plain


def test_wrapper_mask_errors(bsr_mod, monkeypatch):
    n = 100
    s = _Stub(bsr_mod, monkeypatch, 8, n)
    q = np.zeros((3, 8), np.float32)
    mask, masks = np.ones(n, bool), np.ones((2, n), bool)
    bad = [
        dict(allow_mask=mask, allow_ids=[1]),                        # two forms of one mask
        dict(allow_mask=mask, allow_masks=masks, query_mask=[0, 1, 0]),  # one mask and groups
        dict(allow_ids=[1], query_mask=[0, 0, 0]),
        dict(allow_masks=masks),                                     # groups without query_mask
        dict(query_mask=[0, 0, 0]),                                  # ... and the reverse
        dict(allow_masks=masks, query_mask=[0, 1]),                  # length
        dict(allow_masks=masks, query_mask=[0.0, 1.0, 0.0]),         # dtype
        dict(allow_masks=masks, query_mask=[0, -1, 0]),              # a negative id
        dict(allow_masks=np.ones(2, np.uint64), query_mask=[0, 0, 0]),   # packed words want [G][words]
        dict(allow_mask=mask, mask_mode="fastest"),
    ]
    for kw in bad:
        with pytest.raises(bsr_mod.BsrError) as e:
            s.ix.range_search(q, 0.1, **kw)
        assert e.value.status == -1, kw
    with pytest.raises(bsr_mod.BsrError) as e:
        s.ix.range_search(q, 0.1, max_results=4097, allow_mask=mask)
    assert e.value.status == -1
    assert not s.masked and not s.plain
    s2 = _Stub(bsr_mod, monkeypatch, 8, n, status=-1)
    with pytest.raises(bsr_mod.BsrError) as e:
        s2.ix.range_search(q, 0.1, allow_mask=mask)
    assert e.value.status == -1 and len(s2.masked) == 1


def test_device_wrapper_forms(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8, 100)
    q, r = np.zeros((2, 8), np.float32), np.float32([0.1, 0.2])
    oi, od, oc = _outs(2, 4)
    s.ix.range_search_device(q, 2, r, 4, oi, od, oc)
    assert len(s.plain) == 1 and not s.masked
    one = np.arange(2, dtype=np.uint64)
    s.ix.range_search_device(q, 2, r, 4, oi, od, oc, allow_words=one, mask_mode="list")
    c = s.masked[-1]
    assert c["n_masks"] == 1 and c["qm"] is None and np.array_equal(c["allow"], one[None, :]) and c["mode"] == MASK_LIST
    grp = np.arange(6, dtype=np.uint64).reshape(3, 2)
    s.ix.range_search_device(q, 2, r, 4, oi, od, oc, allow_words=grp, query_mask=np.array([2, 1], np.uint32))
    c = s.masked[-1]
    assert c["n_masks"] == 3 and list(c["qm"]) == [2, 1] and np.array_equal(c["allow"], grp)
    with pytest.raises(bsr_mod.BsrError):
        s.ix.range_search_device(q, 2, r, 4, oi, od, oc, query_mask=np.zeros(2, np.uint32))
    with pytest.raises(bsr_mod.BsrError):
        s.ix.range_search_device(q, 2, r, 4, oi, od, oc, allow_words=np.zeros((1, 1, 2), np.uint64))


def test_header_declares_the_entry_point(bsr_mod):
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "bsr.h")).read()
    m = re.search(r"int\s+bsr_local_range_search_masked\s*\(([^;]*)\);", src)
    assert m, "bsr_local_range_search_masked is declared in bsr.h"
    params = [p.strip().split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert params == ["ix", "queries", "n_queries", "radius", "capacity", "allow", "allow_words", "n_masks",
                      "query_mask", "mode", "out_idx", "out_dist", "out_count"]
    f = bsr_mod.lib().bsr_local_range_search_masked
    assert f.restype is ctypes.c_int and len(f.argtypes) == 13
    # (the combination is no longer listed as out of scope)
    assert not re.search(r"Out of scope:\s*an allow mask combined with a radius", src)
