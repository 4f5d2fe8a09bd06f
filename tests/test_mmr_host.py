"""The MMR search's host side, without a GPU: the argument checks of bsr_local_top_k_mmr that need
no device (step 1 of the header's list, in its order, and the step-2 state check), the Python
wrapper's shapes, its fetch_k default and argument exclusions, and the constant."""
import ctypes
import os
import re

import numpy as np
import pytest

NAN = float("nan")


def _outs(nq=1, k=4):
    return (np.full((nq, k), 7, np.uint64), np.full((nq, k), 7, np.float32), np.full((nq, k), 7, np.uint32),
            np.full(nq, 7, np.uint32))


def _untouched(outs):
    return all((o == 7).all() for o in outs)


def _call(L, ix, q, nq, k, fetch_k, lam, allow, words, n_masks, qm, mode, oi, od, orank, oc):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return L.bsr_local_top_k_mmr(ix, p(q), nq, k, fetch_k, lam, p(allow), words, n_masks, p(qm), mode, p(oi), p(od),
                                 p(orank), p(oc))


@pytest.fixture()
def fake_index(bsr_mod):
    """A non-null index pointer for the checks that return before the index is used: zeroed memory
    (`loaded` reads false, so a call that passes every check of step 1 ends in BSR_E_STATE) whose
    leading bsr_config carries max_k = 64."""
    buf = ctypes.create_string_buffer(1 << 16)
    bsr_mod._Config.from_buffer(buf).max_k = 64
    return ctypes.c_void_p(ctypes.addressof(buf)), buf


Q = np.zeros((1, 8), np.float32)
ALLOW = np.zeros(4, np.uint64)
QM = np.zeros(1, np.uint32)


def test_null_index_is_invalid(bsr_mod):
    L = bsr_mod.lib()
    outs = _outs()
    assert _call(L, None, Q, 1, 2, 4, 0.5, None, 0, 0, None, 0, *outs) == -1 and b"null index" in L.bsr_last_error()
    assert _untouched(outs)


@pytest.mark.parametrize("k,fetch_k", [(0, 4), (5, 4), (1, 65), (0, 0), (2 ** 32 - 1, 2 ** 32 - 1)])
def test_k_and_fetch_k_out_of_range(bsr_mod, fake_index, k, fetch_k):
    L = bsr_mod.lib()
    outs = _outs()
    for nq in (0, 1):
        assert _call(L, fake_index[0], Q, nq, k, fetch_k, 0.5, None, 0, 0, None, 0, *outs) == -1
        assert b"fetch_k" in L.bsr_last_error() and b"max_k=64" in L.bsr_last_error()
    assert _untouched(outs)


@pytest.mark.parametrize("lam", [NAN, -0.001, 1.001, float("inf"), float("-inf")])
def test_lambda_out_of_range(bsr_mod, fake_index, lam):
    L = bsr_mod.lib()
    outs = _outs()
    assert _call(L, fake_index[0], Q, 1, 2, 4, lam, None, 0, 0, None, 0, *outs) == -1
    assert b"lambda" in L.bsr_last_error()
    assert _untouched(outs)


def test_inconsistent_mask_arguments(bsr_mod, fake_index):
    L = bsr_mod.lib()
    outs = _outs()
    ix = fake_index[0]
    # no allow masks: n_masks must be 0 and query_mask null
    assert _call(L, ix, Q, 1, 2, 4, 0.5, None, 0, 1, None, 0, *outs) == -1 and b"without allow masks" in L.bsr_last_error()
    assert _call(L, ix, Q, 1, 2, 4, 0.5, None, 0, 0, QM, 0, *outs) == -1 and b"without allow masks" in L.bsr_last_error()
    # allow masks: at least one, and a query_mask for more than one
    assert _call(L, ix, Q, 1, 2, 4, 0.5, ALLOW, 4, 0, None, 0, *outs) == -1 and b"n_masks = 0" in L.bsr_last_error()
    assert _call(L, ix, Q, 1, 2, 4, 0.5, ALLOW, 2, 2, None, 0, *outs) == -1 and b"null query_mask" in L.bsr_last_error()
    assert _untouched(outs)


def test_unknown_mode(bsr_mod, fake_index):
    L = bsr_mod.lib()
    outs = _outs()
    assert _call(L, fake_index[0], Q, 1, 2, 4, 0.5, ALLOW, 4, 1, None, 3, *outs) == -1
    assert b"unknown mask mode 3" in L.bsr_last_error()
    assert _call(L, fake_index[0], Q, 1, 2, 4, 0.5, None, 0, 0, None, 7, *outs) == -1
    assert b"unknown mask mode 7" in L.bsr_last_error()
    assert _untouched(outs)


def test_null_pointers_and_state(bsr_mod, fake_index):
    L = bsr_mod.lib()
    oi, od, orank, oc = outs = _outs()
    ix = fake_index[0]
    assert _call(L, ix, None, 1, 2, 4, 0.5, None, 0, 0, None, 0, *outs) == -1 and b"null queries" in L.bsr_last_error()
    for o in ((None, od, orank, oc), (oi, None, orank, oc), (oi, od, orank, None)):
        assert _call(L, ix, Q, 1, 2, 4, 0.5, None, 0, 0, None, 0, *o) == -1 and b"null output" in L.bsr_last_error()
    # every check of step 1 passed (out_rank is optional; with n_queries = 0 so are the others): the
    # index is not loaded
    for args in ((Q, 1, 2, 4, 0.5, None, 0, 0, None, 0, oi, od, None, oc),
                 (Q, 1, 4, 4, 0.0, ALLOW, 4, 1, None, 1, oi, od, orank, oc),
                 (Q, 1, 1, 64, 1.0, ALLOW, 2, 2, QM, 2, oi, od, orank, oc),
                 (None, 0, 2, 4, 0.5, None, 0, 0, None, 0, None, None, None, None)):
        assert _call(L, ix, *args) == -7 and b"not loaded" in L.bsr_last_error()
    assert _untouched(outs)


def test_check_order(bsr_mod, fake_index):
    """The header's order: k / fetch_k, lambda, the mask set, the mode, the null pointers."""
    L = bsr_mod.lib()
    ix = fake_index[0]
    bad = lambda **kw: _call(L, ix, kw.get("q"), 1, kw.get("k", 2), 4, kw.get("lam", 0.5), None, 0, kw.get("nm", 0),  # noqa: E731
                             None, kw.get("mode", 0), None, None, None, None)
    assert bad(k=0, lam=NAN, nm=1, mode=9) == -1 and b"fetch_k" in L.bsr_last_error()
    assert bad(lam=NAN, nm=1, mode=9) == -1 and b"lambda" in L.bsr_last_error()
    assert bad(nm=1, mode=9) == -1 and b"without allow masks" in L.bsr_last_error()
    assert bad(mode=9) == -1 and b"unknown mask mode" in L.bsr_last_error()
    assert bad() == -1 and b"null queries" in L.bsr_last_error()
    assert bad(q=Q) == -1 and b"null output" in L.bsr_last_error()


class _Stub:
    """Index.mmr_search over a recording stand-in for the library call."""

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

        def fake(h, q, nq, k, fetch_k, lam, allow, words, n_masks, qm, mode, oi, od, orank, oc):
            self.calls.append(dict(nq=nq, k=k, fetch_k=fetch_k, lam=lam, allow=allow, words=words, n_masks=n_masks,
                                   qm=qm, mode=mode, rank=orank))
            np.ctypeslib.as_array(ctypes.cast(oc, ctypes.POINTER(ctypes.c_uint32)), (nq,))[:] = np.arange(nq)
            return status

        class L:
            bsr_local_top_k_mmr = staticmethod(fake)
            bsr_last_error = staticmethod(lambda: b"stub")
            bsr_status_string = staticmethod(lambda s: b"BSR_E")
        monkeypatch.setattr(bsr_mod, "lib", lambda: L)


def test_wrapper_shapes_and_defaults(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.arange(24, dtype=np.float64).reshape(3, 8)
    idx, dist, cnt = s.ix.mmr_search(q, 5)
    assert idx.shape == (3, 5) and idx.dtype == np.uint64
    assert dist.shape == (3, 5) and dist.dtype == np.float32
    assert cnt.shape == (3,) and cnt.dtype == np.uint32 and list(cnt) == [0, 1, 2]
    c = s.calls[-1]
    assert (c["nq"], c["k"], c["fetch_k"], c["lam"]) == (3, 5, 20, 0.5)      # max(20, 4 k)
    assert c["allow"] is None and c["words"] == 0 and c["n_masks"] == 0 and c["qm"] is None and c["rank"] is None
    s.ix.mmr_search(q, 10)
    assert s.calls[-1]["fetch_k"] == 40                                       # 4 k
    s.ix.mmr_search(q, 30)
    assert s.calls[-1]["fetch_k"] == 64                                       # capped by max_k
    s.ix.mmr_search(q[0], 3, fetch_k=7, lambda_mult=0.25)                     # one query as a vector
    c = s.calls[-1]
    assert (c["nq"], c["k"], c["fetch_k"], c["lam"]) == (1, 3, 7, 0.25)
    out = s.ix.mmr_search(q, 4, return_rank=True)
    assert len(out) == 4 and out[3].shape == (3, 4) and out[3].dtype == np.uint32 and s.calls[-1]["rank"] is not None


def test_wrapper_masks(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8, n=100)
    q = np.zeros((3, 8), np.float32)
    s.ix.mmr_search(q, 2, allow_ids=[1, 5, 70], mask_mode="list")
    c = s.calls[-1]
    assert c["allow"] and c["words"] == 2 and c["n_masks"] == 1 and c["qm"] is None and c["mode"] == bsr_mod.BSR_MASK_LIST
    s.ix.mmr_search(q, 2, allow_mask=np.ones(100, bool))
    assert s.calls[-1]["n_masks"] == 1 and s.calls[-1]["mode"] == bsr_mod.BSR_MASK_AUTO
    s.ix.mmr_search(q, 2, allow_masks=np.ones((3, 100), bool), query_mask=[0, 2, 1], mask_mode="filter")
    c = s.calls[-1]
    assert c["words"] == 2 and c["n_masks"] == 3 and c["qm"] and c["mode"] == bsr_mod.BSR_MASK_FILTER


def test_wrapper_errors(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.zeros((3, 8), np.float32)
    m = np.ones(100, bool)
    with pytest.raises(bsr_mod.BsrError) as e:
        s.ix.mmr_search(np.zeros((3, 9), np.float32), 2)
    assert e.value.status == -6
    for kw in (dict(k=0), dict(k=5, fetch_k=4), dict(k=2, fetch_k=65), dict(k=65),
               dict(k=2, lambda_mult=NAN), dict(k=2, lambda_mult=-0.1), dict(k=2, lambda_mult=1.5),
               dict(k=2, allow_mask=m, allow_ids=[1]),
               dict(k=2, allow_mask=m, allow_masks=np.ones((2, 100), bool), query_mask=[0, 1, 0]),
               dict(k=2, allow_ids=[1], query_mask=[0, 0, 0]),
               dict(k=2, allow_masks=np.ones((2, 100), bool)),
               dict(k=2, query_mask=[0, 0, 0]),
               dict(k=2, allow_masks=np.ones((2, 100), bool), query_mask=[0, 1])):
        with pytest.raises(bsr_mod.BsrError) as e:
            s.ix.mmr_search(q, **kw)
        assert e.value.status == -1, kw
    assert not s.calls
    with pytest.raises(bsr_mod.BsrError):
        s.ix.mmr_search_device(q, 3, 2, 4, 0.5, None, None, None, query_mask=np.zeros(3, np.uint32))
    assert not s.calls
    s2 = _Stub(bsr_mod, monkeypatch, 8, status=-2)
    with pytest.raises(bsr_mod.BsrError) as e:
        s2.ix.mmr_search(q, 2)
    assert e.value.status == -2 and len(s2.calls) == 1


def test_device_wrapper_passes_buffers_through(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.zeros((3, 8), np.float32)
    oi, od, orank, oc = _outs(3, 2)
    s.ix.mmr_search_device(q, 3, 2, 6, 0.75, oi, od, oc)
    c = s.calls[-1]
    assert (c["nq"], c["k"], c["fetch_k"], c["lam"]) == (3, 2, 6, 0.75) and c["rank"] is None and c["n_masks"] == 0
    s.ix.mmr_search_device(q, 3, 2, 6, 0.75, oi, od, oc, out_rank=orank, allow_words=np.zeros(2, np.uint64))
    c = s.calls[-1]
    assert c["rank"] == orank.ctypes.data and c["n_masks"] == 1 and c["words"] == 2 and c["qm"] is None
    s.ix.mmr_search_device(q, 3, 2, 6, 0.75, oi, od, oc, allow_words=np.zeros((4, 2), np.uint64),
                           query_mask=np.zeros(3, np.uint32), mask_mode="list")
    c = s.calls[-1]
    assert c["n_masks"] == 4 and c["words"] == 2 and c["qm"] and c["mode"] == bsr_mod.BSR_MASK_LIST
    assert list(oc) == [0, 1, 2]


def test_constant_mirrors_header(bsr_mod):
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "bsr.h")).read()
    m = re.search(r"#define\s+BSR_PATH_MMR\s+(\d+)u", src)
    assert m and int(m.group(1)) == 4096 == bsr_mod.BSR_PATH_MMR
    assert "bsr_local_top_k_mmr" in src
    assert bsr_mod.lib().bsr_local_top_k_mmr.restype is ctypes.c_int
