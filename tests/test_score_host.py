"""The id scoring's host side, without a GPU: the argument checks of bsr_local_score_ids and
bsr_local_rerank_ids that need no device, the Python wrappers' handling of id lists, and the
constants."""
import ctypes
import os
import re

import numpy as np
import pytest

PAD = 2 ** 64 - 1


def _p(a):
    return None if a is None else a.ctypes.data


def _score(L, ix, q, nq, ids, m, od, of):
    return L.bsr_local_score_ids(ix, _p(q), nq, _p(ids), m, _p(od), _p(of))


def _rerank(L, ix, q, nq, ids, m, k, oi, od, oc):
    return L.bsr_local_rerank_ids(ix, _p(q), nq, _p(ids), m, k, _p(oi), _p(od), _p(oc))


def _outs(nq=1, m=4):
    return (np.full((nq, m), 7, np.uint64), np.full((nq, m), 7, np.float32), np.full(nq, 7, np.uint32))


def _untouched(*arrays):
    return all((a == 7).all() for a in arrays)


Q = np.zeros((1, 8), np.float32)
IDS = np.zeros((1, 4), np.uint64)


@pytest.fixture()
def fake_index():
    """A non-null index pointer for the checks that return before the index is looked at (zeroed
    memory: `loaded` reads false, so a check that let the call through would end in BSR_E_STATE)."""
    buf = ctypes.create_string_buffer(1 << 16)
    return ctypes.c_void_p(ctypes.addressof(buf)), buf


def test_null_index_is_invalid(bsr_mod):
    L = bsr_mod.lib()
    oi, od, oc = _outs()
    assert _score(L, None, Q, 1, IDS, 4, od, oc) == -1 and b"null index" in L.bsr_last_error()
    assert _rerank(L, None, Q, 1, IDS, 4, 4, oi, od, oc) == -1 and b"null index" in L.bsr_last_error()
    assert _untouched(oi, od, oc)


def test_list_length_checks(bsr_mod, fake_index):
    L = bsr_mod.lib()
    ix = fake_index[0]
    oi, od, oc = _outs()
    for nq in (0, 1):
        assert _score(L, ix, Q, nq, IDS, 0, od, oc) == -1 and b"m = 0" in L.bsr_last_error()
        assert _rerank(L, ix, Q, nq, IDS, 0, 1, oi, od, oc) == -1 and b"m = 0" in L.bsr_last_error()
    # n_queries * m = 2^32 (nothing is read before the check refuses it)
    for nq, m in ((2 ** 16, 2 ** 16), (2 ** 31, 2), (2 ** 20, 4096)):
        assert _score(L, ix, Q, nq, IDS, m, od, oc) == -1 and b"32 bits" in L.bsr_last_error(), (nq, m)
    assert _rerank(L, ix, Q, 2 ** 20, IDS, 4096, 1, oi, od, oc) == -1 and b"32 bits" in L.bsr_last_error()
    assert _untouched(oi, od, oc)


def test_rerank_k_and_m_limits(bsr_mod, fake_index):
    L = bsr_mod.lib()
    ix = fake_index[0]
    oi, od, oc = _outs()
    for nq in (0, 1):
        assert _rerank(L, ix, Q, nq, IDS, 4, 0, oi, od, oc) == -1 and b"k=0" in L.bsr_last_error()
        assert _rerank(L, ix, Q, nq, IDS, 4, 5, oi, od, oc) == -1 and b"k=5" in L.bsr_last_error()
        assert _rerank(L, ix, Q, nq, IDS, 4097, 1, oi, od, oc) == -1 and b"BSR_SCORE_MAX_IDS" in L.bsr_last_error()
    # the scores have no such limit: m = 4097 reaches the index, which is not loaded
    assert _score(L, ix, Q, 1, IDS, 4097, od, oc) == -7
    assert _untouched(oi, od, oc)


def test_null_pointers_are_invalid(bsr_mod, fake_index):
    L = bsr_mod.lib()
    ix = fake_index[0]
    oi, od, oc = _outs()
    assert _score(L, ix, None, 1, IDS, 4, od, oc) == -1 and b"null queries" in L.bsr_last_error()
    assert _score(L, ix, Q, 1, None, 4, od, oc) == -1 and b"null ids" in L.bsr_last_error()
    assert _score(L, ix, Q, 1, IDS, 4, None, oc) == -1 and b"null output" in L.bsr_last_error()
    assert _rerank(L, ix, None, 1, IDS, 4, 4, oi, od, oc) == -1 and b"null queries" in L.bsr_last_error()
    assert _rerank(L, ix, Q, 1, None, 4, 4, oi, od, oc) == -1 and b"null ids" in L.bsr_last_error()
    for outs in ((None, od, oc), (oi, None, oc), (oi, od, None)):
        assert _rerank(L, ix, Q, 1, IDS, 4, 4, *outs) == -1 and b"null output" in L.bsr_last_error()
    # legal calls reach the index, which is not loaded (out_found may be null; so may everything at
    # n_queries = 0)
    assert _score(L, ix, Q, 1, IDS, 4, od, oc) == -7
    assert _score(L, ix, Q, 1, IDS, 4, od, None) == -7
    assert _score(L, ix, None, 0, None, 4, None, None) == -7
    assert _rerank(L, ix, Q, 1, IDS, 4, 4, oi, od, oc) == -7
    assert _rerank(L, ix, Q, 1, IDS, 4096, 4096, oi, od, oc) == -7
    assert _untouched(oi, od, oc)


class _Stub:
    """Index.score_ids / Index.rerank over a recording stand-in for the library calls."""

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

        def arr(p, ctype, shape):
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), shape)

        def fake_score(h, q, nq, ids, m, od, of):
            self.calls.append(("score", arr(q, ctypes.c_float, (nq, dim)).copy(),
                               arr(ids, ctypes.c_uint64, (nq, m)).copy(), None))
            arr(od, ctypes.c_float, (nq, m))[:] = 0.5
            arr(of, ctypes.c_uint32, (nq,))[:] = np.arange(nq)
            return status

        def fake_rerank(h, q, nq, ids, m, k, oi, od, oc):
            self.calls.append(("rerank", arr(q, ctypes.c_float, (nq, dim)).copy(),
                               arr(ids, ctypes.c_uint64, (nq, m)).copy(), k))
            arr(oc, ctypes.c_uint32, (nq,))[:] = k
            return status

        class L:
            bsr_local_score_ids = staticmethod(fake_score)
            bsr_local_rerank_ids = staticmethod(fake_rerank)
            bsr_last_error = staticmethod(lambda: b"stub")
            bsr_status_string = staticmethod(lambda s: b"BSR_E")
        monkeypatch.setattr(bsr_mod, "lib", lambda: L)


def test_wrapper_pads_ragged_lists_and_maps_negatives(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.arange(24, dtype=np.float64).reshape(3, 8)
    dist = s.ix.score_ids(q, [[5, 6, 7], [9], [1, -1, 2, -5]])
    assert dist.shape == (3, 4) and dist.dtype == np.float32 and (dist == 0.5).all()
    kind, qa, ids, _ = s.calls[-1]
    assert kind == "score" and np.array_equal(qa, q.astype(np.float32))
    assert ids.tolist() == [[5, 6, 7, PAD], [9, PAD, PAD, PAD], [1, PAD, 2, PAD]]
    # a 2-D signed array: negative entries are padding; an unsigned one goes through as it is
    dist, found = s.ix.score_ids(q[:2], np.array([[3, -1], [-7, 4]], np.int64), return_found=True)
    assert s.calls[-1][2].tolist() == [[3, PAD], [PAD, 4]]
    assert dist.shape == (2, 2) and found.dtype == np.uint32 and found.tolist() == [0, 1]
    big = np.array([[2 ** 63 + 1, PAD - 1]], np.uint64)
    s.ix.score_ids(q[0], big)
    assert np.array_equal(s.calls[-1][2], big)
    # Python integers above 2^63 beside small and negative ones (no common numpy integer type)
    s.ix.score_ids(q[:2], [[PAD, 0, 2 ** 64 - 2, 5], [-1, 2 ** 63, 7]])
    assert s.calls[-1][2].tolist() == [[PAD, 0, 2 ** 64 - 2, 5], [PAD, 2 ** 63, 7, PAD]]


def test_wrapper_shapes_a_flat_list_and_defaults_k(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.zeros((2, 8), np.float32)
    dist = s.ix.score_ids(q[0], [4, 5, 6])                       # one query, a 1-D list
    assert dist.shape == (1, 3) and s.calls[-1][2].tolist() == [[4, 5, 6]]
    s.ix.score_ids(q[0], np.array([4, 5, 6]))                    # ... as an array
    assert s.calls[-1][2].tolist() == [[4, 5, 6]]
    idx, dist, cnt = s.ix.rerank(q, [[1, 2, 3], [4]])
    assert s.calls[-1][0] == "rerank" and s.calls[-1][3] == 3, "k defaults to the list length"
    assert idx.shape == (2, 3) and idx.dtype == np.uint64 and dist.shape == (2, 3) and dist.dtype == np.float32
    assert cnt.dtype == np.uint32 and cnt.tolist() == [3, 3]
    assert s.calls[-1][2].tolist() == [[1, 2, 3], [4, PAD, PAD]]
    idx, dist, cnt = s.ix.rerank(q, [[1, 2, 3], [4]], k=2)
    assert idx.shape == (2, 2) and s.calls[-1][3] == 2


def test_wrapper_errors(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.zeros((2, 8), np.float32)
    with pytest.raises(bsr_mod.BsrError) as e:
        s.ix.score_ids(np.zeros((2, 9), np.float32), [[1], [2]])
    assert e.value.status == -6
    for bad in ([[1], [2], [3]], [[1.5], [2.0]], [[], []], np.zeros((2, 2, 2), np.int64), [[2 ** 64], [-1]],
                [[True], [2 ** 64 - 1]]):
        with pytest.raises(bsr_mod.BsrError) as e:
            s.ix.score_ids(q, bad)
        assert e.value.status == -1
    for k in (0, 3):
        with pytest.raises(bsr_mod.BsrError) as e:
            s.ix.rerank(q, [[1, 2], [3]], k=k)
        assert e.value.status == -1
    with pytest.raises(bsr_mod.BsrError) as e:
        s.ix.rerank(q, np.zeros((2, 4097), np.int64))
    assert e.value.status == -1
    assert not s.calls
    s2 = _Stub(bsr_mod, monkeypatch, 8, status=-4)
    with pytest.raises(bsr_mod.BsrError) as e:
        s2.ix.score_ids(q, [[1], [2]])
    assert e.value.status == -4 and len(s2.calls) == 1


def test_constants_mirror_header(bsr_mod):
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "bsr.h")).read()
    for name, want in (("BSR_PATH_SCORE", 131072), ("BSR_SCORE_MAX_IDS", 4096)):
        m = re.search(r"#define\s+%s\s+(\d+)u" % name, src)
        assert m and int(m.group(1)) == want == getattr(bsr_mod, name), name
    assert "bsr_local_score_ids" in src and "bsr_local_rerank_ids" in src
    assert bsr_mod.lib().bsr_local_score_ids.restype is ctypes.c_int
    assert bsr_mod.lib().bsr_local_rerank_ids.restype is ctypes.c_int
