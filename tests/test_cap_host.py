"""The capped search's host side, without a GPU: the argument checks of bsr_local_top_k_capped that
need no device (step 1 of the header's list, in its order, and the step-2 state check), the Python
wrapper's shapes, its defaults and argument exclusions, the three constants, and the host merge
bsr_global_top_k_capped against the model -- on random lists, and as the multi-rank capped search
over a store split by interval_by_rank."""
import ctypes
import os
import re

import numpy as np
import pytest

import kcheck_cap as kp
from kcheck_exact import IDX_NONE

F = np.float32
NONFINITE = -2  # BSR_E_NONFINITE


def _outs(nq=1, k=4):
    return (np.full((nq, k), 7, np.uint64), np.full((nq, k), 7, np.float32), np.full((nq, k), 7, np.uint32),
            np.full(nq, 7, np.uint32))


def _untouched(outs):
    return all((o == 7).all() for o in outs)


def _call(L, ix, q, nq, k, fetch_k, m, rg, rg_len, n_groups, allow, words, n_masks, qm, mode, oi, od, og, oc):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return L.bsr_local_top_k_capped(ix, p(q), nq, k, fetch_k, m, p(rg), rg_len, n_groups, p(allow), words, n_masks,
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
    assert _call(L, None, Q, 1, 2, 4, 2, RG, 16, 3, None, 0, 0, None, 0, *outs) == -1
    assert b"null index" in L.bsr_last_error()
    assert _untouched(outs)


@pytest.mark.parametrize("k,fetch_k", [(0, 4), (5, 4), (1, 65), (0, 0), (2 ** 32 - 1, 2 ** 32 - 1)])
def test_k_and_fetch_k_out_of_range(bsr_mod, fake_index, k, fetch_k):
    L = bsr_mod.lib()
    outs = _outs()
    for nq in (0, 1):
        assert _call(L, fake_index[0], Q, nq, k, fetch_k, 2, RG, 16, 3, None, 0, 0, None, 0, *outs) == -1
        assert b"fetch_k" in L.bsr_last_error() and b"max_k=64" in L.bsr_last_error()
    assert _untouched(outs)


@pytest.mark.parametrize("m", [0, 17, 2 ** 32 - 1])
def test_per_group_out_of_range(bsr_mod, fake_index, m):
    L = bsr_mod.lib()
    outs = _outs()
    for nq in (0, 1):
        assert _call(L, fake_index[0], Q, nq, 2, 4, m, RG, 16, 3, None, 0, 0, None, 0, *outs) == -1
        assert b"per_group=%d outside 1 <= per_group <= 16" % m in L.bsr_last_error()
    assert _untouched(outs)


def test_zero_groups(bsr_mod, fake_index):
    L = bsr_mod.lib()
    outs = _outs()
    for nq in (0, 1):
        assert _call(L, fake_index[0], Q, nq, 2, 4, 2, RG, 16, 0, None, 0, 0, None, 0, *outs) == -1
        assert b"n_groups = 0" in L.bsr_last_error()
    assert _untouched(outs)


def test_table_entries_past_32_bits(bsr_mod, fake_index):
    L = bsr_mod.lib()
    outs = _outs()
    ix = fake_index[0]
    # min(per_group, k) * n_groups: 2 * 2^31 and 16 * 2^28 = 2^32 are refused ...
    for k, m, ng in ((2, 2, 2 ** 31), (4, 2, 2 ** 31), (2, 3, 2 ** 31), (64, 16, 2 ** 28), (3, 16, 2 ** 32 - 1)):
        assert _call(L, ix, Q, 1, k, 64, m, RG, 16, ng, None, 0, 0, None, 0, *outs) == -1, (k, m, ng)
        assert b"exceeds 2^32 - 1" in L.bsr_last_error()
    # ... 2^32 - 1 entries are not (k = 1 caps per_group = 16 to one entry a group; 3 * 0x55555555)
    for k, m, ng in ((1, 16, 2 ** 32 - 1), (2, 1, 2 ** 32 - 1), (3, 3, 0x55555555), (64, 16, 2 ** 28 - 1)):
        assert _call(L, ix, Q, 1, k, 64, m, RG, 16, ng, None, 0, 0, None, 0, *outs) == -7, (k, m, ng)
    assert _untouched(outs)


def test_inconsistent_mask_arguments(bsr_mod, fake_index):
    L = bsr_mod.lib()
    outs = _outs()
    ix = fake_index[0]
    err = L.bsr_last_error
    assert _call(L, ix, Q, 1, 2, 4, 2, RG, 16, 3, None, 0, 1, None, 0, *outs) == -1 and b"without allow masks" in err()
    assert _call(L, ix, Q, 1, 2, 4, 2, RG, 16, 3, None, 0, 0, QM, 0, *outs) == -1 and b"without allow masks" in err()
    assert _call(L, ix, Q, 1, 2, 4, 2, RG, 16, 3, ALLOW, 4, 0, None, 0, *outs) == -1 and b"n_masks = 0" in err()
    assert _call(L, ix, Q, 1, 2, 4, 2, RG, 16, 3, ALLOW, 2, 2, None, 0, *outs) == -1 and b"null query_mask" in err()
    assert _untouched(outs)


def test_unknown_mode(bsr_mod, fake_index):
    L = bsr_mod.lib()
    outs = _outs()
    assert _call(L, fake_index[0], Q, 1, 2, 4, 2, RG, 16, 3, ALLOW, 4, 1, None, 3, *outs) == -1
    assert b"unknown mask mode 3" in L.bsr_last_error()
    assert _call(L, fake_index[0], Q, 1, 2, 4, 2, RG, 16, 3, None, 0, 0, None, 7, *outs) == -1
    assert b"unknown mask mode 7" in L.bsr_last_error()
    assert _untouched(outs)


def test_null_pointers_and_state(bsr_mod, fake_index):
    L = bsr_mod.lib()
    oi, od, og, oc = outs = _outs()
    ix = fake_index[0]
    assert _call(L, ix, None, 1, 2, 4, 2, RG, 16, 3, None, 0, 0, None, 0, *outs) == -1
    assert b"null queries" in L.bsr_last_error()
    for o in ((None, od, og, oc), (oi, None, og, oc), (oi, od, og, None)):
        assert _call(L, ix, Q, 1, 2, 4, 2, RG, 16, 3, None, 0, 0, None, 0, *o) == -1
        assert b"null output" in L.bsr_last_error()
    # every check of step 1 passed (out_group is optional; with n_queries = 0 so are the others; the
    # row_group checks of step 3 come after the state check): the index is not loaded
    for args in ((Q, 1, 2, 4, 1, RG, 16, 3, None, 0, 0, None, 0, oi, od, None, oc),
                 (Q, 1, 4, 4, 16, RG, 16, 1, ALLOW, 4, 1, None, 1, oi, od, og, oc),
                 (Q, 1, 1, 64, 16, RG, 16, 2 ** 32 - 1, ALLOW, 2, 2, QM, 2, oi, od, og, oc),
                 (Q, 1, 2, 4, 2, None, 0, 3, None, 0, 0, None, 0, oi, od, og, oc),
                 (Q, 1, 2, 4, 2, RG, 5, 3, None, 0, 0, None, 0, oi, od, og, oc),
                 (None, 0, 2, 4, 3, None, 0, 1, None, 0, 0, None, 0, None, None, None, None)):
        assert _call(L, ix, *args) == -7 and b"not loaded" in L.bsr_last_error()
    assert _untouched(outs)


def test_check_order(bsr_mod, fake_index):
    """The header's order: k / fetch_k, per_group, n_groups, the table's entries, the mask set, the
    mode, the null pointers, the state."""
    L = bsr_mod.lib()
    ix = fake_index[0]
    bad = lambda **kw: _call(L, ix, kw.get("q"), 1, kw.get("k", 2), 4, kw.get("m", 2), None, 99, kw.get("ng", 3),  # noqa: E731
                             None, 0, kw.get("nm", 0), None, kw.get("mode", 0), kw.get("oi"), kw.get("oi"), None,
                             kw.get("oi"))
    err = L.bsr_last_error
    assert bad(k=0, m=0, ng=0, nm=1, mode=9) == -1 and b"fetch_k" in err()
    assert bad(m=0, ng=0, nm=1, mode=9) == -1 and b"per_group" in err() and b"exceeds" not in err()
    assert bad(m=17, ng=2 ** 31, nm=1, mode=9) == -1 and b"per_group=17" in err()
    assert bad(ng=0, nm=1, mode=9) == -1 and b"n_groups = 0" in err()
    assert bad(ng=2 ** 31, nm=1, mode=9) == -1 and b"exceeds 2^32 - 1" in err()
    assert bad(nm=1, mode=9) == -1 and b"without allow masks" in err()
    assert bad(mode=9) == -1 and b"unknown mask mode" in err()
    assert bad() == -1 and b"null queries" in err()
    assert bad(q=Q) == -1 and b"null output" in err()
    # (a null row_group of the wrong length: the state check comes first)
    assert bad(q=Q, oi=np.zeros(8, np.uint64)) == -7 and b"not loaded" in err()


class _Stub:
    """Index.capped_search over a recording stand-in for the library call."""

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

        def fake(h, q, nq, k, fetch_k, m, rg, rg_len, n_groups, allow, words, n_masks, qm, mode, oi, od, og, oc):
            self.calls.append(dict(nq=nq, k=k, fetch_k=fetch_k, m=m, rg=rg, rg_len=rg_len, n_groups=n_groups,
                                   allow=allow, words=words, n_masks=n_masks, qm=qm, mode=mode, group=og))
            np.ctypeslib.as_array(ctypes.cast(oc, ctypes.POINTER(ctypes.c_uint32)), (nq,))[:] = np.arange(nq)
            return status

        def never(*a):
            raise AssertionError("the capped search calls bsr_local_top_k_capped")

        class L:
            bsr_local_top_k_capped = staticmethod(fake)
            bsr_local_top_k_collapsed = staticmethod(never)
            bsr_last_error = staticmethod(lambda: b"stub")
            bsr_status_string = staticmethod(lambda s: b"BSR_E")
        monkeypatch.setattr(bsr_mod, "lib", lambda: L)


RG100 = np.arange(100) // 7  # groups 0 .. 14


def test_wrapper_shapes_and_defaults(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.arange(24, dtype=np.float64).reshape(3, 8)
    idx, dist, cnt = s.ix.capped_search(q, 5, RG100, 2)
    assert idx.shape == (3, 5) and idx.dtype == np.uint64
    assert dist.shape == (3, 5) and dist.dtype == np.float32
    assert cnt.shape == (3,) and cnt.dtype == np.uint32 and list(cnt) == [0, 1, 2]
    c = s.calls[-1]
    assert (c["nq"], c["k"], c["fetch_k"], c["m"]) == (3, 5, 32, 2)           # max(4 k, 32)
    assert (c["rg_len"], c["n_groups"]) == (100, 15) and c["rg"]              # max(row_group) + 1
    assert c["allow"] is None and c["words"] == 0 and c["n_masks"] == 0 and c["qm"] is None and c["group"] is None
    s.ix.capped_search(q, 10, RG100, per_group=16)
    assert s.calls[-1]["fetch_k"] == 40 and s.calls[-1]["m"] == 16            # 4 k
    s.ix.capped_search(q, 30, RG100, 1)
    assert s.calls[-1]["fetch_k"] == 64 and s.calls[-1]["m"] == 1             # capped by max_k
    s.ix.capped_search(q[0], 3, list(RG100), 3, n_groups=40, fetch_k=7)       # one query as a vector, a list
    c = s.calls[-1]
    assert (c["nq"], c["k"], c["fetch_k"], c["m"], c["n_groups"], c["rg_len"]) == (1, 3, 7, 3, 40, 100)
    out = s.ix.capped_search(q, 4, RG100, 2, return_groups=True)
    assert len(out) == 4 and out[3].shape == (3, 4) and out[3].dtype == np.uint32 and s.calls[-1]["group"] is not None
    # an empty shard: no groups to name, a null row_group
    s.ix.capped_search(q, 4, np.zeros(0, np.int64), 2)
    c = s.calls[-1]
    assert c["rg"] is None and c["rg_len"] == 0 and c["n_groups"] == 1


def test_wrapper_masks(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8, n=100)
    q = np.zeros((3, 8), np.float32)
    s.ix.capped_search(q, 2, RG100, 2, allow_ids=[1, 5, 70], mask_mode="list")
    c = s.calls[-1]
    assert c["allow"] and c["words"] == 2 and c["n_masks"] == 1 and c["qm"] is None and c["mode"] == bsr_mod.BSR_MASK_LIST
    s.ix.capped_search(q, 2, RG100, 2, allow_mask=np.ones(100, bool))
    assert s.calls[-1]["n_masks"] == 1 and s.calls[-1]["mode"] == bsr_mod.BSR_MASK_AUTO
    s.ix.capped_search(q, 2, RG100, 2, allow_masks=np.ones((3, 100), bool), query_mask=[0, 2, 1], mask_mode="filter")
    c = s.calls[-1]
    assert c["words"] == 2 and c["n_masks"] == 3 and c["qm"] and c["mode"] == bsr_mod.BSR_MASK_FILTER


def test_wrapper_errors(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.zeros((3, 8), np.float32)
    m = np.ones(100, bool)
    with pytest.raises(bsr_mod.BsrError) as e:
        s.ix.capped_search(np.zeros((3, 9), np.float32), 2, RG100, 2)
    assert e.value.status == -6
    for kw in (dict(k=0), dict(k=5, fetch_k=4), dict(k=2, fetch_k=65), dict(k=65),
               dict(k=2, per_group=0), dict(k=2, per_group=17), dict(k=2, per_group=-1),
               dict(k=2, n_groups=0), dict(k=2, n_groups=2 ** 32),
               dict(k=2, row_group=RG100 - 1), dict(k=2, row_group=RG100.astype(np.float64)),
               dict(k=2, allow_mask=m, allow_ids=[1]),
               dict(k=2, allow_mask=m, allow_masks=np.ones((2, 100), bool), query_mask=[0, 1, 0]),
               dict(k=2, allow_ids=[1], query_mask=[0, 0, 0]),
               dict(k=2, allow_masks=np.ones((2, 100), bool)),
               dict(k=2, query_mask=[0, 0, 0]),
               dict(k=2, allow_masks=np.ones((2, 100), bool), query_mask=[0, 1])):
        kw.setdefault("row_group", RG100)
        kw.setdefault("per_group", 2)
        with pytest.raises(bsr_mod.BsrError) as e:
            s.ix.capped_search(q, **kw)
        assert e.value.status == -1, kw
    assert not s.calls
    with pytest.raises(bsr_mod.BsrError):
        s.ix.capped_search_device(q, 3, 2, 4, 2, RG100.astype(np.uint32), 15, None, None, None,
                                  query_mask=np.zeros(3, np.uint32))
    assert not s.calls
    s2 = _Stub(bsr_mod, monkeypatch, 8, status=-2)
    with pytest.raises(bsr_mod.BsrError) as e:
        s2.ix.capped_search(q, 2, RG100, 2)
    assert e.value.status == -2 and len(s2.calls) == 1


def test_device_wrapper_passes_buffers_through(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8)
    q = np.zeros((3, 8), np.float32)
    rg = RG100.astype(np.uint32)
    oi, od, og, oc = _outs(3, 2)
    s.ix.capped_search_device(q, 3, 2, 6, 3, rg, 15, oi, od, oc)
    c = s.calls[-1]
    assert (c["nq"], c["k"], c["fetch_k"], c["m"], c["n_groups"], c["rg_len"]) == (3, 2, 6, 3, 15, 100)
    assert c["rg"] == rg.ctypes.data and c["group"] is None and c["n_masks"] == 0
    s.ix.capped_search_device(q, 3, 2, 6, 3, rg, 15, oi, od, oc, out_group=og, allow_words=np.zeros(2, np.uint64))
    c = s.calls[-1]
    assert c["group"] == og.ctypes.data and c["n_masks"] == 1 and c["words"] == 2 and c["qm"] is None
    s.ix.capped_search_device(q, 3, 2, 6, 3, rg, 15, oi, od, oc, allow_words=np.zeros((4, 2), np.uint64),
                              query_mask=np.zeros(3, np.uint32), mask_mode="list")
    c = s.calls[-1]
    assert c["n_masks"] == 4 and c["words"] == 2 and c["qm"] and c["mode"] == bsr_mod.BSR_MASK_LIST
    assert list(oc) == [0, 1, 2]


def test_constants_mirror_header(bsr_mod):
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "bsr.h")).read()
    m = re.search(r"#define\s+BSR_PATH_CAP\s+(\d+)u", src)
    assert m and int(m.group(1)) == 32768 == bsr_mod.BSR_PATH_CAP
    m = re.search(r"#define\s+BSR_PATH_CAP_SCAN\s+(\d+)u", src)
    assert m and int(m.group(1)) == 65536 == bsr_mod.BSR_PATH_CAP_SCAN
    m = re.search(r"#define\s+BSR_CAP_MAX_PER_GROUP\s+(\d+)u", src)
    assert m and int(m.group(1)) == 16 == bsr_mod.BSR_CAP_MAX_PER_GROUP == kp.MAX_PER_GROUP
    assert "bsr_local_top_k_capped" in src and "bsr_global_top_k_capped" in src
    assert bsr_mod.lib().bsr_local_top_k_capped.restype is ctypes.c_int
    assert bsr_mod.lib().bsr_global_top_k_capped.restype is ctypes.c_int


# ----------------------------------------------------------------------------------------
# bsr_global_top_k_capped
# ----------------------------------------------------------------------------------------
def _random_lists(rng, L, Q, k_in, n_ids, n_groups, tie_levels):
    """Lists in (distance, index) order, as a search leaves them: ids drawn from a small range (the
    lists of a query overlap: duplicate indices), distances from a few levels (ties) and a function
    of the id (a duplicate carries its distance); short counts, garbage behind them."""
    group_of = rng.integers(0, n_groups, n_ids).astype(np.uint32)
    idx = np.zeros((L, Q, k_in), np.uint64)
    dist = np.zeros((L, Q, k_in), F)
    grp = np.zeros((L, Q, k_in), np.uint32)
    cnt = np.zeros((L, Q), np.uint32)
    for q in range(Q):
        d_of = (rng.integers(0, tie_levels, n_ids) / F(tie_levels)).astype(F)
        for l in range(L):
            c = int(rng.choice([0, 1, k_in // 2, k_in - 1, k_in, k_in]))
            ids = rng.choice(n_ids, c, replace=False)
            ids = ids[np.lexsort((ids, d_of[ids]))]
            idx[l, q, :c], dist[l, q, :c], grp[l, q, :c], cnt[l, q] = ids, d_of[ids], group_of[ids], c
            idx[l, q, c:], dist[l, q, c:], grp[l, q, c:] = 3, -1.0, 0  # (behind the count: never read)
    return idx, dist, grp, cnt


@pytest.mark.parametrize("L", [1, 3, 8])
def test_global_merge_against_model(bsr_mod, L):
    rng = np.random.default_rng(40 + L)
    Q, k_in = 6, 12
    idx, dist, grp, cnt = _random_lists(rng, L, Q, k_in, 40, 5, 6)
    for k in (1, 5, 12, 30):  # (k_in != k on both sides)
        for m in (1, 2, 3, 40):
            oi, od, og, oc = bsr_mod.merge_top_k_lists_capped(idx, dist, grp, cnt, k, m)
            assert oi.shape == od.shape == og.shape == (Q, k) and oc.shape == (Q,)
            for q in range(Q):
                wi, wd, wg, wc = kp.merge_model(idx[:, q], dist[:, q], grp[:, q], cnt[:, q], k, m)
                what = (L, k, m, q)
                assert oc[q] == wc, what
                assert np.array_equal(oi[q], wi), (what, oi[q], wi)
                assert np.array_equal(od[q].view(np.uint32), wd.view(np.uint32)) and np.array_equal(og[q], wg), what
                assert len(set(oi[q][:wc].tolist())) == wc and np.bincount(og[q][:wc]).max(initial=0) <= m
    # a count above k_in reads k_in entries
    big = np.full_like(cnt, k_in + 5)
    oi, od, og, oc = bsr_mod.merge_top_k_lists_capped(idx, np.abs(dist), grp, big, 4, 2)
    for q in range(Q):
        wi, wd, wg, wc = kp.merge_model(idx[:, q], np.abs(dist[:, q]), grp[:, q], np.full(L, k_in), 4, 2)
        assert oc[q] == wc and np.array_equal(oi[q], wi) and np.array_equal(og[q], wg)


def test_global_merge_unsorted_lists_and_null_group_output(bsr_mod):
    # the merge sorts: a list need not arrive in order
    idx = np.array([[[9, 3, 7]], [[8, 4, 7]]], np.uint64)
    dist = np.array([[[0.5, 0.1, 0.2]], [[0.4, 0.3, 0.2]]], F)
    grp = np.array([[[2, 1, 1]], [[2, 1, 1]]], np.uint32)
    cnt = np.full((2, 1), 3, np.uint32)
    oi, od, og, oc = bsr_mod.merge_top_k_lists_capped(idx, dist, grp, cnt, 5, 2)
    assert oc[0] == 4 and list(oi[0]) == [3, 7, 8, 9, int(IDX_NONE)] and list(og[0]) == [1, 1, 2, 2, 0xFFFFFFFF]
    assert np.isposinf(od[0, 4]) and od[0, 0] == F(0.1)
    L = bsr_mod.lib()
    oi2, od2, oc2 = np.zeros((1, 5), np.uint64), np.zeros((1, 5), F), np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert L.bsr_global_top_k_capped(p(idx), p(dist), p(grp), p(cnt), 2, 1, 3, 5, 2, p(oi2), p(od2), None, p(oc2)) == 0
    assert np.array_equal(oi2, oi) and np.array_equal(oc2, oc)


def test_global_merge_errors(bsr_mod):
    L = bsr_mod.lib()
    idx = np.array([[[3, 7, 9]]], np.uint64)
    dist = np.array([[[0.1, 0.2, 0.5]]], F)
    grp = np.zeros((1, 1, 3), np.uint32)
    cnt = np.full((1, 1), 3, np.uint32)
    oi, od, og, oc = _outs(1, 2)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    call = lambda i, d, g, c, k, m, o=(oi, od, og, oc): L.bsr_global_top_k_capped(  # noqa: E731
        p(i), p(d), p(g), p(c), 1, 1, 3, k, m, p(o[0]), p(o[1]), p(o[2]), p(o[3]))
    assert call(idx, dist, grp, cnt, 2, 0) == -1 and b"per_group" in L.bsr_last_error()
    assert call(idx, dist, grp, cnt, 0, 1) == -1 and b"k must be" in L.bsr_last_error()
    for args in ((None, dist, grp, cnt), (idx, None, grp, cnt), (idx, dist, None, cnt), (idx, dist, grp, None)):
        assert call(*args, 2, 1) == -1 and b"null argument" in L.bsr_last_error()
    for o in ((None, od, og, oc), (oi, None, og, oc), (oi, od, og, None)):
        assert call(idx, dist, grp, cnt, 2, 1, o) == -1 and b"null argument" in L.bsr_last_error()
    nan = dist.copy()
    nan[0, 0, 2] = np.nan
    with pytest.raises(bsr_mod.BsrError) as e:
        bsr_mod.merge_top_k_lists_capped(idx, nan, grp, cnt, 2, 1)
    assert e.value.status == NONFINITE
    assert call(idx, nan, grp, cnt, 2, 1) == NONFINITE and b"NaN distance in query 0" in L.bsr_last_error()
    assert _untouched((oi, od, og, oc))
    # (a NaN behind the count is not an entry)
    cnt2 = np.full((1, 1), 2, np.uint32)
    assert call(idx, nan, grp, cnt2, 2, 1) == 0 and list(oi[0]) == [3, int(IDX_NONE)] and oc[0] == 1
    # no upper cap on per_group; no queries: nothing is read
    assert call(idx, dist, grp, cnt, 2, 2 ** 32 - 1) == 0 and list(oi[0]) == [3, 7]
    assert L.bsr_global_top_k_capped(None, None, None, None, 1, 0, 3, 2, 1, None, None, None, None) == 0


@pytest.mark.parametrize("P", [2, 3, 8])
def test_multi_rank_capped_search_is_the_merge_of_local_ones(bsr_mod, P):
    """A store of 4000 rows in 40 groups split into P shards by interval_by_rank: every shard's
    capped list of length k (the model over the shard's rows, global ids and group ids), merged by
    the library, is the model over the whole store."""
    n, n_groups = 4000, 40
    rng = np.random.default_rng(400 + P)
    rg = rng.integers(0, n_groups, n)
    rg[:300] = 7  # (a long document at the head of rank 0's interval)
    for k, m in ((10, 1), (10, 3), (50, 2)):
        Q = 4
        # distances with ties: 600 levels over 4000 rows; the nearest rows of query 0 all in group 7
        dists = (rng.integers(0, 600, (Q, n)) / F(600)).astype(F)
        dists[0, :300] = (rng.integers(0, 5, 300) / F(6000)).astype(F)
        idx = np.zeros((P, Q, k), np.uint64)
        dist = np.zeros((P, Q, k), F)
        grp = np.zeros((P, Q, k), np.uint32)
        cnt = np.zeros((P, Q), np.uint32)
        for r in range(P):
            iv = bsr_mod.interval_by_rank(r, P, n)
            lo, hi = iv.start_index, iv.end_index
            assert 0 <= lo <= hi <= n
            for q in range(Q):
                idx[r, q], dist[r, q], grp[r, q], cnt[r, q] = kp.cap_model(dists[q, lo:hi], rg[lo:hi], k, m, offset=lo)
        assert sum(bsr_mod.interval_by_rank(r, P, n).get_count() for r in range(P)) == n
        oi, od, og, oc = bsr_mod.merge_top_k_lists_capped(idx, dist, grp, cnt, k, m)
        for q in range(Q):
            wi, wd, wg, wc = kp.cap_model(dists[q], rg, k, m)
            assert oc[q] == wc == k, (P, k, m, q)
            assert np.array_equal(oi[q], wi), (P, k, m, q, oi[q], wi)
            assert np.array_equal(od[q].view(np.uint32), wd.view(np.uint32)) and np.array_equal(og[q], wg)
        # the plain merge of the same lists is not the capped search: query 0's nearest are one group
        if m < k:
            assert np.bincount(og[0]).max() == m
