"""Kernel-level checks of the certifying form of launch_merge (k_merge_lists with MergeArgs::excl,
csrc/k_exact.hip): strided lists as a global-threshold search gathers them, the merged rows against
the host merge (bsr.merge_top_k_lists, tied to the oracle in test_abi.py) and the failure set
against kx.merge_certify at its decision boundaries, bit for bit.
"""
import numpy as np
import pytest

import kcheck_exact as kx
from kcheck_exact import NEG_INF, POS_INF

pytestmark = pytest.mark.gpu

IFILL, CFILL = np.uint64(0x1111111111111111), np.uint32(0x77777777)
NQ = 16


@pytest.fixture(autouse=True, scope="module")
def _switches_unset():
    kx.assert_no_switches()


def make_lists(rng, P, k, short, disjoint):
    """[P][NQ][k] lists without an index twice within a list; `short`: the queries whose lists hold
    k - 1 entries in all (k = 1: none)."""
    li = np.zeros((P, NQ, k), np.uint64)
    ld = np.zeros((P, NQ, k), np.float32)
    lc = np.zeros((P, NQ), np.uint32)
    vals = np.linspace(0.05, 1.95, 60, dtype=np.float32)  # few distinct distances: ties
    for q in range(NQ):
        counts = rng.multinomial(k - 1, np.full(P, 1.0 / P)) if q in short else np.full(P, k)
        for l in range(P):
            c = int(counts[l])
            ids = rng.permutation(1000 if disjoint else max(300, 2 * k))[:c].astype(np.uint64)
            li[l, q, :c] = ids + np.uint64(l * 1000 if disjoint else 0)
            ld[l, q, :c] = np.sort(rng.choice(vals, c))
            lc[l, q] = c
    return li, ld, lc


def strided(a, stride, fill):
    """[P][...] -> a flat buffer with list l at l * stride."""
    P = a.shape[0]
    per = a[0].size
    out = np.full(P * stride, fill, a.dtype)
    for l in range(P):
        out[l * stride:l * stride + per] = a[l].ravel()
    return out


def run_merge(li, ld, lc, k, excl, need, lists_unique, first_nan=0xFFFFFFFF):
    P, nq, k_in = li.shape
    st = kx.consts()
    s_i, s_d, s_c, s_x, s_s = nq * k_in + 6, nq * k_in + 10, nq + 3, nq + 5, st.st_words + 12
    stw = np.arange(P * st.st_words, dtype=np.uint32).reshape(P, st.st_words) + np.uint32(100)
    o = dict(out_idx=np.full((nq, k), IFILL, np.uint64), out_dist=np.full((nq, k), np.nan, np.float32),
             out_count=np.full(nq, CFILL, np.uint32), first_nan=np.array([first_nan], np.uint32),
             fail_cnt=np.zeros(1, np.uint32), fail_list=np.full(nq + 1, 0xFFFFFFFF, np.uint32),
             st_all=np.full((P, st.st_words), CFILL, np.uint32))
    rc = kx.merge_raw(idx=strided(li, s_i, 0xBAD), dist=strided(ld, s_d, np.nan), cnt=strided(lc, s_c, 0),
                      idx_stride=s_i, dist_stride=s_d, cnt_stride=s_c, P=P, nq=nq, k_in=k_in, k=k,
                      excl=strided(excl, s_x, np.nan), excl_stride=s_x, need=need, lists_unique=lists_unique,
                      st=strided(stw, s_s, 0), st_stride=s_s, **o)
    assert rc == 0
    assert np.array_equal(o["st_all"], stw), "every list's status words, compact"
    return o


def check(bsr_mod, o, li, ld, lc, k, excl, need, skip=()):
    wi, wd, wc = bsr_mod.merge_top_k_lists(li, ld, lc, k)
    failed = []
    for q in range(li.shape[1]):
        if q in skip:
            continue
        assert o["out_count"][q] == wc[q], q
        assert np.array_equal(o["out_idx"][q], wi[q]), q
        assert np.array_equal(o["out_dist"][q].view(np.uint32), wd[q].view(np.uint32)), q
        if not kx.merge_certify(int(wc[q]), wd[q, k - 1], excl[:, q], need, k):
            failed.append(q)
    n = int(o["fail_cnt"][0])
    assert n == len(failed), (n, failed)
    assert sorted(o["fail_list"][:n].tolist()) == failed
    return failed


@pytest.mark.parametrize("P", (1, 2, 8))
@pytest.mark.parametrize("k", (1, 10, 100))
def test_merge_certifies_at_the_boundary(bsr_mod, gpu, P, k):
    rng = np.random.default_rng(100 * P + k)
    short = {4, 5, 6, 12}
    for disjoint in (True, False):
        li, ld, lc = make_lists(rng, P, k, short, disjoint)
        _, wd, wc = bsr_mod.merge_top_k_lists(li, ld, lc, k)
        for need in (k, max(k - 1, 0)):
            excl = np.full((P, NQ), POS_INF, np.float32)
            for q in range(NQ):
                dk = wd[q, k - 1]
                r = int(rng.integers(0, P))  # the list that holds the smallest bound
                kind = q % 8
                if kind == 0:    # the k-th distance one f32 below the smallest bound
                    excl[:, q] = np.nextafter(dk, POS_INF) + np.float32(0.5)
                    excl[r, q] = np.nextafter(dk, POS_INF)
                elif kind == 1:  # equal
                    excl[:, q] = dk + np.float32(0.25)
                    excl[r, q] = dk
                elif kind == 2:  # one f32 above
                    excl[r, q] = np.nextafter(dk, NEG_INF)
                elif kind == 3:  # a NaN bound among infinite ones
                    excl[r, q] = np.nan
                elif kind == 6:  # (short lists) one finite bound
                    excl[r, q] = np.float32(1.99)
                elif kind == 7:  # -inf: a list that overflowed
                    excl[:, q] = np.float32(1.9)
                    excl[r, q] = NEG_INF
                # kinds 4 and 5: every bound +inf
            o = run_merge(li, ld, lc, k, excl, need, lists_unique=1)
            failed = check(bsr_mod, o, li, ld, lc, k, excl, need)
            full = [q for q in range(NQ) if q not in short]
            if disjoint:  # (no index twice: every full query's merged list is full, every short one holds k - 1)
                assert all(q not in failed for q in full if q % 8 == 0), "strictly below every bound: certified"
                assert all(q in failed for q in full if q % 8 in (1, 2, 3, 7))
                if need == k:
                    assert short <= set(failed), "got < need"
                else:  # a short list: certified only when every bound is +inf
                    assert not {4, 5, 12} & set(failed) and 6 in failed
            assert o["first_nan"][0] == 0xFFFFFFFF
            # lists_unique only allows a shortcut: the same rows without it
            o2 = run_merge(li, ld, lc, k, excl, need, lists_unique=0)
            for name in ("out_idx", "out_dist", "out_count"):
                assert np.array_equal(o[name].view(np.uint8), o2[name].view(np.uint8)), name
            assert sorted(o2["fail_list"][:o2["fail_cnt"][0]].tolist()) == failed


def test_merge_first_nan(bsr_mod, gpu):
    """A NaN distance: the query's count is 0, its rows (~0, +inf), the lowest such query in
    *first_nan; it is neither certified nor reported as failed; the other queries are unaffected."""
    rng = np.random.default_rng(9)
    P, k = 4, 10
    li, ld, lc = make_lists(rng, P, k, set(), True)
    ld[2, 11, 3] = np.nan
    ld[0, 6, 9] = np.nan
    excl = np.full((P, NQ), POS_INF, np.float32)
    excl[1, 3] = NEG_INF
    o = run_merge(li, ld, lc, k, excl, k, lists_unique=1)
    assert o["first_nan"][0] == 6
    for q in (6, 11):
        assert o["out_count"][q] == 0 and (o["out_idx"][q] == kx.IDX_NONE).all() and np.isposinf(o["out_dist"][q]).all()
    clean = ld.copy()
    clean[np.isnan(clean)] = 0.5
    assert check(bsr_mod, o, li, clean, lc, k, excl, k, skip=(6, 11)) == [3]
