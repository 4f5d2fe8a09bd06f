"""The deep MMR search's host side, without a GPU: every step-1 refusal of bsr_local_top_k_deep_mmr on
a null and on a created-but-unloaded index with the outputs untouched, the state check, nq = 0, the
pair counter before any call, and the Python wrapper's default fetch_k."""
import ctypes

import numpy as np
import pytest

from test_mmr_host import ALLOW, NAN, Q, QM, _Stub, _outs, _untouched, fake_index  # noqa: F401

# k, fetch_k, lambda, allow, words, n_masks, query_mask, mode -> the message
REFUSALS = [
    ((0, 4, 0.5, None, 0, 0, None, 0), b"fetch_k"), ((5, 4, 0.5, None, 0, 0, None, 0), b"fetch_k"),
    ((257, 300, 0.5, None, 0, 0, None, 0), b"fetch_k"), ((4, 1025, 0.5, None, 0, 0, None, 0), b"fetch_k"),
    ((2, 4, NAN, None, 0, 0, None, 0), b"lambda"), ((2, 4, -0.1, None, 0, 0, None, 0), b"lambda"),
    ((2, 4, 1.1, None, 0, 0, None, 0), b"lambda"),
    ((2, 4, 0.5, None, 0, 1, None, 0), b"without allow masks"), ((2, 4, 0.5, None, 0, 0, QM, 0), b"without allow masks"),
    ((2, 4, 0.5, ALLOW, 4, 0, None, 0), b"n_masks = 0"), ((2, 4, 0.5, ALLOW, 2, 2, None, 0), b"null query_mask"),
    ((2, 4, 0.5, None, 0, 0, None, 3), b"unknown mask mode 3"),
]


def _call(L, ix, q, nq, args, oi, od, orank, oc):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    k, fetch_k, lam, allow, words, n_masks, qm, mode = args
    return L.bsr_local_top_k_deep_mmr(ix, p(q), nq, k, fetch_k, lam, p(allow), words, n_masks, p(qm), mode, p(oi), p(od),
                                      p(orank), p(oc))


@pytest.mark.parametrize("args,msg", REFUSALS)
def test_refusals(bsr_mod, fake_index, args, msg):
    L = bsr_mod.lib()
    outs = _outs()
    assert _call(L, None, Q, 1, args, *outs) == -1 and b"null index" in L.bsr_last_error()
    for nq in (0, 1):
        assert _call(L, fake_index[0], Q, nq, args, *outs) == -1 and msg in L.bsr_last_error()
    assert _untouched(outs)


def test_null_pointers_state_and_empty_batch(bsr_mod, fake_index):
    L = bsr_mod.lib()
    oi, od, orank, oc = outs = _outs()
    ix = fake_index[0]
    ok = (2, 4, 0.5, None, 0, 0, None, 0)
    assert _call(L, ix, None, 1, ok, *outs) == -1 and b"null queries" in L.bsr_last_error()
    for o in ((None, od, orank, oc), (oi, None, orank, oc), (oi, od, orank, None)):
        assert _call(L, ix, Q, 1, ok, *o) == -1 and b"null output" in L.bsr_last_error()
    # every check of step 1 passed, whatever max_k is (64 here): the index is not loaded
    for args, nq, o in ((ok, 1, (oi, od, None, oc)), ((256, 1024, 1.0, ALLOW, 2, 2, QM, 2), 1, outs),
                        (ok, 0, (None, None, None, None))):
        assert _call(L, ix, Q if nq else None, nq, args, *o) == -7 and b"not loaded" in L.bsr_last_error()
    assert _untouched(outs)
    # no pair was ever computed
    pairs = ctypes.c_uint64(7)
    assert L.bsr_index_last_mmr_pairs(ix, ctypes.byref(pairs)) == 0 and pairs.value == 0
    assert L.bsr_index_last_mmr_pairs(None, ctypes.byref(pairs)) == -1


def test_wrapper_default_fetch_k_and_limits(bsr_mod, monkeypatch):
    s = _Stub(bsr_mod, monkeypatch, 8, max_k=16)
    L = bsr_mod.lib()
    L.bsr_local_top_k_deep_mmr = L.bsr_local_top_k_mmr  # (the recording stand-in)
    q = np.zeros((3, 8), np.float32)
    for k, fk in ((3, 20), (10, 40), (100, 400), (256, 1024)):  # min(1024, max(20, 4 k)), not max_k
        idx, dist, cnt = s.ix.deep_mmr_search(q, k)
        assert idx.shape == (3, k) and s.calls[-1]["fetch_k"] == fk and s.calls[-1]["lam"] == 0.5
    out = s.ix.deep_mmr_search(q, 4, fetch_k=1000, lambda_mult=0.25, return_rank=True)
    assert len(out) == 4 and s.calls[-1]["fetch_k"] == 1000 and s.calls[-1]["rank"] is not None
    n = len(s.calls)
    for kw in (dict(k=0), dict(k=257), dict(k=5, fetch_k=4), dict(k=2, fetch_k=1025), dict(k=2, lambda_mult=NAN)):
        with pytest.raises(bsr_mod.BsrError) as e:
            s.ix.deep_mmr_search(q, **kw)
        assert e.value.status == -1, kw
    assert len(s.calls) == n
    assert bsr_mod.BSR_DEEP_MMR_MAX_PICKS == 256
