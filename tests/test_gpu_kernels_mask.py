"""Kernel-level checks of the mask bitset kernels (csrc/k_prep.hip: k_mask_count, k_mask_scan,
k_mask_scatter, k_mask_cut) against the exact numpy models of tests/kcheck.py, through the
test-only shim.  Bitsets only, no corpus rows.

What a wrong kernel here would do silently: the masked searches, the live-row list of a shard with
tombstones and the update's block lists all come from these four kernels; a wrong tail word, a
wrong second round of the scan (more than 256 blocks) or a list written past its length gives
exact results on almost all data the end-to-end tests use.
"""
import numpy as np
import pytest

import kcheck as kc

pytestmark = pytest.mark.gpu

CANARY = np.uint32(0xC0FFEE11)


def _scatter_one(allow, dead, n, blk, n_list):
    """The single-list scatter into a canary-filled buffer: (the n_list words, what lies behind)."""
    buf = np.full(n_list + 4, CANARY, np.uint32)
    kc.mask_scatter(allow, dead, n, blk, buf, n_list=n_list)
    return buf[:n_list], buf[n_list:]


@pytest.mark.parametrize("n", kc.MASK_NS)
def test_single_mask_count_and_list(gpu, n):
    """Every mask kind x every dead kind through launch_mask_list_count / launch_mask_list_scatter
    (one mask, the descriptor passed by value): block prefixes, A and the list."""
    assert kc._mask_lib().kc_mask_block_words() == kc.MASK_BLOCK_WORDS
    assert kc._mask_lib().kc_mask_blocks(n) == kc.mask_blocks(n)
    for kind in kc.MASK_KINDS:
        allow = kc.mask_case(n, kind)
        for dkind in kc.DEAD_KINDS:
            dead = kc.dead_case(n, dkind, allow)
            want_blk, want_ids = kc.mask_list_model(allow, dead, n)
            A = len(want_ids)
            if dkind == "superset":
                assert A == 0
            blk, _ = kc.mask_count(allow, dead, n)
            assert np.array_equal(blk[0], want_blk), (kind, dkind)
            got, behind = _scatter_one(allow, dead, n, blk, A)
            assert np.array_equal(got, want_ids), (kind, dkind)
            assert np.all(behind == CANARY), (kind, dkind)


@pytest.mark.parametrize("n", kc.MASK_NS)
def test_scatter_shorter_than_the_mask_writes_n_list_ids(gpu, n):
    """n_list < A: exactly the first n_list ids, the canary behind them untouched."""
    allow = kc.mask_case(n, "full")
    dead = kc.dead_case(n, "random", allow) if n > 1 else None
    want_blk, want_ids = kc.mask_list_model(allow, dead, n)
    A = len(want_ids)
    assert A >= 1
    blk, _ = kc.mask_count(allow, dead, n)
    assert np.array_equal(blk[0], want_blk)
    for n_list in sorted({0, A // 2, A - 1}):
        got, behind = _scatter_one(allow, dead, n, blk, n_list)
        assert np.array_equal(got, want_ids[:n_list]) and np.all(behind == CANARY), n_list
    # the grouped form of the same: one descriptor, a nonzero offset
    n_list = A // 2
    buf = np.full(3 + n_list + 4, CANARY, np.uint32)
    d = np.array([(3, 0, n_list)], kc.LIST_DESC)
    kc.mask_scatter(allow, dead, n, blk, buf, descs=d)
    assert np.array_equal(buf[3:3 + n_list], want_ids[:n_list])
    assert np.all(buf[:3] == CANARY) and np.all(buf[3 + n_list:] == CANARY)


@pytest.mark.parametrize("n", kc.MASK_NS)
def test_three_masks_counts_lists_and_query_mask_check(gpu, n):
    """n_masks = 3 through launch_mask_groups_count / launch_mask_groups_scatter: device descriptors
    in non-ascending mask order with nonzero offsets; a query_mask with two ids >= n_masks."""
    n_masks = 3
    masks = [kc.mask_case(n, "garbage", seed=1), kc.mask_case(n, "last"), kc.mask_case(n, "half", seed=2)]
    allow = np.concatenate(masks)
    qm = np.array([0, 2, 3, 1, 1, 7, 2, 0], np.uint32)
    for dkind in kc.DEAD_KINDS:
        dead = kc.dead_case(n, dkind, masks[2], seed=3)
        want = [kc.mask_list_model(m, dead, n) for m in masks]
        blk, out = kc.mask_count(allow, dead, n, n_masks=n_masks, query_mask=qm, grouped=True)
        for g in range(n_masks):
            assert np.array_equal(blk[g], want[g][0]), (dkind, g)
            assert out[g] == len(want[g][1]), (dkind, g)
        assert out[n_masks] == 2
        if dkind == "superset":
            assert out[2] == 0
        # without a query_mask the checking workgroup is not launched: out[n_masks] stays as it was
        blk2, out2 = kc.mask_count(allow, dead, n, n_masks=n_masks, grouped=True)
        assert np.array_equal(blk2, blk) and np.array_equal(out2[:n_masks], out[:n_masks])
        assert out2[n_masks] == 0xFFFFFFFF
        # the lists: masks 2, 0, 1 at offsets 5, 5 + A2 + 3, ...
        descs, off = [], 5
        for g in (2, 0, 1):
            descs.append((off, g, len(want[g][1])))
            off += len(want[g][1]) + 3
        d = np.array(descs, kc.LIST_DESC)
        buf = np.full(off + 4, CANARY, np.uint32)
        kc.mask_scatter(allow, dead, n, blk, buf, descs=d)
        written = np.zeros(len(buf), bool)
        for o, g, a in descs:
            assert np.array_equal(buf[o:o + a], want[g][1]), (dkind, g)
            written[o:o + a] = True
        assert np.all(buf[~written] == CANARY), dkind


# ---- the cut ------------------------------------------------------------------------------------
CUT_NQ, CUT_NQ_BUF, CUT_CAP, CUT_N = 5, 8, 130, 1000
CUT_LENS = ((0, 1, 64, 65, CUT_CAP), (CUT_CAP + 1, CUT_CAP, 65, 64, 1))


def _cut_lists(lens, seed):
    """cand [nq_buf][cap] and cnt [nq_buf]: keys with the row in the lower half and distinct upper
    halves; among the counted keys rows >= n (inside the last word, behind it, near 2^32) and
    KEY_NONE.  The slots behind a list's count and the queries >= nq hold a pattern."""
    rng = np.random.default_rng(seed)
    cand = np.full((CUT_NQ_BUF, CUT_CAP), 0x5A5A5A5A5A5A5A5A, np.uint64)
    cnt = np.full(CUT_NQ_BUF, 77, np.uint32)
    for q, c in enumerate(lens):
        cnt[q] = c
        m = min(c, CUT_CAP)
        rows = rng.integers(0, CUT_N, m).astype(np.uint64)
        out_of_range = np.array([CUT_N, CUT_N + 23, 1024, 5000, 0xFFFFFFFE], np.uint64)
        for j in range(3, m, 9):
            rows[j] = out_of_range[(j // 9) % len(out_of_range)]
        upper = (np.arange(m, dtype=np.uint64) * np.uint64(7) + np.uint64(q + 1)) << np.uint64(32)
        keys = upper | rows
        keys[5:m:17] = kc.KEY_NONE
        cand[q, :m] = keys
    return cand, cnt


@pytest.mark.parametrize("lens", CUT_LENS)
@pytest.mark.parametrize("with_qmask", (False, True))
@pytest.mark.parametrize("with_dead", (False, True))
def test_mask_cut(gpu, lens, with_qmask, with_dead):
    n = CUT_N
    n_masks = 3 if with_qmask else 1
    masks = [kc.mask_case(n, "garbage", seed=10 + g) for g in range(n_masks)]
    allow = np.concatenate(masks)
    qm = np.array([2, 0, 1, 2, 0], np.uint32) if with_qmask else None
    dead = kc.dead_case(n, "random", None, seed=20) if with_dead else None
    cand, cnt = _cut_lists(lens, 30)
    cand0, cnt0 = cand.copy(), cnt.copy()
    raw, items = kc.mask_cut(cand, cnt, CUT_NQ, allow, n, n_masks=n_masks, query_mask=qm, dead=dead)
    assert items == CUT_NQ
    kept_any = False
    for q, c in enumerate(lens):
        assert raw[q] == c, "raw[q] holds the emitted count"
        if c > CUT_CAP:  # overflowed: the list and its count untouched
            assert cnt[q] == c and np.array_equal(cand[q], cand0[q])
            continue
        want = kc.mask_cut_model(cand0[q, :c], masks[int(qm[q]) if with_qmask else 0], dead, n)
        assert cnt[q] == len(want), (q, c)
        assert np.array_equal(cand[q, :len(want)], want), (q, c)  # (kept keys, in their order)
        assert np.array_equal(cand[q, c:], cand0[q, c:]), "slots behind the emitted count are not written"
        kept_any |= 0 < len(want) < c
    assert kept_any, "test data: some list must be cut to a shorter, non-empty one"
    # queries >= nq: slots and counters unchanged, raw not written
    assert np.array_equal(cand[CUT_NQ:], cand0[CUT_NQ:]) and np.array_equal(cnt[CUT_NQ:], cnt0[CUT_NQ:])
    assert np.all(raw[CUT_NQ:] == 0xFFFFFFFF)
