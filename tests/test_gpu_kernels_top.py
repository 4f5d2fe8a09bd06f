"""Kernel-level checks of the self-thresholded lists (launch_filter_skinny_top, csrc/k_filter.hip):
k_filter_skinny2<Top, 4 | 12 | 16> and k_filter_skinny_glds<Top, 12>, called as top_pass does
(index.cpp): the emit operand (one scale per 32 rows), top_layout = 2, cap = 4 W slots per query with
W = skinny_top_lists(n), status words present.  The product only takes this path from
kSkinnyTopMinRows = 2^21 rows, so these are the smallest shapes in its contract.

Checked, with W lists of 4 keys per query:
  * every list ascending, cnt[q] = 4 W for q < 16, the status words kStFail / kStEmitted / kStFail2
    zeroed, queries >= n_q with no key at all;
  * the union of a query's lists holds the model's 4 best keys of the whole shard;
  * the WORKGROUP form of the contract "every other row of the workgroup scores at most its 4th":
    workgroup b owns the rows of the 16-row units u = b (mod W) under the strided-pair layout
    (kcheck.top_workgroup_rows), and no row of b outside b's list scores strictly above the score of
    b's 4th key.  (In scores, as the kernel documents it: a row that ties the 4th key's score may stay
    out whatever its row id.)
The operand is data (d) -- synthetic int8 with arbitrary block scales -- plus a cluster: a query's
six best rows planted consecutively, which the strided pairs must spread over several lists.
"""
import numpy as np
import pytest

import kcheck as kc

pytestmark = pytest.mark.gpu

N0 = 1 << 21
_cache = {}


def _case(n, row_bytes):
    """(A, a_scale, B, b_scale, keys [16][n]) -- the operand and the model's keys; one case is kept."""
    if (n, row_bytes) in _cache:
        return _cache[(n, row_bytes)]
    _cache.clear()
    rng = np.random.default_rng(50000 + row_bytes + (n - N0))
    n_pad = kc.round_up(n, 256)
    # 2^17 random rows, repeated with the columns rotated by 8 bytes more each time (generating 2M
    # independent rows takes longer than everything else in the test)
    blk = rng.integers(-127, 128, (1 << 17, row_bytes), dtype=np.int8)
    A = np.zeros((n_pad, row_bytes), np.int8)
    for t, r in enumerate(range(0, n, 1 << 17)):
        m = min(1 << 17, n - r)
        sh = (8 * t) % row_bytes
        A[r:r + m, sh:] = blk[:m, :row_bytes - sh]
        A[r:r + m, :sh] = blk[:m, row_bytes - sh:]
    A[n // 2] = 127
    A[n // 2 + 1] = -127
    A[n // 3] = 0
    A[n - 1] = 0
    for start in (n // 5, 2 * n // 3):
        A[start:start + 400] = A[start]
    a_scale = np.ones(n_pad // 32, np.float32)
    nv = (n + 31) // 32
    a_scale[:nv] = np.exp(rng.uniform(np.log(1e-4), np.log(9e-2), nv)).astype(np.float32)
    B, b_scale = kc.synth_queries(rng, 16, 16, row_bytes)
    # the cluster: query 1's six best rows, consecutive, in a block with the largest scale
    r0 = 32 * (n // 64) + 5
    for j in range(6):
        A[r0 + j] = B[1]
        A[r0 + j, :8 * j] = 0
    a_scale[r0 // 32] = np.float32(0.1)
    M = kc.score(kc.idot(A[:n], B), kc.row_scales(a_scale, 32, n), b_scale)  # [row][query]
    keys = kc.score_key(np.ascontiguousarray(M.T), np.arange(n, dtype=np.uint64)[None, :])
    assert kc.key_row(np.sort(keys[1])[:6]).tolist() == list(range(r0, r0 + 6)), "test data: the cluster is query 1's top 6"
    _cache[(n, row_bytes)] = (A, a_scale, B, b_scale, keys)
    return _cache[(n, row_bytes)]


def _run_top(A, a_scale, n, B, b_scale, n_q):
    W = kc.lib().kc_skinny_top_lists(n)
    cap = 4 * W
    cand = np.full((16, cap), 0xEEEEEEEEEEEEEEEE, np.uint64)
    cnt = np.full(kc.cnt_words(16), 0xFFFFFFFF, np.uint32)
    status = np.full(kc.consts().st_words, 0xFFFFFFFF, np.uint32)
    kc.gemm(kc.SKINNY_TOP, A=A, n_rows=n, a_scale_rows=32, B=B, a_scale=a_scale, b_scale=b_scale, n_qt=0,
            cand=cand, cnt=cnt, cap=cap, status=status, n_q=n_q, top_layout=2, n_rt=(n + 255) // 256)
    return W, cand, cnt, status


def _check_top(n, row_bytes, n_q):
    A, a_scale, B, b_scale, keys = _case(n, row_bytes)
    W, cand, cnt, status = _run_top(A, a_scale, n, B, b_scale, n_q)
    c = kc.consts()
    assert W == 512
    assert np.all(cnt[:16] == 4 * W) and np.all(cnt[16:] == 0xFFFFFFFF)
    want_st = np.full(c.st_words, 0xFFFFFFFF, np.uint32)
    want_st[[c.st_fail, c.st_emitted, c.st_fail2]] = 0
    assert np.array_equal(status, want_st)
    lists = cand.reshape(16, W, 4)
    assert np.all(lists[n_q:] == kc.KEY_NONE), "queries >= n_q keep no list"
    wg = kc.top_workgroup_rows(n, W)
    for q in range(n_q):
        L = lists[q]
        assert np.all(L[:, :-1] < L[:, 1:]), f"query {q}: a list is not strictly ascending"
        union = L.ravel()
        assert np.all(union != kc.KEY_NONE), "2^21 rows: every workgroup holds more than 4"
        assert np.all(wg[kc.key_row(union)] == np.repeat(np.arange(W), 4)), f"query {q}: a key outside its workgroup's rows"
        assert np.isin(union, keys[q]).all(), f"query {q}: a key that is no (score, row) of the model"
        best4 = np.partition(keys[q], 3)[:4]
        assert np.isin(best4, union).all(), f"query {q}: the shard's 4 best keys are not all in the lists"
        s4 = kc.score_key_score(L[:, 3])  # per workgroup, the score of its 4th key
        sq = kc.score_key_score(keys[q])
        above = np.flatnonzero(sq > s4[wg])  # rows scoring strictly above their workgroup's 4th
        assert np.isin(keys[q][above], union).all(), \
            f"query {q}: {np.count_nonzero(~np.isin(keys[q][above], union))} rows above their workgroup's 4th key are in no list"


@pytest.mark.parametrize("n,glds", ((N0, None), (N0, "0"), (N0 + 4099, None), (N0 + 4099, "0")))
def test_top_lists_768(gpu, monkeypatch, n, glds):
    """768-byte rows: k_filter_skinny_glds<Top, 12>, and k_filter_skinny2<Top, 12> with
    BSR_SKINNY_GLDS=0; 16 queries, and 5 (queries >= n_q keep no list)."""
    if glds is None:
        monkeypatch.delenv("BSR_SKINNY_GLDS", raising=False)
    else:
        monkeypatch.setenv("BSR_SKINNY_GLDS", glds)
    _check_top(n, 768, 16)
    if n == N0:
        _check_top(n, 768, 5)


@pytest.mark.parametrize("row_bytes", (256, 1024))
def test_top_lists_other_widths(gpu, monkeypatch, row_bytes):
    """k_filter_skinny2<Top, 4> and <Top, 16> at 2^21 rows (the second n is dropped for these
    widths: the model of a 2M-row shard takes seconds)."""
    monkeypatch.delenv("BSR_SKINNY_GLDS", raising=False)
    _check_top(N0, row_bytes, 16)
