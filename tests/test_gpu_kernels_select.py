"""Kernel-level checks of the selection kernels of the candidate stage (csrc/k_filter.hip):
launch_select_tau in its four builds, launch_global_tau in both and launch_select_cand for every
E = 1 .. 10, against order statistics computed with numpy (tests/kcheck.py), bit for bit.

The builds are reached through the launcher's own conditions (BSR_SELECT_TAU_M unset):
  k_select_tau_w<32>   n_s <= 2048, ks <= 64, qpad % 4 == 0
  k_select_tau_m<16>   qpad <= 16, 2048 < n_s <= 16384, ks <= 64
  k_select_tau<1>      otherwise, ks <= 64
  k_select_tau<2>      64 < ks <= 128
"""
import os

import numpy as np
import pytest

import kcheck as kc

pytestmark = pytest.mark.gpu

NEG_INF, POS_INF = np.float32(-np.inf), np.float32(np.inf)
N_S = (63, 64, 65, 2047, 2048, 2049, 16384, 16385)


def _build(qpad, n_s, ks):
    if ks > 64:
        return "tau<2>"
    if qpad <= 16 and 2048 < n_s <= 16384:
        return "tau_m<16>"
    if n_s <= 2048 and qpad % 4 == 0:
        return "tau_w<32>"
    return "tau<1>"


def _sample_rows(rng, nq, n_s, s_ld, ks, qpad):
    """S [qpad][s_ld]: per query one of the row patterns; past n_s a region of -inf and a region of
    values above every score (the clamped duplicates a sample kernel leaves there): both ignored."""
    S = np.zeros((qpad, s_ld), np.float32)
    S[:, n_s:] = NEG_INF
    S[:, n_s + (s_ld - n_s) // 2:] = 9.0
    for q in range(nq):
        kind = q % 8
        if kind == 0:
            v = rng.normal(0, 0.05, n_s)
        elif kind == 1:  # all equal
            v = np.full(n_s, 0.125)
        elif kind == 2:  # ks - 1 copies of the maximum, then a plateau across the ks-th place
            v = rng.uniform(-0.5, 0.1, n_s)
            pos = rng.permutation(n_s)
            v[pos[:ks - 1]] = 0.75
            v[pos[ks - 1:ks - 1 + min(n_s - ks + 1, 40)]] = 0.25
        elif kind == 3:  # +-0.0 only
            v = np.where(rng.integers(0, 2, n_s) == 1, 0.0, -0.0)
        elif kind == 4:  # negative only
            v = -np.abs(rng.normal(0, 0.05, n_s)) - 1e-3
        elif kind == 5:  # few distinct values: ties everywhere
            v = rng.integers(-3, 4, n_s) / 16.0
        elif kind == 6:  # one spike per 64 values: the lane maxima carry the whole selection
            v = rng.normal(0, 0.01, n_s)
            v[::64] = 0.5 + rng.uniform(0, 0.1, len(v[::64]))
        else:  # descending, then ascending: every best value in one wave's share
            v = np.linspace(1, -1, n_s) if q % 16 == 7 else np.linspace(-1, 1, n_s)
        S[q, :n_s] = v.astype(np.float32)
    return S


def _check_select_tau(S, n_s, nq, qflags, ks):
    qpad = len(qflags)
    c = kc.consts()
    tau, cnt, status, smax = kc.select_tau(S, n_s, nq, qflags, ks)
    none = np.arange(qpad) >= nq
    none |= (qflags & kc.Q_NOAPPROX) != 0
    assert np.all(tau[none] == POS_INF), "flagged and padding queries: tau = +inf"
    assert np.all(smax[none] == kc.KEY_NONE)
    live = np.flatnonzero(~none)
    if n_s < ks:
        assert np.all(tau[live] == NEG_INF) and np.all(smax[live] == kc.KEY_NONE)
    else:
        want_tau, want_keys = kc.kth_largest(S[live, :n_s], ks)
        assert np.array_equal(tau[live].view(np.uint32), want_tau.view(np.uint32)), \
            f"tau differs for queries {live[tau[live].view(np.uint32) != want_tau.view(np.uint32)]}"
        assert np.array_equal(smax[live], want_keys), "smax: the ks smallest keys, ascending"
    assert not cnt.any(), "cnt[0 .. qpad), the tail counters and the gang words are zeroed"
    want_st = np.full(c.st_words, 0xFFFFFFFF, np.uint32)
    want_st[[c.st_fail, c.st_emitted, c.st_fail2]] = 0
    assert np.array_equal(status, want_st)


@pytest.mark.parametrize("ks", (1, 8, 24, 48, 64, 65, 128))
def test_select_tau(gpu, ks):
    assert os.environ.get("BSR_SELECT_TAU_M") is None
    rng = np.random.default_rng(4200 + ks)
    seen = set()
    for qpad, nq in ((16, 14), (256, 19)):
        qflags = np.zeros(qpad, np.uint32)
        qflags[nq:] = kc.Q_NOAPPROX
        qflags[5] = kc.Q_NOAPPROX
        qflags[11] = kc.Q_NOAPPROX | kc.Q_NONFINITE
        for n_s in sorted(set(N_S + (ks - 1, ks, ks + 1)) - {0}):
            if qpad == 256 and n_s == 16384:
                continue  # (16385 reaches the same build at this batch size)
            s_ld = kc.round_up(n_s + 70, 64)
            S = _sample_rows(rng, nq, n_s, s_ld, ks, qpad)
            _check_select_tau(S, n_s, nq, qflags, ks)
            seen.add(_build(qpad, n_s, ks))
    want = {"tau<2>"} if ks > 64 else {"tau_w<32>", "tau_m<16>", "tau<1>"}
    assert seen == want, seen


@pytest.mark.parametrize("qpad,nq", ((16, 3), (256, 200)))
def test_select_tau_without_sample(gpu, qpad, nq):
    """sample_pass's call for a shard no larger than a list: S = nullptr, n_s = 0."""
    qflags = np.zeros(qpad, np.uint32)
    qflags[nq:] = kc.Q_NOAPPROX
    qflags[1] = kc.Q_NOAPPROX
    _check_select_tau(None, 0, nq, qflags, 8)


@pytest.mark.parametrize("ks", (8, 64, 65, 128))
def test_global_tau(gpu, ks):
    """tau = the score of the ks-th smallest of the P ranks' gathered keys; kKeyNone entries (a rank
    whose shard has fewer than ks sample values, a query it does not serve) are no keys; the same
    score -- and the same key -- may come from several ranks."""
    rng = np.random.default_rng(900 + ks)
    qpad, nq = 256, 37
    qflags = np.zeros(qpad, np.uint32)
    qflags[nq:] = kc.Q_NOAPPROX
    qflags[4] = kc.Q_NOAPPROX
    for P in (1, 2, 8):
        g = np.full((P, qpad, ks), kc.KEY_NONE, np.uint64)
        for r in range(P):
            vals = (rng.integers(-8, 9, (nq, 3 * ks)) / 64.0).astype(np.float32)  # duplicated scores
            _, best = kc.kth_largest(vals, ks)
            g[r, :nq] = best
        g[P - 1, 0] = kc.KEY_NONE        # query 0: one rank has nothing
        g[:, 1] = kc.KEY_NONE            # query 1: fewer than ks keys anywhere (none)
        g[:, 2, ks // 2:] = kc.KEY_NONE  # query 2: every rank holds half a list
        if P > 1:
            g[1, 3] = g[0, 3]            # query 3: two ranks with identical keys
        tau = kc.global_tau(g, nq, qflags)
        for q in range(qpad):
            if q >= nq or qflags[q]:
                assert tau[q] == POS_INF, q
                continue
            keys = np.sort(g[:, q].ravel())
            want = NEG_INF if keys[ks - 1] == kc.KEY_NONE else kc.score_key_score(keys[ks - 1])
            assert tau[q].view(np.uint32) == np.float32(want).view(np.uint32), (P, q, tau[q], want)


@pytest.mark.parametrize("E", range(1, 11))
def test_select_cand(gpu, E):
    """k_select_cand<E>, kp = 64 E - 1.  What the kernel documents, and the rescore expects:
    cand_rows[q][0 .. ncand) are the rows of the kp smallest keys in ascending key order (score
    descending, row ascending), ncand = min(kp, cnt), tau_excl = the (kp + 1)-th score, or tau[q]
    when no more than kp were emitted.  An overflowed list (cnt > cap: rows were dropped) gets
    ncand = 0 and tau_excl = +inf -- nothing can be certified -- and its cand_rows are not written."""
    kp = 64 * E - 1
    cap = 16 * (kp + 1)
    rng = np.random.default_rng(7000 + E)
    counts = [0, 1, kp - 1, kp, kp + 1, cap, cap + 5]
    nq, nq_buf = len(counts), 16
    cand = np.full((nq_buf, cap), 0xDEAD, np.uint64)
    cnt = np.zeros(nq_buf, np.uint32)
    tau = rng.uniform(-1, 0, nq_buf).astype(np.float32)
    for q, c in enumerate(counts):
        m = min(c, cap)
        scores = (rng.integers(-20, 21, m) / 128.0).astype(np.float32)  # duplicate scores
        rows = rng.permutation(1 << 20)[:m].astype(np.uint64)
        cand[q, :m] = kc.score_key(scores, rows)
        cnt[q] = c
    rows_out, ncand, tau_excl = kc.select_cand(cand, cnt, nq, tau, kp)
    for q, c in enumerate(counts):
        if c > cap:
            assert ncand[q] == 0 and tau_excl[q] == POS_INF
            assert np.all(rows_out[q] == 0xFFFFFFFF)
            continue
        keys = np.sort(cand[q, :c])
        nc = min(kp, c)
        assert ncand[q] == nc, (q, c)
        assert np.array_equal(rows_out[q, :nc], kc.key_row(keys[:nc])), (q, c)
        assert np.all(rows_out[q, nc:] == 0xFFFFFFFF)
        want = kc.score_key_score(keys[kp]) if c > kp else tau[q]
        assert tau_excl[q].view(np.uint32) == np.float32(want).view(np.uint32), (q, c)
