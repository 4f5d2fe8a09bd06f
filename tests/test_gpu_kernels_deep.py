"""launch_deep_select (csrc/k_exact.hip) through its test-only shim (tests/kcheck/kcheck_deep.cpp ->
lib/libbsr_kcheck_deep.so): the selection against numpy.sort of the u64 keys, and the certification
against a float64 restatement of exclusion_bound().  No tolerance: keys are integers, and the bound
is the same IEEE double arithmetic in both."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F, U64 = np.float32, np.uint64
NONE = U64(2 ** 64 - 1)
OFFSET = 1 << 33
LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "better-search-rag-rust_amd", "lib",
                   "libbsr_kcheck_deep.so")


def deep_select(keys, k, kcnt=None, tau=None, ebound=None, nb=None, emit_cnt=None, cap=0):
    """(idx, dist, count, failed ids in ascending order) with pattern-filled outputs."""
    lib = ctypes.CDLL(LIB)
    ni, n_keys = keys.shape
    idx, dist, cnt = np.full((ni, k), 0x1234, U64), np.full((ni, k), -3.0, F), np.full(ni, 0x5A5A, np.uint32)
    fail, status = np.full(ni, 0xFFFF, np.uint32), np.zeros(4, np.uint32)
    arrs = [np.ascontiguousarray(keys, U64), kcnt, tau, ebound, nb, emit_cnt, idx, dist, cnt, fail, status]
    p = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrs]
    u32 = ctypes.c_uint32
    rc = lib.kc_deep_select(p[0], p[1], u32(n_keys), u32(ni), u32(k), ctypes.c_uint64(OFFSET), p[2], p[3], p[4], p[5],
                            u32(cap), p[6], p[7], p[8], p[9], p[10])
    assert rc == 0, f"hipError_t {rc}"
    return idx, dist, cnt, np.sort(fail[:status[0]])


def want_row(keys, k):
    s = np.sort(keys[keys != NONE])[:k]
    idx, dist = np.full(k, NONE, U64), np.full(k, np.inf, F)
    idx[:len(s)] = U64(OFFSET) + (s & U64(0xFFFFFFFF))
    dist[:len(s)] = (s >> U64(32)).astype(np.uint32).view(F)
    return idx, dist, len(s)


def make_keys(rng, kind, c):
    """c distinct keys: random distances and rows with empty slots among them; keys that share all but
    their low 16 bits (six radix passes); one distance, the keys differing only in the row half."""
    if kind == "low_bits":
        return (U64(0x3F0C1234) << U64(32)) | U64(0x5678_0000) | rng.permutation(1 << 16)[:c].astype(U64)
    rows = rng.permutation(1 << 20)[:c].astype(U64)
    if kind == "row_half":
        return (U64(0x3F0C1234) << U64(32)) | rows
    keys = (rng.uniform(0, 2, c).astype(F).view(np.uint32).astype(U64) << U64(32)) | rows
    keys[rng.random(c) < 0.05] = NONE
    return keys


@pytest.mark.parametrize("kind", ["random", "low_bits", "row_half"])
@pytest.mark.parametrize("c", [1, 63, 2048, 2049, 16384, 40_000])
def test_select_against_sort(gpu, c, kind):
    rng = np.random.default_rng(c)
    keys = np.stack([make_keys(rng, kind, c) for _ in range(3)])
    for k in (1000, 1024) if c == 2049 else (1000,):
        idx, dist, cnt, failed = deep_select(keys, k)
        assert len(failed) == 0
        for i in range(3):
            wi, wd, wc = want_row(keys[i], k)
            assert cnt[i] == wc and np.array_equal(idx[i], wi) and np.array_equal(dist[i].view(np.uint32),
                                                                                  wd.view(np.uint32))


def bound_model(tx, eb, mag_b):
    """exclusion_bound() in float64, rounded down to f32."""
    tx, eb, mag_b = float(tx), float(eb), float(mag_b)
    if tx == -np.inf:
        return np.inf
    if not tx < np.inf or not eb < 1.0 or not tx < 1.0 - eb - 1e-4 - 6e-9 / mag_b:
        return -np.inf
    x = 1.0 - tx - eb - 2.5e-7
    xf = F(x)
    return float(np.nextafter(xf, F(-np.inf)) if float(xf) > x else xf)


def test_certification_boundary(gpu):
    rng = np.random.default_rng(5)
    k, c, cap, ni = 100, 300, 512, 8
    keys = np.stack([make_keys(rng, "row_half", c) for _ in range(ni)])
    keys = (keys & U64(0xFFFFFFFF)) | (rng.uniform(0.3, 0.9, (ni, c)).astype(F).view(np.uint32).astype(U64) << U64(32))
    dk = [float(want_row(keys[i], k)[1][k - 1]) for i in range(ni)]
    eb, nb = np.full(ni, 0.01, F), np.ones(ni, F)
    kcnt, emit = np.full(ni, c, np.uint32), np.full(ni, c, np.uint32)
    # items 0-3: the four f32 thresholds nearest the one where the bound equals the k-th distance
    tau = np.full(ni, 0.05, F)  # (items 4-7: a threshold that certifies by a wide margin)
    t = F(1.0 - dk[0] - 0.01 - 2.5e-7)
    while dk[0] < bound_model(t, eb[0], 1.0):
        t = np.nextafter(t, F(2))
    while not dk[0] < bound_model(t, eb[0], 1.0):
        t = np.nextafter(t, F(-1))  # (now the largest threshold that certifies)
    keys[1:4] = keys[0]
    tau[:4] = [np.nextafter(t, F(-1)), t, np.nextafter(t, F(2)), np.nextafter(np.nextafter(t, F(2)), F(2))]
    emit[4] = cap + 1      # an overflowed list
    kcnt[5] = k - 1        # fewer keys than k
    tau[6] = -np.inf       # every row was a candidate
    rejected = [i for i in range(ni) if emit[i] > cap or kcnt[i] < k or
                not dk[0 if i < 4 else i] < bound_model(tau[i], eb[i], nb[i])]
    assert 4 in rejected and 5 in rejected and 0 < len([i for i in rejected if i < 4]) < 4  # (both outcomes)
    idx, dist, cnt, failed = deep_select(keys, k, kcnt, tau, eb, nb, emit, cap)
    assert failed.tolist() == rejected
    for i in range(ni):
        if i in rejected:
            assert np.all(idx[i] == 0x1234) and np.all(dist[i] == -3.0) and cnt[i] == 0x5A5A  # (nothing written)
        else:
            wi, wd, wc = want_row(keys[i], k)
            assert cnt[i] == wc == k and np.array_equal(idx[i], wi) and np.array_equal(dist[i], wd)
