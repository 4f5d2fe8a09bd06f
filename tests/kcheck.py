"""Kernel-level checks of the int8 candidate stage: the ctypes loader of the test-only shim
(tests/kcheck/kcheck.cpp -> lib/libbsr_kcheck.so) and exact numpy models of every kernel's
contract (csrc/k_prep.hip, csrc/k_filter.hip).

The models need no tolerance: the filter's integer dot product is exact, its score is two
separately rounded f32 multiplies, keys are bit manipulations and the selections are order
statistics.  Only the quantisation divides by a norm whose summation order the kernel is free to
choose; `compare_quant` states the one excuse that allows (an element within 1e-9 of a rounding
tie, a scale within a relative 1e-12 of an f32 value) and counts its uses.

tests/test_kernel_models.py pins the models themselves with hand-derived cases (CPU);
tests/test_gpu_kernels_*.py compare the kernels with them.
"""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "better-search-rag-rust_amd", "lib", "libbsr_kcheck.so")

KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
Q_NONFINITE, Q_NOAPPROX = 1, 2

# launch kinds of kc_gemm (kcheck.cpp)
SAMPLE, EMIT, SKINNY_SAMPLE, SKINNY_EMIT, SKINNY_TOP, FIXUP = range(6)


# ----------------------------------------------------------------------------------------
# Loader
# ----------------------------------------------------------------------------------------
class _Consts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "ld_align", "row_pad", "quant_block", "sample_stride", "sample_scale_rows", "filter_tile",
        "tail_counters", "gang_words", "gang_min_tiles", "sample_tile_every", "sample_tile_phase",
        "skinny_max_q", "fused_select_cap", "st_words", "st_fail", "st_emitted", "st_query_flags",
        "st_fail2")] + [("skinny_top_min_rows", ctypes.c_uint64)]


class _Gemm(ctypes.Structure):
    _fields_ = [
        ("A", ctypes.c_void_p), ("a_bytes", ctypes.c_uint64), ("a_stride", ctypes.c_uint64),
        ("n_rows", ctypes.c_uint32), ("a_scale_rows", ctypes.c_uint32),
        ("B", ctypes.c_void_p), ("b_bytes", ctypes.c_uint64),
        ("row_bytes", ctypes.c_uint32), ("n_rt", ctypes.c_uint32), ("n_qt", ctypes.c_uint32),
        ("a_scale", ctypes.c_void_p), ("a_scale_bytes", ctypes.c_uint64),
        ("b_scale", ctypes.c_void_p), ("b_scale_bytes", ctypes.c_uint64),
        ("S", ctypes.c_void_p), ("s_bytes", ctypes.c_uint64), ("s_ld", ctypes.c_uint32), ("s_compact", ctypes.c_uint32),
        ("tau", ctypes.c_void_p), ("tau_bytes", ctypes.c_uint64),
        ("cand", ctypes.c_void_p), ("cand_bytes", ctypes.c_uint64),
        ("cnt", ctypes.c_void_p), ("cnt_bytes", ctypes.c_uint64), ("cap", ctypes.c_uint32), ("tail_off", ctypes.c_int32),
        ("status", ctypes.c_void_p), ("status_bytes", ctypes.c_uint64),
        ("n_q", ctypes.c_uint32), ("top_layout", ctypes.c_uint32), ("s_tiles", ctypes.c_uint32), ("s_vals", ctypes.c_uint32),
    ]


_lib = None
_consts = None


def lib() -> ctypes.CDLL:
    """libbsr_kcheck.so (raises if it has not been built: the tests have no other path).  Load it
    after the `gpu` fixture, i.e. after torch's HIP runtime and libbsr.so (tests/conftest.py)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built (run __graft_entry__.build())")
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.kc_skinny_top_lists.restype = ctypes.c_uint32
        _lib.kc_skinny_top_lists.argtypes = [ctypes.c_uint32]
        _lib.kc_sample_tiles_for.restype = ctypes.c_uint32
        _lib.kc_sample_tiles_for.argtypes = [ctypes.c_uint64]
    return _lib


def consts() -> _Consts:
    global _consts
    if _consts is None:
        _consts = _Consts()
        lib().kc_consts(ctypes.byref(_consts))
    return _consts


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: hipError_t {rc}")


def _own(a, dtype):
    assert a is None or (a.dtype == dtype and a.flags.c_contiguous), (dtype, None if a is None else a.dtype)
    return a


def round_up(x, m):
    return (x + m - 1) // m * m


def ld_for(dim):
    return round_up(dim, 64)


def slab(rows, n_pad=None):
    """The index's f32 slab: [round_up(n, 256)][ld], zero padded (bsr_index_load_impl)."""
    n, dim = rows.shape
    n_pad = n_pad or round_up(max(n, 1), 256)
    out = np.zeros((n_pad, ld_for(dim)), np.float32)
    out[:n, :dim] = rows
    return out


def rows_to_i8(rows):
    """launch_rows_to_i8 as index_finish_load calls it.  Returns (op [n_pad][ld] int8, scales
    [n_pad / 32] f32, ea_max f32).  The outputs start as 0x5A / NaN patterns."""
    n, dim = rows.shape
    s = slab(rows)
    n_pad, ld = s.shape
    op = np.full((n_pad, ld), 0x5A, np.int8)
    sc = np.full(n_pad // 32, np.nan, np.float32)
    ea = np.zeros(1, np.uint32)
    _check(lib().kc_rows_to_i8(_p(s), ctypes.c_uint64(n), ctypes.c_uint64(n_pad), ctypes.c_uint32(dim),
                               ctypes.c_uint32(ld), _p(op), _p(sc), _p(ea)), "rows_to_i8")
    return op, sc, ea.view(np.float32)[0]


def rows_to_i8_sample(rows):
    """launch_rows_to_i8_sample as index_finish_load calls it: (op [n_s_pad][ld], scales [n_s_pad / 128])."""
    n, dim = rows.shape
    s = slab(rows)
    n_pad, ld = s.shape
    n_s = (n + 31) // 32
    n_s_pad = round_up(max(n_s, 1), 128)
    op = np.full((n_s_pad, ld), 0x5A, np.int8)
    sc = np.full(n_s_pad // 128, np.nan, np.float32)
    _check(lib().kc_rows_to_i8_sample(_p(s), ctypes.c_uint64(n), ctypes.c_uint64(n_pad), ctypes.c_uint32(dim),
                                      ctypes.c_uint32(ld), _p(op), _p(sc), ctypes.c_uint64(n_s_pad)), "rows_to_i8_sample")
    return op, sc


def qpad_for(nq):
    return 16 if nq <= 16 else round_up(nq, 256)


def query_prep(q, ea_max, with_op=True, status_in=0):
    """launch_query_prep as search_device calls it.  Returns a dict of the output buffers; each
    starts as a pattern (0x5A bytes / NaN / 0xFFFFFFFF) so that untouched words show."""
    nq, dim = q.shape
    qpad, ld = qpad_for(nq), ld_for(dim)
    o = dict(
        qf32=np.full((qpad, ld), np.nan, np.float32), nb=np.full(qpad, np.nan, np.float32),
        qop=np.full((qpad, ld), 0x5A, np.int8), qscale=np.full(qpad, np.nan, np.float32),
        ebound=np.full(qpad, np.nan, np.float32), qflags=np.full(qpad, 0xFFFFFFFF, np.uint32),
        qids=np.full(qpad, -7, np.int32), status=np.full(consts().st_words, status_in, np.uint32))
    ea = np.array([ea_max], np.float32).view(np.uint32)
    qc = np.ascontiguousarray(q, np.float32)
    _check(lib().kc_query_prep(_p(qc), ctypes.c_uint32(nq), ctypes.c_uint32(qpad), ctypes.c_uint32(dim),
                               ctypes.c_uint32(ld), _p(ea), _p(o["qf32"]), _p(o["nb"]), _p(o["qop"]), _p(o["qscale"]),
                               _p(o["ebound"]), _p(o["qflags"]), _p(o["qids"]), _p(o["status"]),
                               ctypes.c_int(1 if with_op else 0)), "query_prep")
    o["qpad"], o["ld"] = qpad, ld
    return o


def cnt_words(qpad):
    c = consts()
    return qpad + 8 * c.tail_counters + c.gang_words


def gemm(kind, *, A, n_rows, a_scale_rows, B, a_scale, b_scale, n_qt, S=None, s_ld=0, s_compact=0, tau=None,
         cand=None, cnt=None, cap=0, tail=False, status=None, n_q=0, top_layout=0, s_tiles=0, s_vals=0, n_rt=0):
    """One filter launch (kc_gemm).  A [rows][row_bytes] int8, B [qpad][row_bytes] int8; S, cand,
    cnt and status are written in place."""
    g = _Gemm()
    A, B = _own(A, np.int8), _own(B, np.int8)
    a_scale, b_scale = _own(a_scale, np.float32), _own(b_scale, np.float32)
    S, tau = _own(S, np.float32), _own(tau, np.float32)
    cand, cnt, status = _own(cand, np.uint64), _own(cnt, np.uint32), _own(status, np.uint32)
    row_bytes = A.shape[1]
    assert row_bytes % 64 == 0 and B.shape[1] == row_bytes
    for name, arr in (("A", A), ("B", B), ("a_scale", a_scale), ("b_scale", b_scale), ("S", S), ("tau", tau),
                      ("cand", cand), ("cnt", cnt), ("status", status)):
        setattr(g, name, None if arr is None else arr.ctypes.data)
    g.a_bytes, g.b_bytes = A.nbytes, B.nbytes
    g.a_scale_bytes, g.b_scale_bytes = a_scale.nbytes, b_scale.nbytes
    g.s_bytes = 0 if S is None else S.nbytes
    g.tau_bytes = 0 if tau is None else tau.nbytes
    g.cand_bytes = 0 if cand is None else cand.nbytes
    g.cnt_bytes = 0 if cnt is None else cnt.nbytes
    g.status_bytes = 0 if status is None else status.nbytes
    g.a_stride, g.n_rows, g.a_scale_rows, g.row_bytes = row_bytes, n_rows, a_scale_rows, row_bytes
    g.n_rt, g.n_qt, g.s_ld, g.s_compact, g.cap = n_rt, n_qt, s_ld, s_compact, cap
    g.tail_off = (B.shape[0] if tail else -1)
    g.n_q, g.top_layout, g.s_tiles, g.s_vals = n_q, top_layout, s_tiles, s_vals
    _check(lib().kc_gemm(ctypes.c_int(kind), ctypes.byref(g)), f"gemm kind {kind}")


def select_tau(S, n_s, nq, qflags, ks, want_smax=True, cnt_fill=0xFFFFFFFF):
    """launch_select_tau as sample_pass calls it (S None: its n_s = 0 call).  cnt and status start
    0xFF-filled.  Returns (tau, cnt, status, smax)."""
    qpad = len(qflags)
    tau = np.full(qpad, np.nan, np.float32)
    cnt = np.full(cnt_words(qpad), cnt_fill, np.uint32)
    status = np.full(consts().st_words, 0xFFFFFFFF, np.uint32)
    smax = np.full((qpad, ks), 0x1234, np.uint64) if want_smax else None
    s_ld = 0 if S is None else S.shape[1]
    _check(lib().kc_select_tau(_p(S), ctypes.c_uint32(s_ld), ctypes.c_uint32(n_s), ctypes.c_uint32(nq),
                               ctypes.c_uint32(qpad), _p(_own(qflags, np.uint32)), ctypes.c_uint32(ks), _p(tau), _p(cnt),
                               ctypes.c_uint64(len(cnt)), _p(status), _p(smax)), "select_tau")
    return tau, cnt, status, smax


def global_tau(g, nq, qflags):
    P, qpad, ks = g.shape
    tau = np.full(qpad, np.nan, np.float32)
    _check(lib().kc_global_tau(_p(_own(g, np.uint64)), ctypes.c_uint32(P), ctypes.c_uint32(qpad), ctypes.c_uint32(nq),
                               ctypes.c_uint32(ks), _p(_own(qflags, np.uint32)), _p(tau)), "global_tau")
    return tau


def select_cand(cand, cnt, nq, tau, kp):
    nq_buf, cap = cand.shape
    rows = np.full((nq, kp), 0xFFFFFFFF, np.uint32)
    ncand = np.full(nq, 0xFFFFFFFF, np.uint32)
    tau_excl = np.full(nq, np.nan, np.float32)
    _check(lib().kc_select_cand(_p(_own(cand, np.uint64)), _p(_own(cnt, np.uint32)), ctypes.c_uint32(cap),
                                ctypes.c_uint32(nq), ctypes.c_uint32(nq_buf), _p(_own(tau, np.float32)),
                                ctypes.c_uint32(kp), _p(rows), _p(ncand), _p(tau_excl)), "select_cand")
    return rows, ncand, tau_excl


# ----------------------------------------------------------------------------------------
# Models: keys (csrc/bsr_device.hpp)
# ----------------------------------------------------------------------------------------
def ord_f32(s):
    """Monotone u32 image of an f32: a < b (as floats, -0.0 below +0.0) iff ord(a) < ord(b):
    negative values have every bit flipped, the others only the sign bit."""
    u = np.asarray(s, np.float32).view(np.uint32)
    neg = (u.view(np.int32) >> 31).view(np.uint32)  # all ones where the sign bit is set
    return u ^ (neg | np.uint32(0x80000000))


def unord_f32(o):
    o = np.asarray(o, np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(np.float32)


def score_key(s, row):
    """Larger score first, then smaller row: plain u64 order."""
    hi = (~ord_f32(s)).astype(np.uint64)
    return (hi << np.uint64(32)) | np.asarray(row, np.uint64)


def score_key_score(k):
    k = np.asarray(k, np.uint64)
    return unord_f32(~((k >> np.uint64(32)).astype(np.uint32)))


def key_row(k):
    return (np.asarray(k, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def kth_largest(S, ks):
    """The ks-th largest value of each row of S in key order (ties counted, +0.0 above -0.0),
    and the ks smallest keys score_key(S[q][i], i) ascending."""
    S = np.atleast_2d(np.asarray(S, np.float32))
    keys = score_key(S, np.arange(S.shape[1], dtype=np.uint64)[None, :])
    best = np.sort(keys, axis=1)[:, :ks]
    return score_key_score(best[:, ks - 1]), best


# ----------------------------------------------------------------------------------------
# Models: scores
# ----------------------------------------------------------------------------------------
def idot(A, B, chunk=8192):
    """Exact integer dot products of int8 rows, [len(A)][len(B)] int64: a float64 matmul of the
    operands (|I| <= 127^2 * K, far below 2^53).  Rows of up to 1040 bytes take an f32 matmul
    instead, which is exact as well: every partial sum, in any order, is an integer of magnitude
    <= 127^2 * K < 2^24 (half the conversions and memory traffic for the 2M-row shapes)."""
    ft = np.float32 if 127 * 127 * A.shape[1] < (1 << 24) else np.float64
    Bt = np.ascontiguousarray(B.astype(ft).T)
    out = np.empty((A.shape[0], B.shape[0]), np.int64)
    for i in range(0, A.shape[0], chunk):
        out[i:i + chunk] = np.rint(A[i:i + chunk].astype(ft) @ Bt).astype(np.int64)
    return out


def score(I, s_rows, s_query):
    """((float)I * s_block) * s_query, two separately rounded f32 multiplies: [row][query]."""
    t = I.astype(np.float32) * np.asarray(s_rows, np.float32)[:, None]
    return t * np.asarray(s_query, np.float32)[None, :]


def row_scales(block_scales, rows_per_scale, n):
    return np.repeat(np.asarray(block_scales, np.float32), rows_per_scale)[:n]


# ----------------------------------------------------------------------------------------
# Models: quantisation (the comment above k_rows_to_i8, in float64 -- or any wider float type)
# ----------------------------------------------------------------------------------------
def f32_round_up(x):
    """The smallest f32 >= x (x >= 0, finite)."""
    x = np.asarray(x)
    f = x.astype(np.float32)
    return np.where(f.astype(x.dtype) < x, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def unit_rows(a, ft=np.float64):
    """x = a / |a| per row (zero, or overflowing, rows: x = 0)."""
    a = np.asarray(a).astype(ft)
    ss = np.sum(a * a, axis=1)
    ok = (ss > 0) & (ss < ft(1e300))
    norm = np.sqrt(np.where(ok, ss, ft(1)))
    return np.where(ok[:, None], a / norm[:, None], ft(0))


def quant_scales(x, group):
    """One scale per `group` rows: the smallest f32 >= max |x_i| / 127 (1.0 for an all-zero
    group).  Returns (scales f32, the exact ratios max|x| / 127)."""
    n = x.shape[0]
    mx = np.abs(x).max(axis=1) if x.shape[1] else np.zeros(n, x.dtype)
    ng = (n + group - 1) // group
    g = np.zeros(ng * group, x.dtype)
    g[:n] = mx
    ratio = g.reshape(ng, group).max(axis=1) / x.dtype.type(127)
    return np.where(ratio > 0, f32_round_up(ratio), np.float32(1.0)).astype(np.float32), ratio


def quant_q(x, s_rows):
    """q = rint(x / s) clamped to +-127, and t = x / s."""
    t = x / np.asarray(s_rows).astype(x.dtype)[:, None]
    return np.clip(np.rint(t), -127, 127).astype(np.int8), t


def quant_err(x, s_rows, q):
    """e_row = || x - s q ||_2."""
    d = x - np.asarray(s_rows).astype(x.dtype)[:, None] * q.astype(x.dtype)
    return np.sqrt(np.sum(d * d, axis=1))


def quantize(a, group, ft=np.float64):
    """The whole model: (q int8 [n][dim], scales f32 [ceil(n / group)], e_row [n])."""
    x = unit_rows(a, ft)
    sc, _ = quant_scales(x, group)
    s_rows = np.repeat(sc, group)[:x.shape[0]]
    q, _ = quant_q(x, s_rows)
    return q, sc, quant_err(x, s_rows, q)


def compare_quant(a, group, q_gpu, sc_gpu):
    """The kernel's operand against the model.  Scales first: a scale may be the adjacent f32 only
    where the model's max|x| / 127 lies within a relative 1e-12 of an f32 value.  Then the
    elements, quantised by the model with the GPU's scales: an element may differ by +-1 only where
    the model's x / s lies within 1e-9 of a half-integer.  Returns the number of excused elements
    plus scales; anything else raises."""
    x = unit_rows(a)
    n = x.shape[0]
    sc, ratio = quant_scales(x, group)
    sc_gpu = np.asarray(sc_gpu, np.float32)
    assert sc_gpu.shape == sc.shape, (sc_gpu.shape, sc.shape)
    excused = 0
    for g in np.flatnonzero(sc_gpu.view(np.uint32) != sc.view(np.uint32)):
        adjacent = sc_gpu[g] in (np.nextafter(sc[g], np.float32(0)), np.nextafter(sc[g], np.float32(np.inf)))
        near = min(abs(float(sc[g]) - ratio[g]), abs(float(sc_gpu[g]) - ratio[g])) <= 1e-12 * ratio[g]
        assert adjacent and near, f"scale group {g}: gpu {sc_gpu[g]!r} model {sc[g]!r} ratio {ratio[g]!r}"
        excused += 1
    s_rows = np.repeat(sc_gpu, group)[:n]
    q, t = quant_q(x, s_rows)
    bad = np.argwhere(q != q_gpu)
    for r, c in bad:
        tie = abs(abs(t[r, c] - np.floor(t[r, c])) - 0.5) <= 1e-9
        assert tie and abs(int(q[r, c]) - int(q_gpu[r, c])) == 1, \
            f"operand[{r}][{c}]: gpu {q_gpu[r, c]} model {q[r, c]} x/s {t[r, c]!r}"
        excused += 1
    return excused


def seq_norm_f32(q):
    """|b| as src/metrics.rs:155: the sequential f32 sum of squares from -0.0 in index order, then
    a correctly rounded sqrt; a loop over the columns, vectorised over the queries."""
    q = np.asarray(q, np.float32)
    acc = np.full(q.shape[0], -0.0, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(q.shape[1]):
            acc = acc + q[:, c] * q[:, c]
        return np.sqrt(acc)


def query_flags(q, nb):
    """(qflags of the real queries) from the f32 rows and their magnitudes."""
    bad = ~np.isfinite(q).all(axis=1)
    with np.errstate(invalid="ignore"):
        ok = ~bad & np.isfinite(nb) & (nb >= np.float32(1e-18)) & (nb <= np.float32(1e18))
    return (np.where(bad, Q_NONFINITE, 0) | np.where(ok, 0, Q_NOAPPROX)).astype(np.uint32)


def ebound_model(ea, eb):
    """E_q = ea + eb + ea eb + 1.5e-4 in float64."""
    ea = float(ea)
    return ea + eb + ea * eb + 1.5e-4


def cos64(rows, queries):
    """float64 cosine of the original f32 vectors, [row][query]; 0 for a zero vector."""
    a, b = unit_rows(rows), unit_rows(queries)
    return a @ b.T


# ----------------------------------------------------------------------------------------
# Models: emission and selection
# ----------------------------------------------------------------------------------------
def emit_keys(Sq, tau, rows=None):
    """The keys of one query's passing rows: v >= tau (ties included), ascending.  Sq: the model's
    scores of rows 0 .. len(Sq) (or of `rows`)."""
    idx = np.flatnonzero(Sq >= np.float32(tau))
    r = idx if rows is None else np.asarray(rows)[idx]
    return np.sort(score_key(Sq[idx], r.astype(np.uint64)))


def sample_tile_rows(n, s_tiles):
    """Boolean mask of the rows of the sample tiles 32 L + 31 (128 rows each)."""
    c = consts()
    m = np.zeros(n, bool)
    for L in range(s_tiles):
        r0 = (L * c.sample_tile_every + c.sample_tile_phase) * 128
        m[r0:r0 + 128] = True
    return m


def top_workgroup_rows(n, W):
    """k_filter_skinny2 / k_filter_skinny_glds, TOP with top_layout = 2: workgroup b takes the
    16-row units u = b (mod W); unit u holds A-rows m = 0 .. 15 = corpus rows
    (m >> 1) * 2 n_units + 2 u + (m & 1).  Returns wg[row] for every row < n."""
    n_units = (n + 15) // 16
    u = np.arange(n_units, dtype=np.int64)[:, None]
    m = np.arange(16, dtype=np.int64)[None, :]
    rows = (m >> 1) * (2 * n_units) + 2 * u + (m & 1)
    wg = np.full(n, -1, np.int64)
    ok = rows < n
    wg[rows[ok]] = np.broadcast_to(u % W, rows.shape)[ok]
    assert (wg >= 0).all()
    return wg


# ----------------------------------------------------------------------------------------
# Data sets (fixed seeds; tests/test_kernel_models.py checks that none of the committed cases
# sits on a rounding tie, by running the model in np.longdouble as well)
# ----------------------------------------------------------------------------------------
def data_uniform(rng, n, dim):
    """(a) U(-1, 1)."""
    return rng.uniform(-1, 1, (n, dim)).astype(np.float32)


def data_outlier(rng, n, dim):
    """(b) U(-1, 1) with one component of 60.0 in about 0.5% of the rows (at least one): blocks
    with a large scale."""
    a = data_uniform(rng, n, dim)
    for r in rng.choice(n, max(1, n // 200), replace=False):
        a[r, rng.integers(dim)] = 60.0
    return a


def data_positive(rng, n, dim):
    """(c) all-positive vectors; the queries of this set are their negation, so every score and
    every threshold is negative."""
    return rng.uniform(0.05, 1, (n, dim)).astype(np.float32)


def worst_row(rng, dim):
    """A row built to have the largest e_row of its corpus: one component of 127 sets its block's
    scale (its normalised maximum exceeds a uniform row's), every other component lies at
    (k + 0.49) scale steps, k <= 60, i.e. as far from an int8 value as a rounding allows without
    sitting on the tie."""
    a = (rng.integers(0, 61, dim) + 0.49) * rng.choice([-1.0, 1.0], dim)
    a[rng.integers(dim)] = 127.0
    return (a * 0.01).astype(np.float32)


PREP_DIMS = (40, 130, 768, 1024, 1100)
PREP_NS = (1, 31, 33, 257, 4097)
PREP_SAMPLE_NS = PREP_NS + (128 * 32 + 1, 129 * 32)  # k_rows_to_i8_sample: one and two scale groups
PREP_KIND_CASES = ((130, 1000), (768, 1000))         # (dim, n) of the data (b) and (c) corpora
QUERY_DIMS = (40, 768, 1100, 8256)
QUERY_BATCHES = ((3, 0), (3, 1), (300, 0))           # (nq, variant), see special_queries
QUERY_KIND_DIMS = (130, 768)                         # data (b) and (c) batches of 40 queries


def plant_positions(n):
    """Where the worst row is planted in turn: row 0, row n - 1 (a partial block unless n % 32 ==
    0) and, from 96 rows, local rows 0, 8, 16, 24, 31 of a middle block (one per wave of
    k_rows_to_i8's workgroup, and the last)."""
    pos = [0] if n == 1 else [0, n - 1]
    if n >= 96:
        b0 = 32 * ((n // 32) // 2)
        pos += [b0 + i for i in (0, 8, 16, 24, 31)]
    return pos


def prep_rows(n, dim, plant, kind="a"):
    """The corpus of a row-preparation case: data set `kind`, a zero row, a row whose sum of squares
    is 1e-36 and one with 1e36 (from 13 rows), and the worst row at `plant` (None: no plant)."""
    rng = np.random.default_rng(1000003 * dim + 101 * n + (0 if plant is None else 7 + plant))
    a = {"a": data_uniform, "b": data_outlier, "c": data_positive}[kind](rng, n, dim)
    if n > 12:
        for r, norm in ((1, 0.0), (5, 1e-18), (9, 1e18)):
            if r != plant:
                u = a[r].astype(np.float64)
                a[r] = (u * (norm / np.sqrt(np.sum(u * u)))).astype(np.float32)
    if plant is not None:
        a[plant] = worst_row(rng, dim)
    return a


def prep_queries(nq, dim, kind="a", variant=0):
    """A query batch with a zero query, a 1e-25 query, a 1e19 query and a NaN query (see
    special_queries), the others from data set `kind`."""
    rng = np.random.default_rng(77003 * dim + 13 * nq + variant)
    q = {"a": data_uniform, "b": data_outlier, "c": lambda *a: -data_positive(*a)}[kind](rng, nq, dim)
    for name, r in special_queries(nq, variant).items():
        if name == "zero":
            q[r] = 0.0
        elif name == "tiny":
            q[r] *= np.float32(1e-25)
        elif name == "huge":
            q[r] *= np.float32(1e19)
        else:
            q[r, dim // 2] = np.nan
    return q


def special_queries(nq, variant=0):
    """Rows of the special queries.  A batch of fewer than 8 queries cannot hold all four beside an
    ordinary query: variant 0 has the zero and NaN queries, variant 1 the 1e-25 and 1e19 queries."""
    if nq >= 8:
        return {"zero": 1, "tiny": 2, "huge": nq - 2, "nan": nq - 1}
    return {"zero": 0, "nan": nq - 1} if variant == 0 else {"tiny": 0, "huge": 1}


def synth_operand(rng, n, row_bytes, group, n_pad=None):
    """(d) a synthetic int8 operand fed to the filters directly: random rows, rows of all +127 and
    all -127, runs of 400 identical rows, zero rows; arbitrary positive scales spanning 1e-4 ..
    1e-1, one per `group` rows.  Rows n .. n_pad are zero with scale 1.0 (what the load leaves)."""
    n_pad = n_pad or n
    A = np.zeros((n_pad, row_bytes), np.int8)
    A[:n] = rng.integers(-127, 128, (n, row_bytes), dtype=np.int8)
    if n >= 4:
        A[n // 2] = 127
        A[n // 2 + 1] = -127
        A[n // 3] = 0
        A[n - 1] = 0
    for start in ((n // 5, 2 * n // 3) if n >= 3000 else (n // 5,) if n >= 1000 else ()):
        A[start:start + 400] = A[start]
    sc = np.ones((n_pad + group - 1) // group, np.float32)
    nv = (n + group - 1) // group
    sc[:nv] = np.exp(rng.uniform(np.log(1e-4), np.log(1e-1), nv)).astype(np.float32)
    return A, sc


def synth_queries(rng, nq, qpad, row_bytes):
    """(d) the query side: random int8 rows, one of all +127 and one of all -127, scales spanning
    1e-4 .. 1e-1; padding queries (>= nq) zero with scale 0, as k_query_prep leaves them."""
    B = np.zeros((qpad, row_bytes), np.int8)
    B[:nq] = rng.integers(-127, 128, (nq, row_bytes), dtype=np.int8)
    B[0] = 127
    if nq > 1:
        B[nq - 1] = -127
    sc = np.zeros(qpad, np.float32)
    sc[:nq] = np.exp(rng.uniform(np.log(1e-4), np.log(1e-1), nq)).astype(np.float32)
    return B, sc


# ----------------------------------------------------------------------------------------
# The mask bitsets (csrc/k_prep.hip: one kernel family for lists, counts and the cut)
# ----------------------------------------------------------------------------------------
MASK_BLOCK_WORDS = 256  # kMaskBlockWords (the GPU tests check it against the library's)
LIST_DESC = np.dtype([("off", "<u8"), ("mask", "<u4"), ("n_list", "<u4")])  # MaskListDesc


def mask_words(n):
    return (n + 63) // 64


def mask_blocks(n):
    return max(1, (mask_words(n) + MASK_BLOCK_WORDS - 1) // MASK_BLOCK_WORDS)


def pack_bits(bits):
    """bool [n] -> u64 words, bit (i & 63) of word (i >> 6) = bits[i]; the tail bits zero."""
    n = len(bits)
    b = np.zeros(mask_words(n) * 64, np.uint8)
    b[:n] = bits
    return np.packbits(b, bitorder="little").view(np.uint64).copy()


def mask_rows(allow, dead, n):
    """The model of the one bitset reader: bool [n], row i allowed (allow None: every row) and not
    deleted (dead None: none).  Bits at positions >= n are ignored."""
    def unpack(w):
        return np.unpackbits(np.ascontiguousarray(w).view(np.uint8), bitorder="little")[:n].astype(bool)
    rows = np.ones(n, bool) if allow is None else unpack(allow)
    return rows if dead is None else rows & ~unpack(dead)


def mask_list_model(allow, dead, n):
    """(blk [mask_blocks(n) + 1]: the exclusive prefix sums of the per-block counts, then A; the A ids
    ascending)."""
    ids = np.flatnonzero(mask_rows(allow, dead, n)).astype(np.uint32)
    per = np.bincount(ids // (64 * MASK_BLOCK_WORDS), minlength=mask_blocks(n))
    return np.concatenate(([0], np.cumsum(per))).astype(np.uint32), ids


def mask_cut_model(keys, allow, dead, n):
    """The keys of one list that survive the cut, in their order: not KEY_NONE, row < n, allowed, live."""
    keys = np.asarray(keys, np.uint64)
    rows = key_row(keys).astype(np.int64)
    ok = mask_rows(allow, dead, n)
    keep = (keys != KEY_NONE) & (rows < n)
    keep[keep] = ok[rows[keep]]
    return keys[keep]


def _mask_lib():
    L = lib()
    L.kc_mask_block_words.restype = ctypes.c_uint32
    L.kc_mask_blocks.restype = ctypes.c_uint32
    L.kc_mask_blocks.argtypes = [ctypes.c_uint64]
    return L


def mask_count(allow, dead, n, n_masks=1, query_mask=None, grouped=False):
    """launch_mask_list_count (grouped False) / launch_mask_groups_count.  Returns (blk
    [n_masks][mask_blocks(n) + 1], out [n_masks + 1] or None); both start 0xFF-filled."""
    L = _mask_lib()
    words = mask_words(n)
    assert allow is None or allow.size == n_masks * words
    assert dead is None or dead.size == words
    blk = np.full((n_masks, mask_blocks(n) + 1), 0xFFFFFFFF, np.uint32)
    out = np.full(n_masks + 1, 0xFFFFFFFF, np.uint32) if grouped else None
    nq = 0 if query_mask is None else len(query_mask)
    _check(L.kc_mask_count(_p(_own(allow, np.uint64)), ctypes.c_uint64(words), ctypes.c_uint32(n_masks),
                           ctypes.c_uint64(n), _p(_own(dead, np.uint64)), _p(_own(query_mask, np.uint32)),
                           ctypes.c_uint32(nq), _p(blk), _p(out), ctypes.c_int(1 if grouped else 0)), "mask_count")
    return blk, out


def mask_scatter(allow, dead, n, blk, list_buf, n_list=0, descs=None):
    """launch_mask_list_scatter (descs None: the first n_list ids at list_buf[0 ..]) /
    launch_mask_groups_scatter over descs (LIST_DESC).  list_buf is written in place."""
    L = _mask_lib()
    n_masks = blk.shape[0]
    n_lists = 0 if descs is None else len(descs)
    if descs is not None:
        assert descs.dtype == LIST_DESC and all(int(d["off"]) + int(d["n_list"]) <= len(list_buf) for d in descs)
    else:
        assert n_list <= len(list_buf)
    _check(L.kc_mask_scatter(_p(_own(allow, np.uint64)), ctypes.c_uint64(mask_words(n)), ctypes.c_uint32(n_masks),
                             ctypes.c_uint64(n), _p(_own(dead, np.uint64)), _p(_own(blk, np.uint32)), _p(descs),
                             ctypes.c_uint32(n_lists), ctypes.c_uint32(n_list), _p(_own(list_buf, np.uint32)),
                             ctypes.c_uint64(len(list_buf)), ctypes.c_int(0 if descs is None else 1)), "mask_scatter")


def mask_cut(cand, cnt, nq, allow, n, n_masks=1, query_mask=None, dead=None):
    """launch_mask_cut: cand [nq_buf][cap] and cnt [nq_buf] are written in place.  Returns (raw
    [nq_buf], items), both 0xFF-filled before the launch."""
    L = _mask_lib()
    nq_buf, cap = cand.shape
    assert len(cnt) == nq_buf and nq <= nq_buf and allow.size == n_masks * mask_words(n)
    assert query_mask is None or (len(query_mask) == nq and int(query_mask.max()) < n_masks)
    raw = np.full(nq_buf, 0xFFFFFFFF, np.uint32)
    items = np.full(1, 0xFFFFFFFF, np.uint32)
    _check(L.kc_mask_cut(_p(_own(cand, np.uint64)), _p(_own(cnt, np.uint32)), ctypes.c_uint32(cap), ctypes.c_uint32(nq),
                         ctypes.c_uint32(nq_buf), _p(_own(allow, np.uint64)), ctypes.c_uint64(mask_words(n)),
                         ctypes.c_uint32(n_masks), _p(_own(query_mask, np.uint32)), _p(_own(dead, np.uint64)),
                         ctypes.c_uint64(n), _p(raw), _p(items)), "mask_cut")
    return raw, int(items[0])


# The cases of tests/test_gpu_kernels_mask.py (the CPU test of the models walks the small ones).
MASK_NS = (1, 63, 64, 65, 16384, 16385, 2 * 16384 + 100, 257 * 16384 + 5)
MASK_KINDS = ("empty", "full", "half", "last", "garbage", "none")
DEAD_KINDS = ("none", "random", "superset")


def mask_case(n, kind, seed=0):
    """An allow mask of `kind` over n rows (u64 words, or None for kind "none").  "garbage": a random
    mask whose last word is filled at the positions >= n, which every reader must ignore."""
    rng = np.random.default_rng(1000 + 7 * seed + n % 9973)
    if kind == "none":
        return None
    if kind == "empty":
        return pack_bits(np.zeros(n, bool))
    if kind == "full":
        return pack_bits(np.ones(n, bool))
    if kind == "last":
        bits = np.zeros(n, bool)
        bits[n - 1] = True
        return pack_bits(bits)
    w = pack_bits(rng.random(n) < 0.5)
    if kind == "garbage" and n % 64:
        w[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)
    return w


def dead_case(n, kind, allow, seed=0):
    """A bitset of deleted rows (None: no tombstones).  "superset": every allowed row and a random
    half of the others (allow None: every row), so that no row is left.  No bit at a position >= n."""
    rng = np.random.default_rng(2000 + 7 * seed + n % 9973)
    if kind == "none":
        return None
    bits = rng.random(n) < 0.5
    if kind == "superset":
        bits |= mask_rows(allow, None, n)
    return pack_bits(bits)
