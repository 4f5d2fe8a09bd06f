"""Kernel-level checks of the exact stage: the ctypes loader of the test-only shim
(tests/kcheck/kcheck_exact.cpp -> lib/libbsr_kcheck_exact.so) and exact models of the contracts of
csrc/k_exact.hip: the reference's f32 distance, the keys, the candidate selections, the
certification and the exclusion bound, the root merge's certification.

None of the models needs a tolerance: every quantity is an f32 operation in a fixed order, a float64
expression without a product, a bit manipulation or an order statistic.

tests/test_exact_models.py pins the models with hand-derived cases (CPU);
tests/test_gpu_kernels_{rescore,scan,merge_cert}.py compare the kernels with them.
"""
import ctypes
import os

import numpy as np

from kcheck import (KEY_NONE, _check, key_row, ld_for, round_up, score_key,  # noqa: F401
                    score_key_score, seq_norm_f32)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "better-search-rag-rust_amd", "lib", "libbsr_kcheck_exact.so")

NEG_INF, POS_INF = np.float32(-np.inf), np.float32(np.inf)
IDX_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
# the environment switches launch_rescore / launch_merge read: the tests assert they are unset
SWITCHES = ("BSR_RESCORE_KP", "BSR_GT_FLAT", "BSR_SOLO_PUB", "BSR_MERGE_HASH")


def assert_no_switches():
    for name in SWITCHES:
        assert os.environ.get(name) is None, f"{name} is set: the launchers' dispatch is not the product's"


# ----------------------------------------------------------------------------------------
# Loader
# ----------------------------------------------------------------------------------------
class _Consts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "scan_qf", "rescore_all_grid", "ticket_words", "top_keys_per_lane", "merge_max_entries", "fused_select_cap",
        "st_words", "st_fail", "st_emitted", "st_query_flags", "st_fail2",
        "row_non_finite", "row_norm_ovf", "row_norm_range", "query_no_approx")]


def _struct(spec):
    """A ctypes structure from (name, kind): 'buf' = pointer + <name>_bytes, 'ptr', 'u32', 'u64'."""
    fields = []
    for name, kind in spec:
        if kind == "buf":
            fields += [(name, ctypes.c_void_p), (name + "_bytes", ctypes.c_uint64)]
        else:
            fields.append((name, {"ptr": ctypes.c_void_p, "u32": ctypes.c_uint32, "u64": ctypes.c_uint64}[kind]))
    return type("S", (ctypes.Structure,), {"_fields_": fields})


# (the order of struct KcRescore / KcScan / KcMerge in kcheck_exact.cpp)
_RESCORE_SPEC = (
    ("rows", "buf"), ("ld", "u32"), ("dim", "u32"), ("na", "buf"), ("qf32", "buf"), ("nb", "buf"),
    ("n_items", "u32"), ("kp", "u32"), ("n_items_dev", "ptr"), ("qlist", "buf"), ("cand_rows", "buf"),
    ("ncand", "buf"), ("tau_excl", "buf"), ("cand_keys", "buf"), ("cnt", "buf"), ("tau0", "buf"),
    ("cap", "u32"), ("sel", "u32"), ("top_w", "u32"), ("k", "u32"),
    ("qflags", "buf"), ("top_tau", "buf"), ("top_cnt", "buf"), ("ebound", "buf"), ("out_keys", "buf"),
    ("fail_cnt", "buf"), ("fail_list", "buf"), ("res_idx", "buf"), ("res_dist", "buf"), ("res_cnt", "buf"),
    ("offset", "u64"), ("n_rows", "u64"), ("dead", "buf"),
    ("hres_idx", "buf"), ("hres_dist", "buf"), ("hres_cnt", "buf"),
    ("next_status", "buf"), ("emit_cnt", "buf"), ("cur_status", "buf"), ("n_queries", "u32"), ("pub_alias", "u32"),
    ("excl_out", "buf"), ("merge_words", "buf"), ("pub_src", "buf"), ("pub_dst", "ptr"), ("pub_bytes", "u64"),
    ("pub_flag", "ptr"), ("pub_ticket", "ptr"))
_SCAN_SPEC = (
    ("rows", "buf"), ("ld", "u32"), ("dim", "u32"), ("n", "u64"), ("na", "buf"), ("qf32", "buf"), ("qids", "buf"),
    ("nb", "buf"), ("list", "buf"), ("grp", "buf"),
    ("n_list", "u32"), ("nqf", "u32"), ("groups", "u32"), ("k", "u32"), ("grid", "u32"), ("part", "buf"))
_MERGE_SPEC = (
    ("idx", "buf"), ("dist", "buf"), ("cnt", "buf"), ("idx_stride", "u64"), ("dist_stride", "u64"),
    ("cnt_stride", "u64"), ("P", "u32"), ("nq", "u32"), ("k_in", "u32"), ("k", "u32"),
    ("out_idx", "buf"), ("out_dist", "buf"), ("out_count", "buf"), ("first_nan", "ptr"),
    ("excl", "buf"), ("excl_stride", "u64"), ("need", "u32"), ("lists_unique", "u32"), ("fail_cnt", "ptr"),
    ("fail_list", "buf"), ("st", "buf"), ("st_stride", "u64"), ("st_all", "buf"))
_Rescore, _Scan, _Merge = _struct(_RESCORE_SPEC), _struct(_SCAN_SPEC), _struct(_MERGE_SPEC)

# struct ScanGroupDesc { uint64_t off; uint32_t n_list, nq; }
GROUP_DESC = np.dtype([("off", np.uint64), ("n_list", np.uint32), ("nq", np.uint32)])

_lib = None
_consts = None


def lib() -> ctypes.CDLL:
    """libbsr_kcheck_exact.so (raises if it has not been built).  Load it after the `gpu` fixture."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built (run __graft_entry__.build())")
        _lib = ctypes.CDLL(LIB_PATH)
        for f in ("kc_kp_for", "kc_cap_for", "kc_ks_for"):
            getattr(_lib, f).restype = ctypes.c_uint32
            getattr(_lib, f).argtypes = [ctypes.c_uint32]
        _lib.kc_scan_grid_for.restype = ctypes.c_uint32
        _lib.kc_scan_grid_for.argtypes = [ctypes.c_uint64]
        sizes = (ctypes.c_uint32 * 3)()
        _lib.kc_exact_sizes(sizes)
        assert list(sizes) == [ctypes.sizeof(t) for t in (_Rescore, _Scan, _Merge)], "struct layouts differ from the shim's"
    return _lib


def consts() -> _Consts:
    global _consts
    if _consts is None:
        _consts = _Consts()
        lib().kc_exact_consts(ctypes.byref(_consts))
    return _consts


def kp_for(k):
    return lib().kc_kp_for(k)


def cap_for(k):
    return lib().kc_cap_for(k)


def ks_for(k):
    return lib().kc_ks_for(k)


def scan_grid_for(n):
    return lib().kc_scan_grid_for(n)


def _rc(rc):
    """A launcher's refusal (hipErrorInvalidValue) is a result; any other error is a GPU fault or a
    broken set-up (an allocation or copy of the shim that failed), after which nothing more is
    launched: the session ends, and the tests after this one have NOT run."""
    if rc not in (0, 1):
        import pytest
        pytest.exit(f"hipError_t {rc} from the exact-stage shim -- a kernel fault, or a set-up error of the shim "
                    f"itself such as a failed hipMalloc (2 = out of memory): the session stops here so that no "
                    f"further GPU work starts; the remaining tests were not run", returncode=3)
    return rc


def _fill(s, spec, kw):
    """The structure's fields from keyword arguments: numpy arrays for pointers (None: null), ints
    for scalars.  Returns the arrays kept alive."""
    kw = dict(kw)
    keep = []
    for name, kind in spec:
        v = kw.pop(name, None)
        if kind in ("buf", "ptr"):
            if v is not None:
                assert isinstance(v, np.ndarray) and v.flags.c_contiguous, name
                keep.append(v)
                setattr(s, name, v.ctypes.data)
                if kind == "buf":
                    setattr(s, name + "_bytes", v.nbytes)
        else:
            setattr(s, name, int(v or 0))
    assert not kw, f"unknown arguments {sorted(kw)}"
    return keep


def rescore_raw(**kw):
    """launch_rescore through kc_rescore; returns the hipError_t (0 = success)."""
    s = _Rescore()
    keep = _fill(s, _RESCORE_SPEC, kw)
    rc = lib().kc_rescore(ctypes.byref(s))
    del keep
    return _rc(rc)


def scan_raw(kind, **kw):
    """kind 0: launch_scan_exact, 1: launch_scan_list, 2: launch_scan_list_groups."""
    s = _Scan()
    keep = _fill(s, _SCAN_SPEC, kw)
    rc = getattr(lib(), ("kc_scan_exact", "kc_scan_list", "kc_scan_list_groups")[kind])(ctypes.byref(s))
    del keep
    return _rc(rc)


def merge_raw(**kw):
    s = _Merge()
    keep = _fill(s, _MERGE_SPEC, kw)
    rc = lib().kc_merge(ctypes.byref(s))
    del keep
    return _rc(rc)


def _vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def merge_parts(part, grid, qids, nqf, k, out_keys):
    return _rc(lib().kc_merge_parts(_vp(part), ctypes.c_uint64(part.nbytes), ctypes.c_uint32(grid), _vp(qids),
                                    ctypes.c_uint64(qids.nbytes), ctypes.c_uint32(nqf), ctypes.c_uint32(k),
                                    _vp(out_keys), ctypes.c_uint64(out_keys.nbytes)))


def merge_parts_groups(part, grid, qids, qf, grp, k, out_keys):
    return _rc(lib().kc_merge_parts_groups(_vp(part), ctypes.c_uint64(part.nbytes), ctypes.c_uint32(grid), _vp(qids),
                                           ctypes.c_uint64(qids.nbytes), ctypes.c_uint32(qf), _vp(grp),
                                           ctypes.c_uint32(len(grp)), ctypes.c_uint32(k), _vp(out_keys),
                                           ctypes.c_uint64(out_keys.nbytes)))


def finalize(keys, n, offset, emit_cnt=None, n_q=None, fill=0x5A5A5A5A):
    """launch_finalize: returns (idx, dist, count, status, cur_status); status words start as `fill`."""
    nq, k = keys.shape
    idx = np.full((nq, k), 0x1234, np.uint64)
    dist = np.full((nq, k), np.nan, np.float32)
    cnt = np.full(nq, fill, np.uint32)
    st = np.full(consts().st_words, fill, np.uint32)
    cur = np.full(consts().st_words, fill, np.uint32)
    _check(_rc(lib().kc_finalize(_vp(keys), ctypes.c_uint32(nq), ctypes.c_uint32(k), ctypes.c_uint64(n),
                             ctypes.c_uint64(offset), _vp(idx), _vp(dist), _vp(cnt), _vp(st), _vp(emit_cnt), _vp(cur),
                                 _vp(n_q))), "finalize")
    return idx, dist, cnt, st, cur


def row_norms(slab_rows, n, dim, flags_in=0):
    """launch_row_norms over the slab [n_pad][ld]: (na [n_pad], NaN-filled before; the flags word)."""
    n_pad, ld = slab_rows.shape
    na = np.full(n_pad, np.nan, np.float32)
    flags = np.array([flags_in], np.uint32)
    _check(_rc(lib().kc_row_norms(_vp(slab_rows), ctypes.c_uint64(n), ctypes.c_uint64(n_pad), ctypes.c_uint32(dim),
                                  ctypes.c_uint32(ld), _vp(na), _vp(flags))), "row_norms")
    return na, int(flags[0])


# ----------------------------------------------------------------------------------------
# Models: the exact distance and its keys (csrc/bsr_device.hpp, src/metrics.rs:143-165)
# ----------------------------------------------------------------------------------------
def exact_distance(rows, q, na, nb):
    """seq_chunk + finish_distance for every row of `rows` [n][dim] against the query q [dim], with
    the magnitudes GIVEN (na [n], nb): the f32 dot product summed sequentially from -0.0 in index
    order (each product and each sum rounded), 0 when max |a_i - b_i| <= 1e-10, 1 for a zero
    magnitude, else 1 - clamp(dot / (na * nb)) with every operation in f32."""
    rows = np.asarray(rows, np.float32)
    q = np.asarray(q, np.float32).ravel()
    na = np.asarray(na, np.float32)
    nb = np.float32(nb)
    n, dim = rows.shape
    assert q.size == dim and na.shape == (n,)
    with np.errstate(all="ignore"):
        prods = np.empty((n, dim + 1), np.float32)
        prods[:, 0] = -0.0
        prods[:, 1:] = rows * q[None, :]
        dot = np.add.accumulate(prods, axis=1, dtype=np.float32)[:, -1]  # strictly sequential f32 sums
        mx = np.abs(rows - q[None, :]).max(axis=1) if dim else np.zeros(n, np.float32)
        denom = (na * nb).astype(np.float32)
        s = (dot / denom).astype(np.float32)
        s = np.fmin(np.fmax(s, np.float32(-1.0)), np.float32(1.0))
        d = (np.float32(1.0) - s).astype(np.float32)
    d = np.where((na == 0) | (nb == 0), np.float32(1.0), d)
    d = np.where(mx <= np.float32(1e-10), np.float32(0.0), d)
    return d.astype(np.float32)


def dist_key(d, row):
    """(bits(d) << 32) | row: distance ascending, then row ascending, in plain u64 order (d >= 0)."""
    hi = np.asarray(d, np.float32).view(np.uint32).astype(np.uint64)
    return (hi << np.uint64(32)) | np.asarray(row, np.uint64)


def key_dist(k):
    return (np.asarray(k, np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)


def topk_keys(keys, k):
    """The k smallest keys ascending (KEY_NONE is no key), padded with KEY_NONE."""
    keys = np.asarray(keys, np.uint64).ravel()
    keys = np.sort(keys[keys != KEY_NONE])[:k]
    out = np.full(k, KEY_NONE, np.uint64)
    out[:len(keys)] = keys
    return out


# ----------------------------------------------------------------------------------------
# Models: certification (certify / exclusion_bound of k_exact.hip)
# ----------------------------------------------------------------------------------------
def _third_bound(eb, nb):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(((np.float64(1.0) - np.float64(eb)) - np.float64(1e-4)) - np.float64(6e-9) / np.float64(nb))


def certify(tx, kth_key, ebound, nb):
    """Whether a list whose k-th key is kth_key is certified against tau_x = tx: float64 operations
    in the source's order on the f32 inputs."""
    tx, eb, nb = float(np.float32(tx)), float(np.float32(ebound)), float(np.float32(nb))
    if tx == -np.inf:
        return True
    if not (tx < np.inf) or np.uint64(kth_key) == KEY_NONE:
        return False
    dk = float(key_dist(np.uint64(kth_key)))
    return bool(eb < 1.0 and dk < ((1.0 - tx) - eb) - 2.5e-7 and tx < _third_bound(eb, nb))


def exclusion_bound(tx, ebound, nb):
    """The f32 bound a rank reports: ((1 - tx) - E) - 2.5e-7 rounded DOWN to f32; +inf for tx = -inf;
    -inf when nothing can be certified (tx = +inf or NaN, E >= 1 or NaN, the third condition)."""
    tx, eb, nb = float(np.float32(tx)), float(np.float32(ebound)), float(np.float32(nb))
    if tx == -np.inf:
        return POS_INF
    if not (tx < np.inf) or not (eb < 1.0) or not (tx < _third_bound(eb, nb)):
        return NEG_INF
    x = ((1.0 - tx) - eb) - 2.5e-7
    xf = np.float32(x)
    if float(xf) > x:
        xf = np.nextafter(xf, NEG_INF)
    return np.float32(xf)


def select_kp(keys, cnt, cap, kp, tau0):
    """Mode S's selection from an emitted list keys[0 .. cnt): (candidate rows, tau_x).  An overflowed
    list (cnt > cap): no candidates, +inf; cnt <= kp: every key, tau0; else the kp smallest keys (in
    slot order) and the score of the (kp+1)-th."""
    if cnt > cap:
        return np.zeros(0, np.uint32), POS_INF
    keys = np.asarray(keys, np.uint64)[:cnt]
    if cnt <= kp:
        return key_row(keys), np.float32(tau0)
    T = np.sort(keys)[kp]
    return key_row(keys[keys < T]), np.float32(score_key_score(T))


def top_select(lists, top_w, kp, served=True):
    """top_select() of k_exact.hip over a query's 4 * top_w slots (ascending 4-lists, KEY_NONE = no
    key).  Returns dict(rows, tx, top_tau, top_cnt, list): X = the smallest of the lists' 4th slots;
    top_tau = score(X) (-inf when no list has a 4th key, +inf for an unserved query); the keys < X in
    slot order go to the front of the list (top_cnt of them); the candidates are the kp smallest
    valid keys and tx = max(score of the (kp+1)-th, top_tau) (top_tau alone when there is no
    (kp+1)-th).  An unserved query has no candidates and tx = +inf."""
    lists = np.asarray(lists, np.uint64)
    U = 4 * top_w
    new = lists.copy()
    if not served:
        return dict(rows=np.zeros(0, np.uint32), tx=POS_INF, top_tau=POS_INF, top_cnt=0, list=new)
    x = lists[:U]
    X = x[3::4].min()
    top_tau = NEG_INF if X == KEY_NONE else np.float32(score_key_score(X))
    front = x[x < X]
    new[:len(front)] = front
    valid = x[x != KEY_NONE]
    if len(valid) > kp:
        T = np.sort(valid)[kp]
        rows, tx = key_row(valid[valid < T]), np.float32(score_key_score(T))
        tx = np.float32(max(tx, top_tau))
    else:
        rows, tx = key_row(valid), top_tau
    return dict(rows=rows, tx=tx, top_tau=top_tau, top_cnt=len(front), list=new)


def merge_certify(got, kth_dist, excl, need, k):
    """The root's certification of one merged list: got >= need entries; a full list (got == k) needs
    its k-th distance strictly below the smallest bound (float64; a NaN bound counts as -inf); a
    shorter one needs every bound +inf."""
    excl = np.asarray(excl, np.float32)
    xmin = float(np.min(np.where(np.isnan(excl), NEG_INF, excl))) if len(excl) else np.inf
    if got < need:
        return False
    if got == k:
        return bool(float(np.float32(kth_dist)) < xmin)
    return xmin == np.inf


# ----------------------------------------------------------------------------------------
# launch_rescore's dispatch, restated from its conditions (the switches unset)
# ----------------------------------------------------------------------------------------
def rescore_build(*, n_items, ld, k, kp, cap, sel=0, top_w=0, dev=False, pub=False, excl=False, keys=False,
                  hres=False, qlist=False):
    E = (k + 63) // 64
    if sel and not dev and not pub and not excl and n_items <= 16 and ld % 64 == 0 and ld <= 1024 and k <= 64 \
            and kp <= 64 and (cap <= 1024 or top_w):
        return "k_rescore_kp<1>/top" if top_w else "k_rescore_kp<1>"
    if excl and keys and not sel and not dev and not pub and not hres and not qlist and ld % 64 == 0 and ld <= 1024:
        return f"k_rescore_flat<{E},{12 if ld == 768 else 0}>"
    if dev:
        return f"k_rescore<{E},8,2>"
    mode = "excl" if excl else "sel" if sel else "B" if keys else "A"
    return f"k_rescore<{E},1,2,4>/{mode}"


# ----------------------------------------------------------------------------------------
# Data: a corpus with the rows kernels get wrong, and its queries
# ----------------------------------------------------------------------------------------
DIMS = (64, 130, 768, 1024, 1100)  # one chunk; a partial last chunk of 2; 12 chunks; the LDS limit; past it


class Corpus:
    """n rows of U(-1, 1) [n][dim] in a slab [round_up(n, 256)][ld] and nq queries [nq][ld].  Planted:
    rows identical to query 0 (distance 0 through the 1e-10 rule), one row differing from query 0 by
    2e-10 in one element (not identical), zero rows (distance 1), a run of 100 identical rows (ties
    broken by row id) and the negation of query 1 (distance 2).  na and nb are the MODEL's norms."""

    def __init__(self, n, dim, nq, seed):
        rng = np.random.default_rng(seed)
        self.n, self.dim, self.nq, self.ld = n, dim, nq, ld_for(dim)
        a = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
        q = rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
        # (query 0 with a first element small enough for 2e-10 to be representable next to it)
        q[0, 0] = np.float32(1e-9)
        self.ident = [3, n // 2, n - 1]
        for r in self.ident:
            a[r] = q[0]
        self.near = 7
        a[self.near] = q[0]
        a[self.near, 0] = np.float32(1e-9) + np.float32(2e-10)
        self.zero = [5, n - 2]
        for r in self.zero:
            a[r] = 0.0
        self.run = n // 3
        a[self.run:self.run + 100] = a[self.run]
        self.neg = 11
        if nq > 1:
            a[self.neg] = -q[1]
        self.a, self.q = a, q
        self.rows = np.zeros((round_up(n, 256), self.ld), np.float32)
        self.rows[:n, :dim] = a
        self.qf32 = np.zeros((nq, self.ld), np.float32)
        self.qf32[:, :dim] = q
        self.na = np.zeros(self.rows.shape[0], np.float32)
        self.na[:n] = seq_norm_f32(a)
        self.nb = seq_norm_f32(q)

    def dist(self, qi, rows=None, na=None, nb=None):
        """The model's distances of the given rows (default: all) to query qi; na (per row of the
        slab) and nb (a scalar) default to the model's norms."""
        rows = np.arange(self.n) if rows is None else np.asarray(rows, np.int64)
        na = self.na if na is None else na
        return exact_distance(self.a[rows], self.q[qi], na[rows], self.nb[qi] if nb is None else nb)

    def keys(self, qi, rows, na=None, nb=None):
        """The model's distance keys of the given rows for query qi."""
        rows = np.asarray(rows, np.int64)
        return dist_key(self.dist(qi, rows, na, nb), rows.astype(np.uint64))

    def special_rows(self):
        return self.ident + [self.near] + self.zero + [self.neg] + list(range(self.run, self.run + 100))


def f32_neighbours(x):
    """The four f32 values nearest to the real x: two at or below, two above."""
    c = np.float32(x)
    if float(c) > x:
        c = np.nextafter(c, NEG_INF)
    lo2 = np.nextafter(c, NEG_INF)
    hi1 = np.nextafter(c, POS_INF)
    hi2 = np.nextafter(hi1, POS_INF)
    return [np.float32(v) for v in (lo2, c, hi1, hi2)]
