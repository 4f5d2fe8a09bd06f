"""launch_deep_cap_scan_list (csrc/k_exact.hip) through its test-only shim (kcheck_deep_cap_list): one
query group over one list segment, over two segments of one list with the carry between them, and on
one or two workgroups so that full buffers are compacted -- bit for bit against kcheck_cap's model
over kcheck_exact's distances of the listed rows."""
import numpy as np
import pytest

import kcheck_cap as kp
import kcheck_deep_cap_list as kd
import kcheck_exact as kx

pytestmark = pytest.mark.gpu

U64 = np.uint64
OFFSET = 1 << 33
NQ = 4
KM = ((1, 1), (257, 3), (1024, 16), (1024, 1), (257, 16))
# (name, list length, groups): few groups -- the cap drops most rows, the answer lies far beyond the
# k-th nearest, fewer keepable rows than k; one group -- count min(m, k); every row its own group --
# nothing is dropped; ties -- the run of identical rows alone, the index decides
CASES = (("few", 5000, 4), ("few", 3000, 40), ("few", 257, 4), ("few", 255, 300), ("one", 3000, 1), ("own", 3000, 0),
         ("ties", 100, 7), ("few", 1, 4), ("few", 0, 4))

_corpora, _models = {}, {}


def corpus(dim):
    if dim not in _corpora:
        c = kx.Corpus(5300, dim, NQ, 2900 + dim)
        c.all_dist = [c.dist(q) for q in range(c.nq)]
        _corpora[dim] = c
    return _corpora[dim]


def listed(corp, case, length, G):
    rng = np.random.default_rng(length + G)
    if case == "ties":
        rows = np.array(corp.special_rows()[-100:])
    else:
        special = np.array(corp.special_rows())[:length // 2]  # (identical rows, zero rows, the run of ties)
        rest = rng.choice(np.setdiff1d(np.arange(corp.n), special), length - len(special), replace=False)
        rows = np.sort(np.concatenate([special, rest]))
    rg = rng.integers(0, G, corp.n) if G else np.arange(corp.n)
    return rows.astype(np.uint32), rg.astype(np.uint32)


def model(corp, dim, case, length, G, rows, rg, q, m):
    """(keys, idx, dist, group, count) at k = 1024; the result at a smaller k is its prefix."""
    key = (dim, case, length, G, q, m)
    if key not in _models:
        allowed = np.zeros(corp.n, bool)
        allowed[rows] = True
        idx, dist, grp, c = kp.cap_model(corp.all_dist[q], rg, 1024, m, allowed=allowed, offset=OFFSET)
        keys = np.full(1024, kx.KEY_NONE, U64)
        keys[:c] = kx.dist_key(dist[:c], idx[:c] - U64(OFFSET))
        _models[key] = (keys, idx, dist, grp, c)
    return _models[key]


@pytest.mark.parametrize("dim", (64, 130, 768))
@pytest.mark.parametrize("qf,nq_own", ((1, 1), (2, 1), (2, 2)))
@pytest.mark.parametrize("case,length,G", CASES)
def test_deep_cap_scan_list(gpu, dim, qf, nq_own, case, length, G):
    corp = corpus(dim)
    rows, rg = listed(corp, case, length, G)
    own = [1, 3][:nq_own]
    qids = own + [own[0]] * (qf - nq_own)  # (a padding slot: its part is never written, never merged)
    cut = length // 3
    # grid 0: one workgroup a tile; 1 and 2 (the long lists): every buffer fills and is compacted
    runs = [([(0, length)], 0)] + ([([(0, cut), (cut, length - cut)], 0)] if cut else []) + \
        ([([(0, length)], 1), ([(0, cut), (cut, length - cut)], 2)] if length >= 3000 else [])
    for k, m in KM:
        for segs, grid in runs:
            carry, idx, dist, cnt, grp = kd.scan(corp, rg, rows, segs, qids, nq_own, k, min(m, k), grid, OFFSET)
            for q in range(NQ):
                ctx = (k, m, len(segs), grid, q)
                if q not in own:
                    assert (carry[q] == kx.KEY_NONE).all() and cnt[q] == 0, ctx
                    continue
                keys, wi, wd, wg, c = model(corp, dim, case, length, G, rows, rg, q, m)
                c = min(c, k)
                assert cnt[q] == c and np.array_equal(carry[q, :c], keys[:c]) and (carry[q, c:] == kx.KEY_NONE).all(), ctx
                assert np.array_equal(idx[q, :c], wi[:c]) and (idx[q, c:] == kx.IDX_NONE).all(), ctx
                assert np.array_equal(dist[q, :c].view(np.uint32), wd[:c].view(np.uint32)), ctx
                assert np.isposinf(dist[q, c:]).all(), ctx
                assert np.array_equal(grp[q, :c], wg[:c]) and (grp[q, c:] == kp.GROUP_NONE).all(), ctx
    if case == "one":
        assert c == min(KM[-1][1], KM[-1][0])  # (one group holds the whole list: min(m, k) rows)
