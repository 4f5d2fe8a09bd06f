"""Kernel-level checks of launch_rescore (csrc/k_exact.hip) against the exact models of
tests/kcheck_exact.py, bit for bit: the distances and lists of every kernel build in modes A, B, S
and S-top and with the global threshold's exclusion bounds, the certification at its decision
boundaries, and the bookkeeping and publication of the batch's last kernel.

The builds are reached through the launcher's own conditions (kx.rescore_build restates them; the
environment switches are unset):
  k_rescore_kp<1>            mode S, <= 16 items, ld <= 1024, k <= 64        (plain and top_w)
  k_rescore<E,1,2,4>         one wave per item: /sel, /A, /B and /excl (ld > 1024, or publishing)
  k_rescore<E,8,2>           the item count read on the device (the second chance)
  k_rescore_flat<E,12|0>     exclusion bounds, ld <= 1024 (12: ld = 768)
"""
import numpy as np
import pytest

import kcheck as kc
import kcheck_exact as kx
from kcheck_exact import KEY_NONE, NEG_INF, POS_INF

pytestmark = pytest.mark.gpu

OFFSET = (1 << 33) + 5
KFILL, IFILL, CFILL = np.uint64(0x5A5A5A5A5A5A5A5A), np.uint64(0x1111111111111111), np.uint32(0x77777777)
KS_ALL = (1, 10, 64, 65, 100, 130, 256)  # E = ceil(k / 64) = 1 .. 4; 64 | 65: the last lane of a register | the next one
INVALID = 1  # hipErrorInvalidValue


@pytest.fixture(autouse=True, scope="module")
def _switches_unset():
    kx.assert_no_switches()


_corpora = {}


def corpus(dim):
    if dim not in _corpora:
        _corpora[dim] = kx.Corpus(6000 if dim == 64 else 2311, dim, 48, 900 + dim)
    return _corpora[dim]


def pick_rows(c, rng, m):
    """m distinct rows: the planted ones mixed with random ones."""
    pool = np.unique(np.concatenate([c.special_rows(), rng.choice(c.n, 3 * m + 10)]))
    if len(pool) < m:
        pool = np.arange(c.n)
    return rng.permutation(pool)[:m].astype(np.int64)


def launch(c, slots, k, *, nb=None, na=None, want_rc=0, hres=False, n_rows=None, **kw):
    """One launch_rescore over query slots holding the corpus queries `slots`.  Outputs start as
    patterns.  Returns the dict of every written buffer."""
    nq = len(slots)
    n_pad = c.rows.shape[0]
    o = dict(out_keys=np.full((nq, k), KFILL, np.uint64), fail_cnt=np.zeros(1, np.uint32),
             fail_list=np.full(nq + 1, 0xFFFFFFFF, np.uint32),
             res_idx=np.full((nq, k), IFILL, np.uint64), res_dist=np.full((nq, k), np.nan, np.float32),
             res_cnt=np.full(nq, CFILL, np.uint32))
    if hres:
        o.update(hres_idx=np.full((nq, k), IFILL, np.uint64), hres_dist=np.full((nq, k), np.nan, np.float32),
                 hres_cnt=np.full(nq, CFILL, np.uint32))
    # bounds, before anything runs: every row a kernel can gather lies in the slab, every query id in the batch
    if kw.get("cand_rows") is not None:
        assert kw["cand_rows"].shape == (nq, kw["kp"]) and kw["cand_rows"].max(initial=0) < n_pad
        assert len(kw["ncand"]) == nq and kw["ncand"].max(initial=0) <= kw["kp"] and len(kw["tau_excl"]) == nq
    if kw.get("cand_keys") is not None:
        ck = kw["cand_keys"]
        assert ck.shape == (nq, kw["cap"])
        assert kc.key_row(ck[ck != KEY_NONE]).max(initial=0) < n_pad
        if kw.get("excl_out") is not None:  # (k_rescore_flat gathers every slot below the count)
            for q in range(nq):
                assert kw["cnt"][q] > kw["cap"] or not (ck[q, :int(kw["cnt"][q])] == KEY_NONE).any()
        if not kw.get("top_w"):
            assert len(kw["cnt"]) == nq and len(kw["tau0"]) == nq
    if kw.get("qlist") is not None:
        assert kw["qlist"].max(initial=0) < nq and int(kw["n_items_dev"][0]) <= len(kw["qlist"])
    if kw.get("dead") is not None:
        assert kw["dead"].nbytes * 8 >= n_pad
    assert len(kw["ebound"]) == nq
    args = dict(rows=c.rows, ld=c.ld, dim=c.dim, na=c.na if na is None else na,
                qf32=np.ascontiguousarray(c.qf32[slots]),
                nb=np.ascontiguousarray(c.nb[slots] if nb is None else np.asarray(nb, np.float32)),
                k=k, offset=OFFSET, n_rows=c.n if n_rows is None else n_rows)
    args.update(o)
    args.update(kw)
    assert kx.rescore_raw(**args) == want_rc
    o.update({n: v for n, v in kw.items() if isinstance(v, np.ndarray)})
    return o


def result_rows(keys_k, k, cnt):
    idx = np.full(k, kx.IDX_NONE, np.uint64)
    dist = np.full(k, POS_INF, np.float32)
    has = (np.arange(k) < cnt) & (keys_k != KEY_NONE)
    idx[has] = np.uint64(OFFSET) + kc.key_row(keys_k[has]).astype(np.uint64)
    dist[has] = kx.key_dist(keys_k[has])
    return idx, dist


def check_rows(o, q, keys_k, cnt, pre="res"):
    k = len(keys_k)
    idx, dist = result_rows(keys_k, k, cnt)
    assert np.array_equal(o[pre + "_idx"][q], idx), (pre, q)
    assert np.array_equal(o[pre + "_dist"][q].view(np.uint32), dist.view(np.uint32)), (pre, q)
    assert o[pre + "_cnt"][q] == cnt, (pre, q)


def check_untouched(o, q, pre="res"):
    assert (o[pre + "_idx"][q] == IFILL).all() and np.isnan(o[pre + "_dist"][q]).all() and o[pre + "_cnt"][q] == CFILL, q


def check_fail(o, want_failed):
    n = int(o["fail_cnt"][0])
    assert n == len(want_failed), (n, sorted(want_failed))
    assert sorted(o["fail_list"][:n].tolist()) == sorted(want_failed)
    assert (o["fail_list"][n:] == 0xFFFFFFFF).all()


def score_keys(rng, rows, scores=None):
    rows = np.asarray(rows, np.uint64)
    if scores is None:
        scores = rng.uniform(-1, 1, len(rows))
    return kc.score_key(np.asarray(scores, np.float32), rows)


def key_lists(nq, cap, lists):
    ck = np.full((nq, cap), KEY_NONE, np.uint64)
    for q, keys in enumerate(lists):
        ck[q, :min(len(keys), cap)] = keys[:cap]
    return ck


def verdicts(c, slots, rows_of, tx, eb, nb, k, na=None):
    """Per slot: the model's k best keys over rows_of[q] and whether certify() accepts them."""
    want, ok = [], []
    for q, s in enumerate(slots):
        keys_k = kx.topk_keys(c.keys(s, rows_of[q], na=na, nb=nb[q]), k)
        want.append(keys_k)
        ok.append(kx.certify(tx[q], keys_k[k - 1], eb[q], nb[q]))
    return want, ok


# ----------------------------------------------------------------------------------------
# Distances and lists
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", kx.DIMS)
def test_mode_a(gpu, dim):
    """The k' candidates of k_select_cand: cand_rows / ncand / tau_excl."""
    c = corpus(dim)
    seen = set()
    for k in KS_ALL:
        rng = np.random.default_rng(31 * dim + k)
        kp = kx.kp_for(k)
        ncs = sorted({min(x, kp) for x in (0, 1, max(k - 1, 0), k, 63, 64, 65, kp)})
        nq = len(ncs)
        slots = list(range(nq))
        cand = np.zeros((nq, kp), np.uint32)
        rows_of = [pick_rows(c, rng, m) for m in ncs]
        for q, r in enumerate(rows_of):
            cand[q, :len(r)] = r
        tx = np.array([(NEG_INF, POS_INF, 0.2, -0.5)[q % 4] for q in range(nq)], np.float32)
        eb = np.full(nq, 0.01, np.float32)
        want, ok = verdicts(c, slots, rows_of, tx, eb, c.nb[slots], k)
        for n_rows, hres in ((c.n, k == 10), (max(k - 1, 1), False)):
            o = launch(c, slots, k, cand_rows=cand, ncand=np.array(ncs, np.uint32), kp=kp, tau_excl=tx, ebound=eb,
                       n_items=nq, hres=hres, n_rows=n_rows)
            for q in range(nq):
                assert np.array_equal(o["out_keys"][q], want[q]), (k, q)
                for pre in ("res", "hres") if hres else ("res",):
                    if ok[q]:
                        check_rows(o, q, want[q], min(k, n_rows), pre)
                    else:
                        check_untouched(o, q, pre)
            check_fail(o, [q for q in range(nq) if not ok[q]])
        assert any(ok) and not all(ok)
        seen.add(kx.rescore_build(n_items=nq, ld=c.ld, k=k, kp=kp, cap=0))
    assert seen == {f"k_rescore<{e},1,2,4>/A" for e in (1, 2, 3, 4)}, seen


@pytest.mark.parametrize("dim", kx.DIMS)
def test_mode_b_one_wave(gpu, dim):
    """Every emitted row of a list (cand_keys / cnt / tau0), one wave per query; KEY_NONE holes
    offer no row, an overflowed list offers none and cannot be certified."""
    c = corpus(dim)
    seen = set()
    for k in KS_ALL:
        rng = np.random.default_rng(57 * dim + k)
        kp, cap = kx.kp_for(k), kx.cap_for(k)
        big = min(cap, 2000)
        counts = [0, 1, 63, 64, 65, k, 300, big, cap + 5]
        nq = len(counts)
        slots = list(range(8, 8 + nq))
        lists, rows_of = [], []
        for q, m in enumerate(counts):
            rows = pick_rows(c, rng, min(m, big))
            keys = score_keys(rng, rows)
            if q == 6:  # holes
                holes = rng.choice(len(keys), 25, replace=False)
                keys[holes] = KEY_NONE
                rows = np.delete(rows, holes)
            lists.append(keys)
            rows_of.append(rows if m <= cap else np.zeros(0, np.int64))
        cnt = np.array(counts, np.uint32)
        tx = np.array([(NEG_INF, 0.2, -0.5)[q % 3] for q in range(nq)], np.float32)
        eb = np.full(nq, 0.01, np.float32)
        tx_eff = np.where(cnt > cap, POS_INF, tx).astype(np.float32)
        want, ok = verdicts(c, slots, rows_of, tx_eff, eb, c.nb[slots], k)
        o = launch(c, slots, k, cand_keys=key_lists(nq, cap, lists), cnt=cnt, cap=cap, tau0=tx, kp=kp, ebound=eb,
                   n_items=nq)
        for q in range(nq):
            assert np.array_equal(o["out_keys"][q], want[q]), (k, q)
            if ok[q]:
                check_rows(o, q, want[q], min(k, c.n))
            else:
                check_untouched(o, q)
        check_fail(o, [q for q in range(nq) if not ok[q]])
        assert not ok[-1] and any(ok)
        seen.add(kx.rescore_build(n_items=nq, ld=c.ld, k=k, kp=kp, cap=cap, keys=True))
    assert seen == {f"k_rescore<{e},1,2,4>/B" for e in (1, 2, 3, 4)}, seen


def dev_launch(c, k, n_dev, bound, seed, *, pub=False, ticket=None, hres=False):
    """The second chance: the item count on the device, the items' queries in qlist, 8 waves per
    item.  48 query slots; lists of 0, 1, 64*8-1, 64*8+1 and `big` keys, one with holes, one
    overflowed.  Returns (outputs, expectations)."""
    rng = np.random.default_rng(seed)
    st = kx.consts()
    nq = 48
    kp, cap = kx.kp_for(k), kx.cap_for(k)
    big = min(cap, 2000)
    slots = list(range(nq))
    qlist = rng.permutation(nq).astype(np.uint32)
    counts = [(0, 1, 511, 513, big, 300, cap + 9)[q % 7] for q in range(nq)]
    lists, rows_of = [], []
    for q, m in enumerate(counts):
        rows = pick_rows(c, rng, min(m, big))
        keys = score_keys(rng, rows)
        if q % 7 == 5:
            holes = rng.choice(len(keys), 40, replace=False)
            keys[holes] = KEY_NONE
            rows = np.delete(rows, holes)
        lists.append(keys)
        rows_of.append(rows if m <= cap else np.zeros(0, np.int64))
    cnt = np.array(counts, np.uint32)
    tx = np.array([(NEG_INF, 0.2, -0.5, 0.05)[q % 4] for q in range(nq)], np.float32)
    eb = np.full(nq, 0.01, np.float32)
    tx_eff = np.where(cnt > cap, POS_INF, tx).astype(np.float32)
    want, ok = verdicts(c, slots, rows_of, tx_eff, eb, c.nb[slots], k)
    emit = rng.integers(0, 5000, nq).astype(np.uint32)
    kw = dict(cand_keys=key_lists(nq, cap, lists), cnt=cnt, cap=cap, tau0=tx, kp=kp, ebound=eb, n_items=bound,
              n_items_dev=np.array([n_dev], np.uint32), qlist=qlist,
              next_status=np.full(st.st_words, CFILL, np.uint32), emit_cnt=emit,
              cur_status=np.full(st.st_words, CFILL, np.uint32), n_queries=nq - 3,
              merge_words=np.full(2, CFILL, np.uint32))
    if pub:
        kw.update(pub_alias=1, pub_bytes=nq * k * 8, pub_dst=np.full(nq * k * 8, 0xEE, np.uint8),
                  pub_flag=np.zeros(1, np.uint32),
                  pub_ticket=np.zeros(st.ticket_words, np.uint32) if ticket is None else ticket)
    o = launch(c, slots, k, hres=hres, **kw)
    items = qlist[:n_dev].tolist()
    for q in range(nq):
        if q in items:
            assert np.array_equal(o["out_keys"][q], want[q]), (k, q)
            for pre in ("res", "hres") if hres else ("res",):
                check_rows(o, q, want[q], min(k, c.n), pre)  # mode B: every item becomes result rows
        else:
            assert (o["out_keys"][q] == KFILL).all(), q
            check_untouched(o, q)
    check_fail(o, [q for q in items if not ok[q]])
    assert not o["next_status"].any(), "the next search's status words are zeroed"
    want_cur = np.full(st.st_words, CFILL, np.uint32)
    want_cur[st.st_emitted] = emit[:nq - 3].sum(dtype=np.uint32)
    assert np.array_equal(o["cur_status"], want_cur)
    assert o["merge_words"].tolist() == [0, 0xFFFFFFFF]
    if pub:
        assert np.array_equal(o["pub_dst"], o["res_idx"].view(np.uint8).ravel()), "the published copy"
        assert o["pub_flag"][0] == 1 and not o["pub_ticket"].any()
    build = kx.rescore_build(n_items=bound, ld=c.ld, k=k, kp=kp, cap=cap, keys=True, dev=True, pub=pub, qlist=True)
    return o, dict(ok=ok, items=items, build=build)


@pytest.mark.parametrize("dim", kx.DIMS)
def test_mode_b_device_counted(gpu, dim):
    c = corpus(dim)
    seen = set()
    for k in KS_ALL:
        for n_dev, bound in ((0, 16), (3, 16), (3, 40), (40, 40), (40, 16)):
            if k != 10 and (n_dev, bound) not in ((3, 16), (40, 40)):
                continue
            _, x = dev_launch(c, k, n_dev, bound, 1000 * dim + 10 * k + n_dev + bound)
            seen.add(x["build"])
    assert seen == {f"k_rescore<{e},8,2>" for e in (1, 2, 3, 4)}, seen


def s_lists(c, rng, kinds):
    """Mode S lists (kp = 63, cap = 1024) of the given kinds: 0 .. 5 emitted counts of 0, 1, kp, kp + 1,
    1024 and 1029 (overflowed); 6 .. 8 see below."""
    hi_a = np.float32(0.5)
    hi_b = np.array([0x80000000 | (~hi_a.view(np.uint32) & 0x7FFFFFFF)], np.uint32).view(np.float32)[0]
    lists, counts = [], []
    for kind in kinds:
        if kind < 6:
            m = (0, 1, 63, 64, 1024, 1029)[kind]
            keys = score_keys(rng, pick_rows(c, rng, min(m, 1024)))
        elif kind == 6:  # duplicated scores across the (kp+1)-th place
            sc = np.concatenate([np.full(60, 0.9), np.full(10, 0.5), np.full(130, 0.1)])
            keys = score_keys(rng, pick_rows(c, rng, 200), rng.permutation(sc))
            m = 200
        elif kind == 7:  # every high word equal
            keys, m = score_keys(rng, pick_rows(c, rng, 100), np.full(100, 0.25)), 100
        else:  # high words that differ only in their top bit
            keys, m = score_keys(rng, pick_rows(c, rng, 100), rng.permutation(np.repeat([hi_a, hi_b], 50))), 100
        lists.append(keys)
        counts.append(m)
    return lists, np.array(counts, np.uint32)


def s_check(c, slots, kinds, k, seed, dead=None):
    rng = np.random.default_rng(seed)
    nq, kp, cap = len(slots), 63, 1024
    lists, cnt = s_lists(c, rng, kinds)
    ck = key_lists(nq, cap, lists)
    tau0 = np.array([(-0.75, NEG_INF, 0.3)[q % 3] for q in range(nq)], np.float32)
    eb = np.full(nq, 0.01, np.float32)
    rows_of, tx = [], []
    for q in range(nq):
        r, t = kx.select_kp(ck[q], int(cnt[q]), cap, kp, tau0[q])
        if dead is not None:
            r = r[((dead.view(np.uint32)[r >> 5] >> (r & 31)) & 1) == 0]
        rows_of.append(r.astype(np.int64))
        tx.append(t)
    want, ok = verdicts(c, slots, rows_of, np.array(tx, np.float32), eb, c.nb[slots], k)
    o = launch(c, slots, k, cand_keys=ck, cnt=cnt, cap=cap, tau0=tau0, kp=kp, sel=1, ebound=eb, n_items=nq,
               dead=dead, hres=True)
    for q in range(nq):
        assert np.array_equal(o["out_keys"][q], want[q]), (k, q, kinds[q])
        for pre in ("res", "hres"):
            if ok[q]:
                check_rows(o, q, want[q], min(k, c.n), pre)
            else:
                check_untouched(o, q, pre)
    check_fail(o, [q for q in range(nq) if not ok[q]])
    return kx.rescore_build(n_items=nq, ld=c.ld, k=k, kp=kp, cap=cap, sel=1, keys=True), ok


def dead_bits(c, rng):
    """A bitset with a third of the rows deleted, the planted rows among them."""
    d = np.zeros(c.rows.shape[0] // 64, np.uint64)
    gone = np.unique(np.concatenate([rng.choice(c.n, c.n // 3, replace=False), c.ident[:2], [c.run + 1]]))
    np.bitwise_or.at(d, gone >> 6, np.uint64(1) << (gone & 63).astype(np.uint64))
    return d


@pytest.mark.parametrize("dim", kx.DIMS)
def test_mode_s(gpu, dim):
    """The rescore's own selection of the k' candidates (kp = 63, cap = 1024, k <= 10): 5 items reach
    k_rescore_kp (ld <= 1024), 40 items k_rescore; with a bitset of deleted rows, those offer no key."""
    c = corpus(dim)
    seen, oks = set(), []
    k40 = [q % 9 for q in range(40)]
    for k in (1, 10):
        for kinds in ((0, 1, 2, 3, 4), (5, 6, 7, 8)):  # (at most five items a launch)
            b, ok = s_check(c, list(range(kinds[0], kinds[0] + len(kinds))), kinds, k, 77 * dim + k + kinds[0])
            seen.add(b)
            oks += ok
        b, ok = s_check(c, list(range(40)), k40, k, 78 * dim + k)
        seen.add(b)
        oks += ok
    rng = np.random.default_rng(dim)
    seen.add(s_check(c, [0, 1, 2, 3, 4], (2, 3, 4, 6, 8), 10, 79 * dim, dead=dead_bits(c, rng))[0])
    seen.add(s_check(c, list(range(40)), k40, 10, 80 * dim, dead=dead_bits(c, rng))[0])
    assert any(oks) and not all(oks)
    want = {"k_rescore<1,1,2,4>/sel"} | ({"k_rescore_kp<1>"} if c.ld <= 1024 else set())
    assert seen == want, seen


def top_lists(c, rng, top_w, kind):
    """4 * top_w slots: ascending 4-lists with distinct rows."""
    rows = rng.permutation(c.n)[:4 * top_w].astype(np.uint64).reshape(top_w, 4)
    if kind == 5:
        sc = rng.integers(-4, 5, (top_w, 4)) / 8.0  # few distinct scores: ties across lists
    else:
        sc = rng.uniform(-1, 1, (top_w, 4))
    keys = np.sort(kc.score_key(sc.astype(np.float32), rows), axis=1)
    if kind == 1:    # lists with fewer than 4 keys
        for i in range(top_w):
            keys[i, rng.integers(0, 5):] = KEY_NONE
    elif kind == 2:  # few non-empty lists
        keep = rng.choice(top_w, min(top_w, 10), replace=False)
        mask = np.ones(top_w, bool)
        mask[keep] = False
        keys[mask] = KEY_NONE
    elif kind == 4:  # no list has a 4th key
        keys[:, 3] = KEY_NONE
        keys[::3, 1:] = KEY_NONE
    return keys.ravel()


@pytest.mark.parametrize("dim", (64, 130, 768, 1024))
@pytest.mark.parametrize("top_w", (4, 37, 512))
def test_mode_s_top(gpu, dim, top_w):
    """The self-thresholded selection (top_select): top_tau, top_cnt, the rewritten front of each
    list, the candidates and their certification."""
    c = corpus(dim)
    rng = np.random.default_rng(13 * dim + top_w)
    nq, k, kp, cap = 6, 10, 63, 4 * top_w
    slots = list(range(20, 20 + nq))
    ck = np.stack([top_lists(c, rng, top_w, q) for q in range(nq)])
    before = ck.copy()
    qflags = np.zeros(nq, np.uint32)
    qflags[3] = kx.consts().query_no_approx
    eb = np.full(nq, 0.01, np.float32)
    m = [kx.top_select(before[q], top_w, kp, served=q != 3) for q in range(nq)]
    want, ok = verdicts(c, slots, [x["rows"].astype(np.int64) for x in m], [x["tx"] for x in m], eb, c.nb[slots], k)
    o = launch(c, slots, k, cand_keys=ck, cap=cap, kp=kp, sel=1, top_w=top_w, qflags=qflags, ebound=eb, n_items=nq,
               top_tau=np.full(nq, np.nan, np.float32), top_cnt=np.full(nq, CFILL, np.uint32), hres=True)
    for q in range(nq):
        assert o["top_tau"][q].view(np.uint32) == np.float32(m[q]["top_tau"]).view(np.uint32), q
        assert o["top_cnt"][q] == m[q]["top_cnt"], q
        assert np.array_equal(o["cand_keys"][q], m[q]["list"]), q
        assert np.array_equal(o["out_keys"][q], want[q]), q
        for pre in ("res", "hres"):
            if ok[q]:
                check_rows(o, q, want[q], min(k, c.n), pre)
            else:
                check_untouched(o, q, pre)
    check_fail(o, [q for q in range(nq) if not ok[q]])
    assert not ok[3] and m[4]["top_tau"] == NEG_INF and (ok[4] or top_w > 4)
    assert kx.rescore_build(n_items=nq, ld=c.ld, k=k, kp=kp, cap=cap, sel=1, top_w=top_w, keys=True) == "k_rescore_kp<1>/top"


def test_top_w_and_dead_rejections(gpu):
    """launch_rescore refuses what its kernels do not implement, before any launch."""
    rng = np.random.default_rng(3)

    def top(c, nq=4, k=10, kp=63, top_w=4):
        ck = np.stack([top_lists(c, rng, top_w, 0) for _ in range(nq)])
        return launch(c, list(range(nq)), k, cand_keys=ck, cap=4 * top_w, kp=kp, sel=1, top_w=top_w,
                      qflags=np.zeros(nq, np.uint32), ebound=np.full(nq, 0.01, np.float32), n_items=nq,
                      top_tau=np.full(nq, np.nan, np.float32), top_cnt=np.full(nq, CFILL, np.uint32), want_rc=INVALID)

    c = corpus(768)
    for kw in (dict(nq=17), dict(k=65), dict(kp=64), dict(top_w=513)):
        o = top(c, **kw)
        assert (o["out_keys"] == KFILL).all() and np.isnan(o["top_tau"]).all()
    top(corpus(1100))  # ld > 1024
    # exclusion bounds with a bitset of deleted rows: k_rescore_flat does not read it
    nq, k = 5, 10
    cap = kx.cap_for(k)
    for cc in (c, corpus(1100)):
        lists = [score_keys(rng, pick_rows(cc, rng, 20)) for _ in range(nq)]
        o = launch(cc, list(range(nq)), k, cand_keys=key_lists(nq, cap, lists), cnt=np.full(nq, 20, np.uint32), cap=cap,
                   tau0=np.zeros(nq, np.float32), kp=kx.kp_for(k), ebound=np.full(nq, 0.01, np.float32), n_items=nq,
                   excl_out=np.full(nq, np.nan, np.float32), dead=np.zeros(cc.rows.shape[0] // 64, np.uint64),
                   want_rc=INVALID)
        assert (o["out_keys"] == KFILL).all() and np.isnan(o["excl_out"]).all()


def excl_launch(c, k, seed, *, pub=False, tx=None, eb=None, nb=None, counts=None):
    """The global threshold's rescore: every emitted row of every query, result rows for all, and
    the exclusion bound.  The four queries of the first workgroup hold 0, 1, 70 and 300 rows."""
    rng = np.random.default_rng(seed)
    st = kx.consts()
    kp, cap = kx.kp_for(k), kx.cap_for(k)
    counts = [0, 1, 70, 300, 5, 64, cap + 3, 200, 10, 3, 130] if counts is None else counts
    nq = len(counts)
    slots = list(range(nq))
    rows_of = [pick_rows(c, rng, m if m <= cap else 16) for m in counts]
    lists = [score_keys(rng, r) for r in rows_of]
    cnt = np.array(counts, np.uint32)
    if tx is None:
        tx = np.full(nq, 0.3, np.float32)
        tx[1], tx[5], tx[8], tx[9] = NEG_INF, 0.9999, -0.25, -0.5
        eb = np.full(nq, 0.01, np.float32)
        eb[4], eb[7], eb[9] = 1.0, np.nan, 0.999
    nbv = c.nb[slots] if nb is None else np.asarray(nb, np.float32)
    emit = rng.integers(0, 5000, nq).astype(np.uint32)
    kw = dict(cand_keys=key_lists(nq, cap, lists), cnt=cnt, cap=cap, tau0=tx, kp=kp, ebound=eb, n_items=nq,
              excl_out=np.full(nq, np.nan, np.float32), next_status=np.full(st.st_words, CFILL, np.uint32),
              emit_cnt=emit, cur_status=np.full(st.st_words, CFILL, np.uint32), n_queries=nq,
              merge_words=np.full(2, CFILL, np.uint32), nb=nbv)
    pub_bytes = nq * k * 8 // 16 * 16  # (the publish copies whole 16-byte units: the product's sizes are rounded to them)
    if pub:
        kw.update(pub_alias=1, pub_bytes=pub_bytes, pub_dst=np.full(pub_bytes, 0xEE, np.uint8),
                  pub_flag=np.zeros(1, np.uint32), pub_ticket=np.zeros(st.ticket_words, np.uint32))
    o = launch(c, slots, k, **kw)
    bounds = []
    for q in range(nq):
        over = counts[q] > cap
        want = kx.topk_keys(c.keys(q, np.zeros(0, np.int64) if over else rows_of[q], nb=nbv[q]), k)
        assert np.array_equal(o["out_keys"][q], want), (k, q)
        check_rows(o, q, want, 0 if over else min(k, counts[q]))
        b = kx.exclusion_bound(POS_INF if over else tx[q], eb[q], nbv[q])
        assert o["excl_out"][q].view(np.uint32) == b.view(np.uint32), (k, q, o["excl_out"][q], b)
        bounds.append(b)
    assert o["fail_cnt"][0] == 0, "no local certification"
    assert not o["next_status"].any()
    assert o["cur_status"][st.st_emitted] == emit.sum(dtype=np.uint32) and o["merge_words"].tolist() == [0, 0xFFFFFFFF]
    if pub:
        assert np.array_equal(o["pub_dst"], o["res_idx"].view(np.uint8).ravel()[:pub_bytes])
        assert o["pub_flag"][0] == 1 and not o["pub_ticket"].any()
    return bounds, kx.rescore_build(n_items=nq, ld=c.ld, k=k, kp=kp, cap=cap, keys=True, excl=True, pub=pub)


@pytest.mark.parametrize("dim", kx.DIMS)
def test_exclusion_bounds(gpu, dim):
    c = corpus(dim)
    seen = set()
    for k in KS_ALL:
        bounds, b = excl_launch(c, k, 400 * dim + k)
        seen.add(b)
        assert bounds[1] == POS_INF and bounds[6] == NEG_INF and bounds[4] == NEG_INF and bounds[5] == NEG_INF
        assert bounds[7] == NEG_INF and np.isfinite(bounds[0]) and np.isfinite(bounds[9])
    es = (1, 2, 3, 4)
    if dim == 1100:
        want = {f"k_rescore<{e},1,2,4>/excl" for e in es}
    else:
        want = {f"k_rescore_flat<{e},{12 if dim == 768 else 0}>" for e in es}
    assert seen == want, seen


def test_kernel_reads_the_magnitudes_it_is_given(gpu):
    """na and nb doubled: every distance follows the model with THOSE magnitudes (a kernel that
    recomputed the norms would not); the identical rows stay at 0, the row 2e-10 away does not."""
    c = corpus(130)
    rng = np.random.default_rng(8)
    k, kp = 10, 63
    na2 = (c.na * np.float32(2)).astype(np.float32)
    planted = np.array(c.ident + [c.near] + c.zero)
    rows = np.concatenate([planted, np.setdiff1d(pick_rows(c, rng, 50), planted)])[:kp]
    nq = 3
    cand = np.zeros((nq, kp), np.uint32)
    cand[:, :len(rows)] = rows
    nb2 = (c.nb[:nq] * np.float32(2)).astype(np.float32)
    o = launch(c, [0, 1, 2], k, na=na2, nb=nb2, cand_rows=cand, ncand=np.full(nq, len(rows), np.uint32), kp=kp,
               tau_excl=np.full(nq, NEG_INF, np.float32), ebound=np.zeros(nq, np.float32), n_items=nq)
    for q in range(nq):
        want = kx.topk_keys(c.keys(q, rows, na=na2, nb=nb2[q]), k)
        assert np.array_equal(o["out_keys"][q], want)
        assert not np.array_equal(want, kx.topk_keys(c.keys(q, rows), k)), "the case must tell the two apart"
    d0 = kx.key_dist(o["out_keys"][0])
    assert (d0[:3] == 0).all() and kc.key_row(o["out_keys"][0][:3]).tolist() == sorted(c.ident)
    near = o["out_keys"][0][kc.key_row(o["out_keys"][0]) == c.near]
    assert len(near) == 1 and kx.key_dist(near)[0] > 0.5  # (about 1 - 1/4: not identical, and the doubled norms)


# ----------------------------------------------------------------------------------------
# Certification at its decision boundaries
# ----------------------------------------------------------------------------------------
E_BOUNDARY = (np.float32(1e-3), np.float32(0.02))


def second_condition_cases(c, k, rows_of, slots, nb):
    """Per slot (4 per pair of query and E): tau_x at the four f32 values nearest to
    1 - dk - E - 2.5e-7, dk the model's k-th distance over the slot's candidate rows."""
    tx, eb = [], []
    for q, s in enumerate(slots):
        E = E_BOUNDARY[(q // 4) % 2]
        dk = float(kx.key_dist(kx.topk_keys(c.keys(s, rows_of[q], nb=nb[q]), k)[k - 1]))
        tx.append(kx.f32_neighbours(1.0 - dk - float(E) - 2.5e-7)[q % 4])
        eb.append(E)
    return np.array(tx, np.float32), np.array(eb, np.float32)


def third_condition_cases(nq):
    """Per slot (4 per pair of |b| and E): a row identical to the query in the list and k = 1, so
    dk = 0; tau_x at the four f32 values nearest to 1 - E - 1e-4 - 6e-9 / |b|."""
    tx, eb, nb = [], [], []
    for q in range(nq):
        E, b = E_BOUNDARY[(q // 4) % 2], (np.float32(1.0), np.float32(1e-6))[(q // 8) % 2]
        tx.append(kx.f32_neighbours(1.0 - float(E) - 1e-4 - 6e-9 / float(b))[q % 4])
        eb.append(E)
        nb.append(b)
    return np.array(tx, np.float32), np.array(eb, np.float32), np.array(nb, np.float32)


def boundary_launch(c, mode, k, nq, seed, third):
    """One launch of `mode` with tau_x planted per slot; returns (failed per the kernel == the
    model asserted inside, the model's verdicts, the build)."""
    rng = np.random.default_rng(seed)
    kp = 63 if mode in ("S", "top") else kx.kp_for(k)
    cap = {"S": 1024, "top": 4 * 37}.get(mode, kx.cap_for(k))
    slots = [0] * nq if third else [q % 8 for q in range(nq)]  # (query 0 has rows identical to it)
    m = 44 if mode == "top" else kp if mode in ("S", "A") else min(cap, 700)
    rows_of = []
    for q in range(nq):
        r = pick_rows(c, rng, m)
        if third and c.ident[0] not in r:
            r[0] = c.ident[0]
        rows_of.append(r)
    if third:
        tx, eb, nb = third_condition_cases(nq)
    else:
        nb = np.ascontiguousarray(c.nb[slots])
        tx, eb = second_condition_cases(c, k, rows_of, slots, nb)
    want, ok = verdicts(c, slots, rows_of, tx, eb, nb, k)
    kw = dict(ebound=eb, n_items=nq, kp=kp, nb=nb)
    if mode == "A":
        cand = np.stack([r.astype(np.uint32) for r in rows_of])
        kw.update(cand_rows=cand, ncand=np.full(nq, m, np.uint32), tau_excl=tx)
    elif mode in ("B", "dev"):
        kw.update(cand_keys=key_lists(nq, cap, [score_keys(rng, r) for r in rows_of]), cnt=np.full(nq, m, np.uint32),
                  cap=cap, tau0=tx)
        if mode == "dev":
            kw.update(n_items_dev=np.array([nq], np.uint32), qlist=rng.permutation(nq).astype(np.uint32))
    elif mode == "S":
        # the kp candidates score above tau_x, the (kp+1)-th row scores tau_x exactly, 20 more lie below
        lists = []
        for q in range(nq):
            extra = np.setdiff1d(np.arange(c.n), rows_of[q])[:21]
            sc = np.concatenate([np.float32(tx[q]) + rng.uniform(1, 2, kp), [tx[q]], np.float32(tx[q]) - rng.uniform(1, 2, 20)])
            order = rng.permutation(kp + 21)
            lists.append(score_keys(rng, np.concatenate([rows_of[q], extra])[order], sc.astype(np.float32)[order]))
        kw.update(cand_keys=key_lists(nq, cap, lists), cnt=np.full(nq, kp + 21, np.uint32), cap=cap, sel=1,
                  tau0=np.full(nq, NEG_INF, np.float32))
    else:  # top: 44 keys <= kp, all candidates; list 0 alone has a 4th key, X, whose score is tau_x
        lists = np.full((nq, cap), KEY_NONE, np.uint64)
        for q in range(nq):
            r = rows_of[q].astype(np.uint64)
            lists[q, :4] = np.sort(kc.score_key(np.array([tx[q] + 3, tx[q] + 2, tx[q] + 1, tx[q]], np.float32), r[:4]))
            for i in range(20):
                lists[q, 4 + 4 * i:6 + 4 * i] = np.sort(score_keys(rng, r[4 + 2 * i:6 + 2 * i]))
            assert kx.top_select(lists[q], 37, kp)["tx"].view(np.uint32) == np.float32(tx[q]).view(np.uint32)
        kw.update(cand_keys=lists, cap=cap, sel=1, top_w=37, qflags=np.zeros(nq, np.uint32),
                  top_tau=np.full(nq, np.nan, np.float32), top_cnt=np.full(nq, CFILL, np.uint32))
    o = launch(c, slots, k, **kw)
    for q in range(nq):
        assert np.array_equal(o["out_keys"][q], want[q]), (mode, k, q)
    check_fail(o, [q for q in range(nq) if not ok[q]])
    build = kx.rescore_build(n_items=nq, ld=c.ld, k=k, kp=kp, cap=cap, sel=mode in ("S", "top"),
                             top_w=37 if mode == "top" else 0, dev=mode == "dev", keys=mode != "A", qlist=mode == "dev")
    return ok, build


BOUNDARY_MODES = (("A", 32), ("B", 32), ("dev", 16), ("dev", 32), ("S", 16), ("S", 32), ("top", 16))


@pytest.mark.parametrize("mode,nq", BOUNDARY_MODES)
def test_certify_second_condition_boundary(gpu, mode, nq):
    """dk < 1 - tau_x - E - 2.5e-7, strictly, in f64: of four adjacent f32 values of tau_x the model
    says which certify; the kernel's failure list must be exactly the others."""
    seen = set()
    for dim in (768, 1100) if mode in ("A", "B", "dev") else (768,):
        c = corpus(dim)
        for k in ((10, 64, 65, 100, 130, 256) if mode in ("A", "B", "dev") and dim == 768 else (10,)):
            ok, b = boundary_launch(c, mode, k, nq, 5000 + 7 * k + nq, third=False)
            assert any(ok) and not all(ok), (mode, k, ok)
            for g in range(0, nq, 4):  # each group of four is cut somewhere inside or at its edge ...
                assert ok[g:g + 4] == sorted(ok[g:g + 4], reverse=True), "certified below the bound, not above"
            seen.add(b)
    if mode in ("A", "B"):
        assert seen == {f"k_rescore<{e},1,2,4>/{mode}" for e in (1, 2, 3, 4)}, seen
    elif mode == "dev":
        assert seen == {f"k_rescore<{e},8,2>" for e in (1, 2, 3, 4)}, seen
    elif mode == "S":
        assert seen == {"k_rescore_kp<1>" if nq <= 16 else "k_rescore<1,1,2,4>/sel"}, seen
    else:
        assert seen == {"k_rescore_kp<1>/top"}, seen


@pytest.mark.parametrize("mode,nq", BOUNDARY_MODES)
def test_certify_third_condition_boundary(gpu, mode, nq):
    """tau_x < 1 - E - 1e-4 - 6e-9 / |b|: with a row identical to the query as the k = 1 result the
    second condition holds throughout, and tau_x walks across the third for |b| in {1, 1e-6}."""
    c = corpus(768)
    ok, _ = boundary_launch(c, mode, 1, nq, 6000 + nq, third=True)
    assert any(ok) and not all(ok), (mode, ok)
    for g in range(0, nq, 4):
        assert any(ok[g:g + 4]) and not all(ok[g:g + 4]), "every group of four straddles the bound"


def test_certify_special_cases(gpu):
    """tau_x = -inf certifies a short list; a finite tau_x with fewer than k keys fails; E of 0.999,
    1.0 and NaN; an overflowed list fails.  Modes A and B in one launch each: certify() is one
    device function, and the device-counted and mode S builds meet tau_x = -inf, short and overflowed
    lists only through the mixes of dev_launch, s_check and test_mode_s_top, not case by case here."""
    c = corpus(130)
    rng = np.random.default_rng(21)
    k, kp, cap = 10, kx.kp_for(10), kx.cap_for(10)
    #         tx       E      rows
    cases = ((NEG_INF, 0.01, 4), (-0.9, 0.01, 4), (-3.0, 0.999, 40), (-3.0, 1.0, 40), (-3.0, np.nan, 40),
             (NEG_INF, np.nan, 40), (POS_INF, 0.0, 40), (-0.9, 0.01, 40))
    nq = len(cases)
    slots = list(range(nq))
    tx = np.array([t for t, _, _ in cases], np.float32)
    eb = np.array([e for _, e, _ in cases], np.float32)
    rows_of = [pick_rows(c, rng, m) for _, _, m in cases]
    want, ok = verdicts(c, slots, rows_of, tx, eb, c.nb[slots], k)
    assert ok == [True, False, True, False, False, True, False, True]
    cand = np.zeros((nq, kp), np.uint32)
    for q, r in enumerate(rows_of):
        cand[q, :len(r)] = r
    o = launch(c, slots, k, cand_rows=cand, ncand=np.array([m for _, _, m in cases], np.uint32), kp=kp, tau_excl=tx,
               ebound=eb, n_items=nq)
    check_fail(o, [q for q in range(nq) if not ok[q]])
    cnt = np.array([m for _, _, m in cases], np.uint32)
    cnt[7] = cap + 1  # the last case, certified above, overflowed
    o = launch(c, slots, k, cand_keys=key_lists(nq, cap, [score_keys(rng, r) for r in rows_of]), cnt=cnt, cap=cap,
               tau0=tx, kp=kp, ebound=eb, n_items=nq)
    check_fail(o, [q for q in range(nq) if not ok[q] or q == 7])


def test_exclusion_bound_boundaries(gpu):
    """The bits of excl_out for tau0 at the f32 neighbours of the third condition's edge and for
    ordinary thresholds (rounded down), both kernels (k_rescore_flat, k_rescore)."""
    for dim in (768, 1100):
        c = corpus(dim)
        nq = 16
        tx, eb, nb = third_condition_cases(nq)
        bounds, _ = excl_launch(c, 10, 9 + dim, tx=tx, eb=eb, nb=nb, counts=[30 + q for q in range(nq)])
        assert any(b == NEG_INF for b in bounds) and any(np.isfinite(b) for b in bounds)
        tx = np.linspace(-0.9, 0.9, nq).astype(np.float32)
        bounds, _ = excl_launch(c, 10, 10 + dim, tx=tx, eb=np.full(nq, 0.02, np.float32),
                                counts=[30 + q for q in range(nq)])
        assert all(np.isfinite(b) for b in bounds)


# ----------------------------------------------------------------------------------------
# Bookkeeping and publication
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dev,bound", ((3, 16), (40, 40), (0, 16), (0, 40)))
def test_second_chance_publishes(gpu, n_dev, bound):
    """The batch's last kernel: the solo grid, a grid of 40 workgroups and a device count of 0; the
    published copy is what the kernel left in the result buffer, the flag is raised, the ticket is
    zero again -- and a second launch with the same ticket buffer gives the same."""
    c = corpus(768)
    o1, x = dev_launch(c, 10, n_dev, bound, 33 + n_dev, pub=True, hres=True)
    assert x["build"] == "k_rescore<1,8,2>"
    o2, _ = dev_launch(c, 10, n_dev, bound, 33 + n_dev, pub=True, hres=True, ticket=o1["pub_ticket"])
    for name in ("out_keys", "res_idx", "res_dist", "res_cnt", "pub_dst", "hres_idx"):
        assert np.array_equal(o1[name].view(np.uint8), o2[name].view(np.uint8)), name
    assert sorted(o1["fail_list"][:o1["fail_cnt"][0]].tolist()) == sorted(o2["fail_list"][:o2["fail_cnt"][0]].tolist())


@pytest.mark.parametrize("dim", (768, 1100))
def test_global_threshold_launch_publishes(gpu, dim):
    """With the publish fields the global threshold's rescore takes k_rescore (4 items per workgroup)."""
    seen = set()
    for k in (10, 65, 130, 256):
        seen.add(excl_launch(corpus(dim), k, 71 + dim + k, pub=True)[1])
    assert seen == {f"k_rescore<{e},1,2,4>/excl" for e in (1, 2, 3, 4)}, seen
