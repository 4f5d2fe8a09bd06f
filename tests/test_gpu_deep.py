"""Deep search (bsr_local_top_k_deep) through the C ABI.  Every expected row is the
oracle's top-1024 of the live rows (oracle.parallel_top_k, one rank), computed once per shard and
cut to k; indices, order and distance bits must be equal -- no tolerance anywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
PAD = np.uint64(2 ** 64 - 1)
KMAX, OFFSET = 1024, 7000
E_INVALID, E_NONFINITE, E_STATE = -1, -2, -7
SHAPES = [(64, 40_000), (768, 40_000), (130, 50_001)]
_made = {}


def shard(bsr_mod, oracle_mod, dim, n, flags=0, nq=40, plant=None, dead=None):
    """(index, queries, oracle top-1024 with global ids) of a U(-1, 1) shard, made once per key."""
    key = (dim, n, flags, nq, plant is not None, dead is not None)
    if key not in _made:
        rng = np.random.default_rng(dim * 1000 + n)
        rows = rng.uniform(-1, 1, (n, dim)).astype(F)
        qs = rng.uniform(-1, 1, (nq, dim)).astype(F)
        if plant:
            plant(rng, rows, qs)
        ix = bsr_mod.Index(dim, max_k=256, device=0, flags=flags)
        ix.load(rows, global_offset=OFFSET)
        live = np.arange(n)
        if dead is not None:
            gone = dead(rng, oracle_mod, rows, qs)
            assert ix.delete(gone + OFFSET) == len(gone)
            live = np.setdiff1d(live, gone)
        wi, wd, wc = oracle_mod.parallel_top_k(rows[live], qs, KMAX, size=1, threads=8)
        _made[key] = (ix, qs, (live[wi.astype(np.int64)].astype(np.uint64) + np.uint64(OFFSET), wd, wc))
    return _made[key]


def check(got, ref, k, nq=None):
    gi, gd, gc = got
    wi, wd, wc = ref
    for q in range(len(gc) if nq is None else nq):
        c = min(k, int(wc[q]))
        assert gc[q] == c
        assert np.array_equal(gi[q, :c], wi[q, :c]), f"query {q}: indices / order"
        assert np.array_equal(gd[q, :c].view(np.uint32), wd[q, :c].view(np.uint32)), f"query {q}: distance bits"
        assert np.all(gi[q, c:] == PAD) and np.all(np.isposinf(gd[q, c:]))


@pytest.mark.parametrize("k", [1, 257, 1000, 1024])
@pytest.mark.parametrize("nq", [3, 40])
@pytest.mark.parametrize("dim,n", SHAPES)
def test_filter_rung(bsr_mod, oracle_mod, gpu, dim, n, nq, k):
    ix, qs, ref = shard(bsr_mod, oracle_mod, dim, n)
    check(ix.deep_search(qs[:nq], k), ref, k)
    st = ix.last_stats()
    print(f"emitted/query={st.n_emitted / nq:.0f} fallback={st.n_fallback} direct={st.n_exact_direct} "
          f"cap={st.n_candidates}")
    assert st.search_path & bsr_mod.BSR_PATH_DEEP and st.n_queries == nq
    assert st.n_fallback + st.n_exact_direct <= nq / 10  # (the scan must not hide a rung that never certifies)


def test_agreement(bsr_mod, oracle_mod, gpu):
    ix, qs, _ = shard(bsr_mod, oracle_mod, 768, 40_000)
    for a, b in zip(ix.deep_search(qs, 256), ix.local_top_k(qs, 256)):
        assert a.tobytes() == b.tobytes()
    deep, shallow = ix.deep_search(qs, 1000), ix.deep_search(qs, 257)
    assert np.array_equal(deep[0][:, :257], shallow[0]) and np.array_equal(deep[1][:, :257], shallow[1])


@pytest.mark.parametrize("exact_only,n,k,nq", [(True, 40_000, 1000, 5), (False, 3000, 1000, 7), (False, 3000, 1024, 6),
                                               (False, 256 * 3 + 1, 1000, 5)])
def test_scan_rung_alone(bsr_mod, oracle_mod, gpu, exact_only, n, k, nq):
    ix, qs, ref = shard(bsr_mod, oracle_mod, 64, n, flags=bsr_mod.BSR_FLAG_EXACT_ONLY if exact_only else 0, nq=nq)
    got = ix.deep_search(qs, k)
    check(got, ref, k)
    assert np.all(got[2] == min(k, n))  # (k > n: count = n, padding behind)
    st = ix.last_stats()
    assert st.search_path == bsr_mod.BSR_PATH_DEEP | bsr_mod.BSR_PATH_DEEP_SCAN
    assert st.n_exact_direct == nq and st.n_fallback == 0 and st.n_emitted == 0


def plant_ladder(rng, rows, qs):
    n, dim = rows.shape
    qs[0] = rows[5] + rng.uniform(-0.01, 0.01, dim).astype(F)  # 3000 near-duplicates hold its answer
    rows[1000:4000] = qs[0] + rng.uniform(-0.02, 0.02, (3000, dim)).astype(F)
    rows[rng.permutation(np.arange(4000, n))[:20_000]] = rows[4500]  # 20 000 exact copies: ties by index
    qs[1] = rows[4500]
    qs[2] = 0  # distance 1.0 everywhere: index order


def test_ladder_in_one_batch(bsr_mod, oracle_mod, gpu):
    ix, qs, ref = shard(bsr_mod, oracle_mod, 64, 45_000, nq=8, plant=plant_ladder)
    check(ix.deep_search(qs, 1000), ref, 1000)
    assert np.all(ref[1][1, :1000] == 0) and np.all(ref[1][2, :1000] == 1) and np.all(np.diff(ref[0][2]) == 1)
    st = ix.last_stats()
    assert st.search_path & bsr_mod.BSR_PATH_DEEP_SCAN and st.n_fallback >= 1 and st.n_exact_direct >= 1


def dead_rows(rng, oracle_mod, rows, qs):
    top = oracle_mod.parallel_top_k(rows, qs[:1], 1000, size=1, threads=1)[0][0].astype(np.int64)
    return np.union1d(top[::2], np.flatnonzero(rng.random(len(rows)) < 0.3))  # half of query 0's top 1000 too


@pytest.mark.parametrize("n,k", [(40_000, 1000), (1300, 1024)])
def test_tombstones(bsr_mod, oracle_mod, gpu, n, k):
    ix, qs, ref = shard(bsr_mod, oracle_mod, 64, n, nq=6, dead=dead_rows)
    got = ix.deep_search(qs, k)
    check(got, ref, k)
    assert np.all(got[2] == min(k, ix.live_count()))  # (n = 1300: live < k, count = live)


def test_device_pointers(bsr_mod, oracle_mod, gpu):
    import torch
    ix, qs, ref = shard(bsr_mod, oracle_mod, 64, 40_000)
    dev = torch.device("cuda:0")
    oi = torch.zeros((40, 1000), dtype=torch.int64, device=dev)
    od = torch.zeros((40, 1000), dtype=torch.float32, device=dev)
    oc = torch.zeros(40, dtype=torch.int32, device=dev)
    ix.deep_search_device(torch.from_numpy(qs).to(dev), 40, 1000, oi, od, oc)
    torch.cuda.synchronize()
    host = ix.deep_search(qs, 1000)
    for d, h in zip((oi, od, oc), host):
        assert d.cpu().numpy().tobytes() == h.tobytes()
    check(host, ref, 1000)


@pytest.mark.parametrize("case", ["k0", "k1025", "null_out", "not_loaded", "nan_query"])
def test_argument_checks(bsr_mod, oracle_mod, gpu, case):
    ix, qs, _ = shard(bsr_mod, oracle_mod, 64, 40_000)
    q, k = qs[:4].copy(), {"k0": 0, "k1025": 1025}.get(case, 300)
    oi, od, oc = np.full((4, 1025), 0x1234, np.uint64), np.full((4, 1025), -3.0, F), np.full(4, 0x5A5A, np.uint32)
    want = E_INVALID
    if case == "not_loaded":
        ix, want = bsr_mod.Index(64, max_k=16, device=0), E_STATE
    if case == "nan_query":
        q[2, 7], want = np.nan, E_NONFINITE
    with pytest.raises(bsr_mod.BsrError) as e:
        ix.deep_search_device(q, 4, k, oi, od, None if case == "null_out" else oc)
    assert e.value.status == want
    assert np.all(oi == 0x1234) and np.all(od == -3.0) and np.all(oc == 0x5A5A)  # (untouched)
