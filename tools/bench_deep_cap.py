#!/usr/bin/env python3
"""Deep capped search timings, tools/bench_deep.py's protocol: a synthetic shard
(default 1M x 768 f32, seed 42), 1000 device queries (seed 43), device outputs, 100k groups
(row_group uniform, seed 44), k in {257, 1000} x per_group in {1, 3}.

Per point: bsr_local_top_k_deep_capped, next to the route without it -- bsr_local_top_k_deep(k),
the groups of its rows looked up (a torch gather), bsr_global_top_k_capped on the device over that
one list -- which is inexact whenever the cap drops a row (its count falls short of k).  Medians of
--reps calls after warm-up with min and max, the emitted keys per query, the fallbacks, the stage
times of profile level 2, and the rank in the plain order of the last row the walk keeps (its
position in bsr_local_top_k_deep(1024)'s list; beyond it: counted).  Then one scanned query (an
index that cannot filter) at 1, 3 and 16 table entries per group.

    python tools/bench_deep_cap.py --out profiles/deep_cap_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "better-search-rag-rust_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--groups", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import bsr

    dev = "cuda:0"
    n, dim, nq, G = args.rows, args.dim, args.queries, args.groups
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(rows.data_ptr(), 0, n, dim, 42)
    qdev = torch.empty((nq, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qdev.data_ptr(), 0, nq, dim, 43)
    rg = torch.randint(0, G, (n,), dtype=torch.int32, device=dev, generator=torch.Generator(dev).manual_seed(44))
    torch.cuda.synchronize()
    ix = bsr.Index(dim, max_k=256, device=0, flags=bsr.BSR_FLAG_PROFILE)
    ix.set_profile(0)
    ix.load(rows)

    def outs(q, k):
        return (torch.empty((q, k), dtype=torch.int64, device=dev), torch.empty((q, k), dtype=torch.float32, device=dev),
                torch.empty((q,), dtype=torch.int32, device=dev), torch.empty((q, k), dtype=torch.int32, device=dev))

    def timed(fn, reps, warmup):
        for _ in range(warmup):
            fn()
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), calls=len(t))

    def staged(index, fn, calls):
        index.set_profile(2)
        index.profile(reset=True)
        for _ in range(calls):
            fn()
        p = index.profile(reset=True)
        index.set_profile(0)
        return dict(rescore_ms=p.rescore_ms / calls, scan_ms=p.scan_ms / calls, emit_ms=p.gemm_emit_ms / calls,
                    sample_ms=p.gemm_sample_ms / calls, profiled_search_ms=p.search_ms / calls)

    d1024 = outs(nq, 1024)
    ix.deep_search_device(qdev, nq, 1024, *d1024[:3])
    points = {}
    for k in (257, 1000):
        for m in (1, 3):
            oi, od, oc, og = outs(nq, k)
            bi, bd, bc, bg = outs(nq, k)
            li, ld, lc, _ = outs(nq, k)

            def new():
                ix.deep_capped_search_device(qdev, nq, k, m, rg, G, oi, od, oc, out_group=og)

            def base():
                ix.deep_search_device(qdev, nq, k, li, ld, lc)
                lg = rg[li.clamp(0, n - 1)]  # (a full list: every slot is a row)
                bsr.merge_top_k_lists_capped_device(li[None], ld[None], lg[None], lc[None], k, m, bi, bd, bg, bc)

            v = dict(new=timed(new, args.reps, args.warmup))
            st = ix.last_stats()
            v.update(emitted_per_query=st.n_emitted / nq, n_fallback=int(st.n_fallback),
                     n_exact_direct=int(st.n_exact_direct), n_candidates=int(st.n_candidates),
                     search_path=int(st.search_path), stages=staged(ix, new, 3))
            v["baseline"] = timed(base, args.reps, args.warmup)
            torch.cuda.synchronize()
            v["baseline_short_queries"] = int((bc < k).sum())  # the queries the route answers with fewer than k rows
            v["baseline_rows_equal"] = bool(torch.equal(bi[bc == k], oi[bc == k]))
            # the plain rank of the last kept row of every query
            pos = (d1024[0] == oi[:, k - 1:k]).int().argmax(1) + 1
            found = (d1024[0] == oi[:, k - 1:k]).any(1)
            v.update(last_rank_median=float(pos[found].float().median()) if found.any() else None,
                     last_rank_max_within_1024=int(pos[found].max()) if found.any() else None,
                     last_rank_beyond_1024=int((~found).sum()))
            points[f"k{k}_m{m}"] = v
            print(f"k={k} m={m}: new {v['new']['median_ms']:.3f} ms ({v['new']['min_ms']:.3f}-{v['new']['max_ms']:.3f})  "
                  f"baseline {v['baseline']['median_ms']:.3f} ms ({v['baseline']['min_ms']:.3f}-"
                  f"{v['baseline']['max_ms']:.3f}), short {v['baseline_short_queries']}  emitted/query "
                  f"{v['emitted_per_query']:.0f} fallback {v['n_fallback']} direct {v['n_exact_direct']} last rank "
                  f"median {v['last_rank_median']} beyond 1024: {v['last_rank_beyond_1024']}  stages {v['stages']}",
                  flush=True)
    # one scanned query: the scan, the one-workgroup selection over the table, the finish
    ex = bsr.Index(dim, max_k=256, device=0, flags=bsr.BSR_FLAG_EXACT_ONLY | bsr.BSR_FLAG_PROFILE)
    ex.set_profile(0)
    ex.load(rows)
    del rows
    scanned = {}
    o1 = outs(1, 1000)
    for m in (1, 3, 16):
        def one():
            ex.deep_capped_search_device(qdev, 1, 1000, m, rg, G, o1[0], o1[1], o1[2], out_group=o1[3])

        scanned[f"m{m}"] = dict(table_keys=m * G, **timed(one, 5, 1), stages=staged(ex, one, 2))
        print(f"one scanned query, {m * G} table keys: {scanned[f'm{m}']}", flush=True)
    res = dict(rows=n, dim=dim, queries=nq, groups=G, reps=args.reps, points=points, one_scanned_query=scanned)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
