#!/usr/bin/env python3
"""Deep group search timings, tools/bench_deep_cap.py's protocol: a synthetic shard
(default 1M x 768 f32, seed 42), 1000 device queries (seed 43), device outputs, 100k groups (row i in
group i mod 100000: ten rows a group), a host clock around calls that end in the library's wait,
warm-ups, medians with min and max.

Per point (k, m) in {(1000, 3), (257, 3)}: bsr_local_top_groups_deep next to the head search alone
(bsr_local_top_k_deep_capped, per_group = 1, same arguments), alternating in the same rounds -- the
difference is the inverted list, the plan and the fill -- and the fill's rate: the rows of the result
groups x 4 ld bytes over the plan-and-fill time of profile level 2 (rescore_ms of the call minus the
head search's).  Then one query at (1000, 3), which takes the split launch, and (200, 3) against
bsr_local_top_groups(fetch_k = 256) in the same process.

    python tools/bench_deep_groups.py --out profiles/deep_groups_bench.json
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
    rg = (torch.arange(n, device=dev) % G).to(torch.int32)
    gsize = torch.bincount(rg.long(), minlength=G)
    torch.cuda.synchronize()
    ix = bsr.Index(dim, max_k=256, device=0, flags=bsr.BSR_FLAG_PROFILE)
    ix.set_profile(0)
    ix.load(rows)
    del rows
    ld = (dim + 63) // 64 * 64

    def outs(q, k, m):
        e = lambda shape, t: torch.empty(shape, dtype=t, device=dev)
        return (e((q, k, m), torch.int64), e((q, k, m), torch.float32), e((q,), torch.int32), e((q, k), torch.int32),
                e((q, k), torch.int32))

    def timed(fns, reps, warmup):
        """The calls of fns alternating in every round -> one summary each."""
        t = [[] for _ in fns]
        for r in range(warmup + reps):
            for i, fn in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= warmup:
                    t[i].append((time.perf_counter() - t0) * 1e3)
        return [dict(median_ms=statistics.median(x), min_ms=min(x), max_ms=max(x), calls=len(x)) for x in t]

    def rescore_ms(fn, calls=3):
        ix.set_profile(2)
        ix.profile(reset=True)
        for _ in range(calls):
            fn()
        p = ix.profile(reset=True)
        ix.set_profile(0)
        return p.rescore_ms / calls

    def point(q, k, m, reps):
        oi, od, oc, og, orw = outs(q, k, m)
        hi, hd, hc, hg, _ = outs(q, k, 1)

        def groups():
            ix.deep_group_search_device(qdev, q, k, m, rg, G, oi, od, oc, out_group=og, out_rows=orw)

        def heads():
            ix.deep_capped_search_device(qdev, q, k, 1, rg, G, hi, hd, hc, out_group=hg)

        a, b = timed([groups, heads], reps, args.warmup)
        groups()
        path = int(ix.last_stats().search_path)
        torch.cuda.synchronize()
        scored = int(gsize[og[og >= 0].long()].sum())  # the rows of the result groups
        fill_ms = rescore_ms(groups) - rescore_ms(heads)
        v = dict(groups=a, heads=b, difference_ms=a["median_ms"] - b["median_ms"], search_path=path, rows_scored=scored,
                 plan_fill_ms=fill_ms, fill_tb_per_s=scored * 4 * ld / (fill_ms * 1e-3) / 1e12 if fill_ms > 0 else None)
        print(f"q={q} k={k} m={m}: {v}", flush=True)
        return v

    res = dict(rows=n, dim=dim, queries=nq, groups=G, reps=args.reps)
    res["k1000_m3"] = point(nq, 1000, 3, args.reps)
    res["k257_m3"] = point(nq, 257, 3, args.reps)
    res["one_query_k1000_m3"] = point(1, 1000, 3, args.reps)
    # (200, 3): the deep call and the shallow one, the same bytes
    oi, od, oc, og, orw = outs(nq, 200, 3)
    si, sd, sc, sg, srw = outs(nq, 200, 3)
    a, b = timed([lambda: ix.deep_group_search_device(qdev, nq, 200, 3, rg, G, oi, od, oc, out_group=og, out_rows=orw),
                  lambda: ix.group_search_device(qdev, nq, 200, 3, 256, rg, G, si, sd, sc, out_group=sg, out_rows=srw)],
                 args.reps, args.warmup)
    torch.cuda.synchronize()
    res["k200_m3"] = dict(deep=a, shallow_fetch_256=b, equal=bool(torch.equal(oi, si) and torch.equal(orw, srw)))
    print(f"k=200 m=3: {res['k200_m3']}", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
