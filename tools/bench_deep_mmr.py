#!/usr/bin/env python3
"""Deep MMR timings: bsr_local_top_k_deep_mmr at lambda = 0.5 over a synthetic shard
(default 1M x 768 f32, seed 42) for a batch of 1000 device queries (seed 43) with device outputs, at
(fetch_k, k) = (200, 10), (1000, 10), (1000, 50), (1000, 256) and one query at (1000, 10); next to
bsr_local_top_k_mmr at (200, 10) -- the unchanged column-per-pick kernel, whose result must be the
same bytes -- and bsr_local_top_k_deep(1000), the candidate search alone: the selection's time is the
difference.  With every point the pair distances computed (last_mmr_pairs) over the sum of (picks - 1)
* m of the column-per-pick schedule.

--clustered replaces 5 % of the rows by near copies (noise 1e-3) of 1000 seed rows: uniform rows
have D ~ 1 everywhere, the case where the fewest candidates can be left stale.

The host clock runs around calls that end in the library's own wait; medians of --reps calls after
--warmup.

    python tools/bench_deep_mmr.py --out profiles/deep_mmr_bench.json
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--clustered", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import bsr

    dev = "cuda:0"
    n, dim, nq = args.rows, args.dim, args.queries
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(rows.data_ptr(), 0, n, dim, 42)
    if args.clustered:
        g = torch.Generator(device=dev).manual_seed(44)
        where = torch.randperm(n, generator=g, device=dev)[: n // 20]
        seeds = torch.randint(0, n, (1000,), generator=g, device=dev)
        src = rows[seeds[torch.arange(n // 20, device=dev) % 1000]]
        rows[where] = src + 1e-3 * torch.randn((n // 20, dim), generator=g, device=dev)
    qdev = torch.empty((nq, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qdev.data_ptr(), 0, nq, dim, 43)
    if args.clustered:  # (queries near seed rows, so that the clusters are what they find)
        qdev = rows[seeds[torch.arange(nq, device=dev) % 1000]] + 0.3 * torch.randn((nq, dim), generator=g, device=dev)
    torch.cuda.synchronize()
    ix = bsr.Index(dim, max_k=256, device=0)
    ix.load(rows)
    del rows

    def outs(q, k):
        return (torch.empty((q, k), dtype=torch.int64, device=dev), torch.empty((q, k), dtype=torch.float32, device=dev),
                torch.empty((q,), dtype=torch.int32, device=dev))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), calls=len(t))

    res = {"rows": n, "dim": dim, "queries": nq, "lambda": args.lam, "clustered": args.clustered, "points": {}}
    o1000 = outs(nq, 1000)
    res["deep1000"] = timed(lambda: ix.deep_search_device(qdev, nq, 1000, *o1000))
    for q, fk, k in ((nq, 200, 10), (nq, 1000, 10), (nq, 1000, 50), (nq, 1000, 256), (1, 1000, 10)):
        o = outs(q, k)
        p = timed(lambda: ix.deep_mmr_search_device(qdev, q, k, fk, args.lam, *o))
        pairs = ix.last_mmr_pairs()
        dense = int(((o[2].clamp(min=1) - 1).to(torch.int64) * fk).sum())  # (m = fetch_k: the shard is deep enough)
        p.update(pairs=pairs, dense_pairs=dense, pairs_ratio=pairs / max(dense, 1))
        if fk <= 256:
            m = outs(q, k)
            p["mmr"] = timed(lambda: ix.mmr_search_device(qdev, q, k, fk, args.lam, *m))
            p["equals_mmr"] = all(torch.equal(a, b) for a, b in zip(o, m))
        res["points"][f"nq{q}_fetch{fk}_k{k}"] = p
        print(f"nq={q} fetch_k={fk} k={k}: {p['median_ms']:.3f} ms (min {p['min_ms']:.3f}, max {p['max_ms']:.3f}); "
              f"pairs {pairs} of {dense} = {p['pairs_ratio']:.3f}" + (f"; mmr {p['mmr']['median_ms']:.3f} ms, equal "
              f"{p['equals_mmr']}" if "mmr" in p else ""), flush=True)
    print(f"deep(1000) alone: {res['deep1000']['median_ms']:.3f} ms", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
