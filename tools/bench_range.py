#!/usr/bin/env python3
"""Range search timings: bsr_local_range_search over a synthetic shard (default
1M x 768 f32, seed 42) for a batch of 1000 queries (seed 43), radius[q] = the exact distance of
query q's 100th neighbour (taken from a local_top_k(k = 100) call), 256 result slots per query --
next to bsr_local_top_k with k = 10 and k = 100 on the same batch and index.

One process: the variants run in blocks, each warmed first (the plain searches up to their graph
replay, which needs the calls before a search to have its shape) and then timed, --reps
repetitions over two passes; the host clock runs around calls that end in the library's own wait
(device queries, device radii, device outputs).  Prints the medians
and writes a JSON with them, the emitted keys per query, the fallback count and the path bits.

    python tools/bench_range.py --out profiles/range_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "better-search-rag-rust_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--neighbour", type=int, default=100, help="the radius is this neighbour's distance")
    ap.add_argument("--capacity", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bsr

    dev = "cuda:0"
    n, dim, nq, cap = args.rows, args.dim, args.queries, args.capacity
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(rows.data_ptr(), 0, n, dim, 42)
    qdev = torch.empty((nq, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qdev.data_ptr(), 0, nq, dim, 43)
    torch.cuda.synchronize()
    ix = bsr.Index(dim, max_k=max(128, args.neighbour), device=0)
    ix.load(rows)
    del rows

    def outs(k):
        return (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
                torch.empty((nq,), dtype=torch.int32, device=dev))

    o10, o100, orange = outs(10), outs(args.neighbour), outs(cap)
    ix.local_top_k_device(qdev, nq, args.neighbour, *o100)
    radius = o100[1][:, args.neighbour - 1].contiguous()
    torch.cuda.synchronize()

    variants = {
        "range": lambda: ix.range_search_device(qdev, nq, radius, cap, *orange),
        "top10": lambda: ix.local_top_k_device(qdev, nq, 10, *o10),
        f"top{args.neighbour}": lambda: ix.local_top_k_device(qdev, nq, args.neighbour, *o100),
    }
    # Each variant in blocks of its own (a plain search replays its captured graph only when the
    # calls before it had the same shape), two passes over the variants so that drift would show.
    stats = {}
    times = {name: [] for name in variants}
    passes = 2
    for _ in range(passes):
        for name, fn in variants.items():
            for _ in range(args.warmup):
                fn()
            for _ in range(args.reps // passes):
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
            st = ix.last_stats()
            stats[name] = dict(n_emitted=int(st.n_emitted), n_fallback=int(st.n_fallback),
                               n_exact_direct=int(st.n_exact_direct), search_path=int(st.search_path),
                               graph_replay=int(st.graph_replay))
    torch.cuda.synchronize()
    counts = orange[2].cpu().numpy().view(np.uint32)
    # the range result against the top-k it was derived from: the first `neighbour` rows of a query
    # whose count fits are the top-k's, bit for bit
    fits = counts <= cap
    ri, rd = orange[0].cpu().numpy(), orange[1].cpu().numpy()
    ti, td = o100[0].cpu().numpy(), o100[1].cpu().numpy()
    m = args.neighbour
    agree = bool(np.array_equal(ri[fits, :m], ti[fits]) and
                 np.array_equal(rd[fits, :m].view(np.uint32), td[fits].view(np.uint32)))
    res = {
        "rows": n, "dim": dim, "queries": nq, "neighbour": m, "capacity": cap, "reps": args.reps,
        "radius_min": float(radius.min()), "radius_max": float(radius.max()),
        "count_min": int(counts.min()), "count_max": int(counts.max()), "counts_above_capacity": int((~fits).sum()),
        "first_rows_equal_top_k": agree,
        "emitted_per_query": stats["range"]["n_emitted"] / nq,
        "row_ebound": float(ix.last_stats().row_ebound),
        "variants": {name: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), **stats[name])
                     for name, t in times.items()},
    }
    for name, v in res["variants"].items():
        print(f"{name:8s} median {v['median_ms']:.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})  "
              f"emitted/query {v['n_emitted'] / nq:.1f} fallback {v['n_fallback']} path {v['search_path']}")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
