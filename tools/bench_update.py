#!/usr/bin/env python3
"""In-place update timings: bsr_index_update of m random distinct rows of a
synthetic shard (default 1M x 768 f32, seed 42; m = 1, 1,000, 100,000) against the only alternative
without it: bsr_index_load of the whole modified shard from device memory.

One process per shard size; ids and rows are device-resident and complete before the clock starts,
and both calls end in the library's own wait, so the host clock around them is the cost a caller
sees.  Every repetition draws new ids and new rows; the update and the reload of the same modified
shard alternate.  After the last repetition of a point the updated index and the reloaded one must
answer a batch of queries identically (indices and distance bits).  Prints a table and writes a
JSON (median, min, max per point and column, the touched 32-row blocks and sample groups).

    python tools/bench_update.py --out profiles/update_bench.json
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
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--updates", type=int, nargs="+", default=[1, 1_000, 100_000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bsr

    dev = "cuda:0"
    dim, k, nq = args.dim, 10, 40
    rng = np.random.default_rng(42)
    results = []
    for n in args.rows:
        rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
        bsr.synth_uniform(rows.data_ptr(), 0, n, dim, 42)
        qdev = torch.empty((nq, dim), dtype=torch.float32, device=dev)
        bsr.synth_uniform(qdev.data_ptr(), 0, nq, dim, 43)
        torch.cuda.synchronize()
        ix = bsr.Index(dim, max_k=64, device=0)
        ix.load(rows)
        other = bsr.Index(dim, max_k=64, device=0)  # the alternative: reloaded whole
        other.load(rows)
        seed = 1000
        for m in args.updates:
            m = min(m, n)
            new = torch.empty((m, dim), dtype=torch.float32, device=dev)
            t_upd, t_load, blocks, groups = [], [], [], []
            for rep in range(args.warmup + args.reps):
                ids = rng.choice(n, m, replace=False)
                ids_dev = torch.from_numpy(ids).to(dev)
                seed += 1
                bsr.synth_uniform(new.data_ptr(), 0, m, dim, seed)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ix.update(ids_dev, new)
                t1 = time.perf_counter()
                rows.index_copy_(0, ids_dev, new)  # the modified shard, as the caller would hold it
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                other.load(rows)
                t3 = time.perf_counter()
                if rep >= args.warmup:
                    t_upd.append((t1 - t0) * 1e3)
                    t_load.append((t3 - t2) * 1e3)
                    blocks.append(int(np.unique(ids // 32).size))
                    groups.append(int(np.unique(ids[ids % 32 == 0] // 4096).size))
            a = ix.local_top_k(qdev.cpu().numpy(), k)
            b = other.local_top_k(qdev.cpu().numpy(), k)
            same = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))
            row = dict(rows=n, updated=m, reps=len(t_upd), blocks_touched_median=statistics.median(blocks),
                       groups_touched_median=statistics.median(groups), blocks_total=(n + 31) // 32,
                       update_median_ms=statistics.median(t_upd), update_min_ms=min(t_upd), update_max_ms=max(t_upd),
                       reload_median_ms=statistics.median(t_load), reload_min_ms=min(t_load),
                       reload_max_ms=max(t_load), same_answers=same)
            results.append(row)
            print(f"n={n:9d} m={m:7d} blocks={row['blocks_touched_median']:8.0f}/{row['blocks_total']} "
                  f"update {row['update_median_ms']:9.3f} ms [{row['update_min_ms']:.3f}, {row['update_max_ms']:.3f}]  "
                  f"reload {row['reload_median_ms']:9.3f} ms [{row['reload_min_ms']:.3f}, {row['reload_max_ms']:.3f}]  "
                  f"same={same}", flush=True)
            if not same:
                raise SystemExit("the updated index and the reloaded one disagree")
            del new
        ix.close()
        other.close()
        del rows, qdev
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), dim=dim, reps=args.reps, results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
