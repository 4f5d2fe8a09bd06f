#!/usr/bin/env python3
"""Search timings with tombstones: bsr_local_top_k over a synthetic shard (default
1M x 768 f32, seed 42, k = 10) for batches of 1000 and 1 queries with 0 / 10 / 50 / 90 / 98 % of the rows
deleted at random, against the two alternatives a caller has:

    fresh    a second index loaded with the live rows alone (what compaction would give);
    masked   bsr_local_top_k_masked with ~deleted as the allow mask on an index without tombstones.

One process: every shape is warmed first (the plain searches up to their graph replay), then --reps
timed repetitions in which the three variants of a point alternate; the host clock runs around
calls that end in the library's own wait (device queries, device mask, device outputs).  Prints a
table and writes a JSON (median, min, max, the search statistics and the fraction of queries
rescued by the second chance or sent to the exact fallback at each point).

    python tools/bench_deleted.py --out profiles/deleted_bench.json
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

FRACTIONS = [0.0, 0.1, 0.5, 0.9, 0.98]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1000, 1])
    ap.add_argument("--fractions", type=float, nargs="+", default=FRACTIONS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bsr

    dev = "cuda:0"
    n, dim, k = args.rows, args.dim, args.k
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(rows.data_ptr(), 0, n, dim, 42)
    qmax = max(args.batches)
    qdev = torch.empty((qmax, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qdev.data_ptr(), 0, qmax, dim, 43)
    torch.cuda.synchronize()
    plain = bsr.Index(dim, max_k=64, device=0)  # no tombstones: the masked variant's index
    plain.load(rows)

    rng = np.random.default_rng(42)
    results = []
    for frac in args.fractions:
        dead = rng.random(n) < frac
        dead_ids = torch.from_numpy(np.flatnonzero(dead)).to(dev)
        live_ids = torch.from_numpy(np.flatnonzero(~dead)).to(dev)
        tomb = bsr.Index(dim, max_k=64, device=0)
        tomb.load(rows)
        assert tomb.delete(dead_ids) == int(dead.sum())
        fresh = bsr.Index(dim, max_k=64, device=0)
        live_rows = rows.index_select(0, live_ids)
        torch.cuda.synchronize()
        fresh.load(live_rows)
        del live_rows
        allow = torch.from_numpy(bsr.pack_allow_mask(n, mask=~dead).view(np.int64)).to(dev)
        torch.cuda.synchronize()
        for nq in args.batches:
            oi = torch.zeros((nq, k), dtype=torch.int64, device=dev)
            od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
            oc = torch.zeros(nq, dtype=torch.int32, device=dev)

            def run(name):
                t0 = time.perf_counter()
                if name == "tombstones":
                    tomb.local_top_k_device(qdev, nq, k, oi, od, oc)
                elif name == "fresh":
                    fresh.local_top_k_device(qdev, nq, k, oi, od, oc)
                else:
                    plain.local_top_k_device(qdev, nq, k, oi, od, oc, allow_words=allow, mask_mode="auto")
                return (time.perf_counter() - t0) * 1e3

            index_of = {"tombstones": tomb, "fresh": fresh, "masked": plain}
            stats, times = {}, {}
            for name, ix in index_of.items():
                for _ in range(args.warmup):
                    run(name)
                st = ix.last_stats()
                stats[name] = dict(path=int(st.search_path), graph_replay=int(st.graph_replay),
                                   n_rescued=int(st.n_rescued), n_fallback=int(st.n_fallback),
                                   n_exact_direct=int(st.n_exact_direct), n_emitted=int(st.n_emitted),
                                   rescued_fraction=st.n_rescued / nq,
                                   fallback_fraction=(st.n_fallback + st.n_exact_direct) / nq)
                times[name] = []
            for _ in range(args.reps):  # the variants alternate
                for name in index_of:
                    times[name].append(run(name))
            for name in index_of:
                t = times[name]
                row = dict(deleted_fraction=frac, nq=nq, variant=name, live=int(n - dead.sum()),
                           median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), reps=len(t), **stats[name])
                results.append(row)
                print(f"deleted={frac:4.0%} nq={nq:5d} {name:11s} live={row['live']:8d} median "
                      f"{row['median_ms']:8.3f} ms [{row['min_ms']:.3f}, {row['max_ms']:.3f}]  "
                      f"replay={row['graph_replay']} rescued={row['n_rescued']} fallback={row['n_fallback']} "
                      f"direct={row['n_exact_direct']}", flush=True)
        tomb.close()
        fresh.close()
        del allow, dead_ids, live_ids
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), rows=n, dim=dim, k=k, reps=args.reps, results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    plain.close()


if __name__ == "__main__":
    main()
