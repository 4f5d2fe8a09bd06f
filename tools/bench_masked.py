#!/usr/bin/env python3
"""Masked search timings: bsr_local_top_k_masked over a synthetic shard (default
1M x 768 f32, seed 42, k = 10) for batches of 1000 and 1 queries and random masks of density rho in
{1, 1/2, 1/4, 1/16, 1/100, 1/1000}, on the list path and the filter path where each applies, with the
unmasked bsr_local_top_k of the same batch as the baseline.

One process: every shape is warmed first, then --reps timed repetitions in which the variants of a
batch size alternate; the host clock runs around calls that end in the library's own wait (device
queries, device mask, device outputs).  Prints a table and writes a JSON (median, min, max, and
the search statistics of each variant).

    python tools/bench_masked.py --out profiles/masked_bench.json
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

RHOS = [("1", 1.0), ("1/2", 0.5), ("1/4", 0.25), ("1/16", 1 / 16), ("1/100", 0.01), ("1/1000", 0.001)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1000, 1])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bsr

    dev = "cuda:0"
    n, dim, k = args.rows, args.dim, args.k
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(rows.data_ptr(), 0, n, dim, 42)
    torch.cuda.synchronize()
    ix = bsr.Index(dim, max_k=64, device=0)
    ix.load(rows)
    del rows
    torch.cuda.empty_cache()
    qmax = max(args.batches)
    qdev = torch.empty((qmax, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qdev.data_ptr(), 0, qmax, dim, 43)
    torch.cuda.synchronize()

    rng = np.random.default_rng(42)
    masks = {}
    for name, rho in RHOS:
        bits = np.ones(n, bool) if rho == 1.0 else rng.random(n) < rho
        w = bsr.pack_allow_mask(n, mask=bits)
        masks[name] = (torch.from_numpy(w.view(np.int64)).to(dev), int(bits.sum()))
    torch.cuda.synchronize()

    results = []
    for nq in args.batches:
        oi = torch.zeros((nq, k), dtype=torch.int64, device=dev)
        od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
        oc = torch.zeros(nq, dtype=torch.int32, device=dev)
        variants = [("unmasked", None, None)]
        for name, _ in RHOS:
            for mode in ("list", "filter", "auto"):
                variants.append((f"{mode} rho={name}", name, mode))

        def run(v):
            _, name, mode = v
            t0 = time.perf_counter()
            if name is None:
                ix.local_top_k_device(qdev, nq, k, oi, od, oc)
            else:
                ix.local_top_k_device(qdev, nq, k, oi, od, oc, allow_words=masks[name][0], mask_mode=mode)
            return (time.perf_counter() - t0) * 1e3

        keep, stats = [], {}
        for v in variants:  # warm every shape; drop a forced filter mode that fell to the list path
            for _ in range(args.warmup):
                run(v)
            st = ix.last_stats()
            took_filter = bool(st.search_path & bsr.BSR_PATH_MASK_FILTER)
            if v[2] == "filter" and not took_filter:
                continue
            keep.append(v)
            stats[v[0]] = dict(path=int(st.search_path), n_fallback=int(st.n_fallback),
                               n_exact_direct=int(st.n_exact_direct), n_emitted=int(st.n_emitted),
                               took_filter=took_filter)
        times = {v[0]: [] for v in keep}
        for _ in range(args.reps):  # the variants alternate
            for v in keep:
                times[v[0]].append(run(v))
        for v in keep:
            t = times[v[0]]
            row = dict(nq=nq, variant=v[0], rho=v[1], mode=v[2], allowed=masks[v[1]][1] if v[1] else n,
                       median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), reps=len(t), **stats[v[0]])
            results.append(row)
            print(f"nq={nq:5d} {v[0]:20s} A={row['allowed']:8d} median {row['median_ms']:9.3f} ms  "
                  f"[{row['min_ms']:.3f}, {row['max_ms']:.3f}]  filter={row['took_filter']} "
                  f"fallback={row['n_fallback']}", flush=True)
    name = torch.cuda.get_device_name(0)
    out = dict(device=name, rows=n, dim=dim, k=k, reps=args.reps, results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    ix.close()


if __name__ == "__main__":
    main()
