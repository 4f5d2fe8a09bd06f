#!/usr/bin/env python3
"""Masked deep capped search timings: bsr_local_top_k_deep_capped_masked at k = 257
and k = 1000, per_group = 1 and 3, over a synthetic shard (default 1M x 768 f32, seed 42) with 100 000
uniform groups for a batch of 1000 device queries (seed 43), under one mask of rho = 1/100 and under
50 masks of rho = 1/50 (query q takes mask q % 50) through the list scan, and under one mask of rho =
1/2 at k = 257 through the filter rung.  Beside every point, from the same process:
  masked  bsr_local_top_k_deep_masked(k) alone over the same masks -- the price of the cap is the
          difference;
  route   what a caller could do without this call: bsr_local_top_k_deep_masked(k), a gather of the
          rows' groups, bsr_global_top_k_capped on the device -- inexact: `short` is the number of
          queries it answers with fewer rows than the exact call.
The variants run in blocks, each warmed first and then timed, --reps repetitions over two passes, the
host clock around calls that end in the library's own wait.  Afterwards one call of every point with
every stage evented (BSR_FLAG_PROFILE, level 2) gives scan_ms and the list scan's ns per (listed row,
query).  Prints the medians and writes a JSON with them.

    python tools/bench_deep_cap_masked.py --out profiles/deep_cap_masked_bench.json
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bsr

    dev = "cuda:0"
    n, dim, nq, G = args.rows, args.dim, args.queries, args.groups
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(rows.data_ptr(), 0, n, dim, 42)
    qdev = torch.empty((nq, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qdev.data_ptr(), 0, nq, dim, 43)
    torch.cuda.synchronize()
    ix = bsr.Index(dim, max_k=256, device=0, flags=bsr.BSR_FLAG_PROFILE)
    ix.set_profile(0)
    ix.load(rows)
    del rows

    rng = np.random.default_rng(44)
    rg = torch.from_numpy(rng.integers(0, G, n).astype(np.int32)).to(dev)

    def words(masks):
        return torch.from_numpy(bsr.pack_allow_masks(n, masks=masks).view(np.int64)).to(dev)

    # name -> (packed words on the device, query_mask or None, listed rows summed over the queries, mode)
    masks = {}
    for name, rho, mode in (("rho100", 0.01, "list"), ("rho2", 0.5, "filter")):
        m = rng.random((1, n)) < rho
        masks[name] = (words(m), None, int(m.sum()) * nq, mode)
    m50 = rng.random((50, n)) < 0.02
    qm = np.arange(nq, dtype=np.int32) % 50
    masks["g50"] = (words(m50), torch.from_numpy(qm).to(dev), int(sum(m50[g].sum() for g in qm)), "list")

    def outs(k, lists=None):
        shape = (nq, k) if lists is None else (lists, nq, k)
        return (torch.empty(shape, dtype=torch.int64, device=dev), torch.empty(shape, dtype=torch.float32, device=dev),
                torch.empty(shape[:-1], dtype=torch.int32, device=dev), torch.empty(shape, dtype=torch.int32, device=dev))

    variants, counts, outbuf = {}, {}, {}
    for name, (w, q, listed, mode) in masks.items():
        for k in (257,) if name == "rho2" else (257, 1000):
            o, li = outs(k), outs(k, 1)
            variants[f"{name}_k{k}_masked"] = (lambda k=k, w=w, q=q, o=o, mode=mode: ix.deep_search_device(
                qdev, nq, k, o[0], o[1], o[2], allow_words=w, query_mask=q, mask_mode=mode))
            for m in (1, 3):
                variants[f"{name}_k{k}_m{m}"] = (lambda k=k, m=m, w=w, q=q, o=o, mode=mode: ix.deep_capped_search_device(
                    qdev, nq, k, m, rg, G, o[0], o[1], o[2], out_group=o[3], allow_words=w, query_mask=q, mask_mode=mode))

                def route(k=k, m=m, w=w, q=q, o=o, li=li, mode=mode):
                    ix.deep_search_device(qdev, nq, k, li[0][0], li[1][0], li[2][0], allow_words=w, query_mask=q,
                                          mask_mode=mode)
                    li[3][0] = rg[li[0][0].clamp(0, n - 1)]  # (padding slots lie behind the counts)
                    bsr.merge_top_k_lists_capped_device(li[0], li[1], li[3], li[2], k, m, o[0], o[1], o[3], o[2])
                    torch.cuda.synchronize()
                variants[f"{name}_k{k}_m{m}_route"] = route
                outbuf[f"{name}_k{k}_m{m}"] = outbuf[f"{name}_k{k}_m{m}_route"] = o

    stats, times = {}, {name: [] for name in variants}
    passes = 2
    for _ in range(passes):
        for name, fn in variants.items():
            for _ in range(args.warmup):
                fn()
            for _ in range(max(1, args.reps // passes)):
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
            st = ix.last_stats()
            stats[name] = dict(n_emitted=int(st.n_emitted), n_fallback=int(st.n_fallback),
                               n_exact_direct=int(st.n_exact_direct), search_path=int(st.search_path))
    # the counts of every point, and the queries the route answers short of the exact call
    for name, fn in variants.items():
        if name.endswith("_masked"):
            continue
        fn()
        torch.cuda.synchronize()
        oc = outbuf[name][2].clone()
        if name.endswith("_route"):
            stats[name]["short"] = int((oc < counts[name[:-len("_route")]]).sum())
        else:
            counts[name] = oc
            stats[name]["min_count"] = int(oc.min())
    # every stage evented, one call each; the list scan's cost per (listed row, query)
    for name, fn in variants.items():
        if name.endswith("_route"):
            continue
        ix.set_profile(2)
        ix.profile(reset=True)
        fn()
        p = ix.profile(reset=True)
        ix.set_profile(0)
        listed = masks[name.split("_")[0]][2]
        stats[name].update(rescore_ms=p.rescore_ms, scan_ms=p.scan_ms, scan_ns_per_row_query=p.scan_ms * 1e6 / max(1, listed))
    res = {"rows": n, "dim": dim, "queries": nq, "groups": G, "reps": args.reps,
           "listed_rows_per_query": {name: v[2] / nq for name, v in masks.items()},
           "variants": {name: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), calls=len(t), **stats[name])
                        for name, t in times.items()}}
    for name, v in res["variants"].items():
        print(f"{name:24s} median {v['median_ms']:9.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})  "
              f"path {v['search_path']:#x} fallback {v['n_fallback']} direct {v['n_exact_direct']} "
              f"scan {v.get('scan_ms', float('nan')):.3f} ms ns/(row,query) {v.get('scan_ns_per_row_query', float('nan')):.3f} "
              f"short {v.get('short', '-')} min_count {v.get('min_count', '-')}", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
