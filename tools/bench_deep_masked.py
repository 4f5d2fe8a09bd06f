#!/usr/bin/env python3
"""Masked deep search timings: bsr_local_top_k_deep_masked at k = 257 and k = 1000
over a synthetic shard (default 1M x 768 f32, seed 42) for a batch of 1000 queries (seed 43), under
one mask that allows a fraction rho of the rows (1/100, 1/4, 1/2) and under 50 masks of rho = 1/50
(query q takes mask q % 50), in every mode a point can run: the list scan everywhere, the filter
rung where ks_m = ceil(max(8, k/8) / rho) <= 128, and BSR_MASK_AUTO.  Baselines from the same run:
the unmasked bsr_local_top_k_deep at the same k, and bsr_local_top_k_masked_groups at k = 256 under
the same masks.

One process: the variants run in blocks, each warmed first and then timed, --reps repetitions over
two passes; the host clock runs around calls that end in the library's own wait (device queries,
masks and outputs).  Afterwards one call of every masked variant with every stage evented
(BSR_FLAG_PROFILE, level 2) gives scan_ms, from which the list scan's ns per (listed row, query)
follows, and rescore_ms.  Prints the medians and writes a JSON with them.

    python tools/bench_deep_masked.py --out profiles/deep_masked_bench.json
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bsr

    dev = "cuda:0"
    n, dim, nq = args.rows, args.dim, args.queries
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

    def words(masks):
        return torch.from_numpy(bsr.pack_allow_masks(n, masks=masks).view(np.int64)).to(dev)

    # name -> (packed words [G][words] on the device, query_mask or None, allowed rows per query's mask)
    masks = {}
    for name, rho in (("rho100", 0.01), ("rho4", 0.25), ("rho2", 0.5)):
        m = rng.random((1, n)) < rho
        masks[name] = (words(m), None, [int(m.sum())] * nq)
    m50 = rng.random((50, n)) < 0.02
    qm = np.arange(nq, dtype=np.int32) % 50
    masks["g50"] = (words(m50), torch.from_numpy(qm).to(dev), [int(m50[g].sum()) for g in qm])

    def outs(k):
        return (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
                torch.empty((nq,), dtype=torch.int32, device=dev))

    o = {k: outs(k) for k in (256, 257, 1000)}
    variants = {}
    for k in (257, 1000):
        variants[f"deep{k}"] = lambda k=k: ix.deep_search_device(qdev, nq, k, *o[k])
        for name, (w, q, a) in masks.items():
            live = n
            filt = -(-max(8, -(-k // 8)) * live // max(1, min(a))) <= 128  # (ks_m of the sparsest mask)
            for mode in ("list", "filter", "auto") if filt else ("list", "auto"):
                variants[f"k{k}_{name}_{mode}"] = (lambda k=k, w=w, q=q, mode=mode: ix.deep_search_device(
                    qdev, nq, k, *o[k], allow_words=w, query_mask=q, mask_mode=mode))
    for name, (w, q, a) in masks.items():
        qq = q if q is not None else torch.zeros(nq, dtype=torch.int32, device=dev)
        variants[f"groups256_{name}"] = (lambda w=w, qq=qq: ix.local_top_k_grouped_device(
            qdev, nq, 256, *o[256], w if w.dim() == 2 else w.reshape(1, -1), qq, mask_mode="auto"))

    stats = {}
    times = {name: [] for name in variants}
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
                               n_exact_direct=int(st.n_exact_direct), n_candidates=int(st.n_candidates),
                               search_path=int(st.search_path))
    torch.cuda.synchronize()
    # every stage evented, one call each; the list scan's cost per (listed row, query)
    for name, fn in variants.items():
        ix.set_profile(2)
        ix.profile(reset=True)
        fn()
        p = ix.profile(reset=True)
        ix.set_profile(0)
        stats[name].update(rescore_ms=p.rescore_ms, scan_ms=p.scan_ms, emit_ms=p.gemm_emit_ms, sample_ms=p.gemm_sample_ms,
                           profiled_search_ms=p.search_ms)
        mask = next((m for m in masks if f"_{m}_" in name and name.endswith("_list")), None)
        if mask:
            stats[name]["scan_ns_per_row_query"] = p.scan_ms * 1e6 / max(1, sum(masks[mask][2]))
    res = {
        "rows": n, "dim": dim, "queries": nq, "reps": args.reps,
        "allowed_rows": {name: (min(a), max(a)) for name, (_, _, a) in masks.items()},
        "variants": {name: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), calls=len(t), **stats[name])
                     for name, t in times.items()},
    }
    for name, v in res["variants"].items():
        print(f"{name:22s} median {v['median_ms']:9.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f}, {v['calls']} calls)  "
              f"path {v['search_path']:#x} fallback {v['n_fallback']} direct {v['n_exact_direct']} "
              f"rescore {v['rescore_ms']:.3f} ms scan {v['scan_ms']:.3f} ms "
              f"ns/(row,query) {v.get('scan_ns_per_row_query', float('nan')):.3f}", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
