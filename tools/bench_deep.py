#!/usr/bin/env python3
"""Deep search timings: bsr_local_top_k_deep at k = 257 and k = 1000 over a
synthetic shard (default 1M x 768 f32, seed 42) for a batch of 1000 queries (seed 43), next to two
baselines on the same rows: the same calls on a BSR_FLAG_EXACT_ONLY index (the scan rung alone,
what a caller would otherwise pay) and bsr_local_top_k at k = 200, the deepest filtered search of
the plain entry point.

One process: the variants run in blocks, each warmed first and then timed, --reps repetitions over
two passes; the host clock runs around calls that end in the library's own wait (device queries,
device outputs).  Afterwards a few calls with every stage evented (BSR_FLAG_PROFILE, level 2) give
the time of the rescore + selection (rescore_ms) and of the scan rounds (scan_ms).  Prints the
medians and writes a JSON with them, the emitted keys per query, the fallback counts and the path bits.

    python tools/bench_deep.py --out profiles/deep_bench.json
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
    ap.add_argument("--scan-reps", type=int, default=4, help="repetitions of the EXACT_ONLY calls (seconds each)")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

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
    ex = bsr.Index(dim, max_k=256, device=0, flags=bsr.BSR_FLAG_EXACT_ONLY | bsr.BSR_FLAG_PROFILE)
    ex.set_profile(0)
    ex.load(rows)
    del rows

    def outs(k):
        return (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
                torch.empty((nq,), dtype=torch.int32, device=dev))

    o = {k: outs(k) for k in (200, 257, 1000)}
    oe = {k: outs(k) for k in (257, 1000)}
    variants = {
        "deep257": (ix, args.reps, lambda: ix.deep_search_device(qdev, nq, 257, *o[257])),
        "deep1000": (ix, args.reps, lambda: ix.deep_search_device(qdev, nq, 1000, *o[1000])),
        "top200": (ix, args.reps, lambda: ix.local_top_k_device(qdev, nq, 200, *o[200])),
        "scan257": (ex, args.scan_reps, lambda: ex.deep_search_device(qdev, nq, 257, *oe[257])),
        "scan1000": (ex, args.scan_reps, lambda: ex.deep_search_device(qdev, nq, 1000, *oe[1000])),
    }
    stats = {}
    times = {name: [] for name in variants}
    passes = 2
    for _ in range(passes):
        for name, (index, reps, fn) in variants.items():
            for _ in range(args.warmup if index is ix else 1):
                fn()
            for _ in range(max(1, reps // passes)):
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
            st = index.last_stats()
            stats[name] = dict(n_emitted=int(st.n_emitted), n_fallback=int(st.n_fallback),
                               n_exact_direct=int(st.n_exact_direct), n_candidates=int(st.n_candidates),
                               search_path=int(st.search_path))
    torch.cuda.synchronize()
    # the filtered and the scanned answers are the same bytes
    agree = {k: all(torch.equal(a, b) for a, b in zip(o[k], oe[k])) for k in (257, 1000)}
    # the new kernels' own time: every stage evented, a few calls each
    for name, (index, _, fn) in variants.items():
        if name == "top200":
            continue
        index.set_profile(2)
        index.profile(reset=True)
        calls = 3 if index is ix else 1
        for _ in range(calls):
            fn()
        p = index.profile(reset=True)
        index.set_profile(0)
        stats[name].update(rescore_ms=p.rescore_ms / calls, scan_ms=p.scan_ms / calls, emit_ms=p.gemm_emit_ms / calls,
                           sample_ms=p.gemm_sample_ms / calls, profiled_search_ms=p.search_ms / calls)
    res = {
        "rows": n, "dim": dim, "queries": nq, "reps": args.reps, "scan_reps": args.scan_reps,
        "filtered_equals_scanned": agree, "row_ebound": float(ix.last_stats().row_ebound),
        "variants": {name: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), calls=len(t),
                                emitted_per_query=stats[name]["n_emitted"] / nq, **stats[name])
                     for name, t in times.items()},
    }
    for name, v in res["variants"].items():
        print(f"{name:9s} median {v['median_ms']:.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f}, {v['calls']} calls)  "
              f"emitted/query {v['emitted_per_query']:.1f} fallback {v['n_fallback']} direct {v['n_exact_direct']} "
              f"rescore {v.get('rescore_ms', 0):.3f} ms scan {v.get('scan_ms', 0):.3f} ms", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
