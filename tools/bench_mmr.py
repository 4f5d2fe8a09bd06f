#!/usr/bin/env python3
"""MMR search timings: bsr_local_top_k_mmr over a synthetic shard (default 1M x 768
f32, seed 42) for batches of 1000 queries and of 1 query (seed 43), k = 10, lambda = 0.5,
fetch_k in {20, 64, 100, 200} -- each next to bsr_local_top_k with k = fetch_k on the same batch
and index, measured in the same run: that call is the stage's parent cost.

One process: per configuration the two variants run in blocks, each warmed first (the plain search
up to its graph replay, which needs the calls before a search to have its shape) and then timed,
--reps repetitions over two passes; the host clock runs around calls that end in the library's own
wait (device queries, device outputs).  The difference of the medians is the MMR stage; it is also
reported as bytes per second of the model k * m * 4 * ld bytes of gathered row reads per query.
Prints the medians and writes a JSON with them.

    python tools/bench_mmr.py --out profiles/mmr_bench.json
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
    ap.add_argument("--queries", type=int, nargs="+", default=[1000, 1])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fetch-k", type=int, nargs="+", default=[20, 64, 100, 200])
    ap.add_argument("--lambda-mult", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bsr

    dev = "cuda:0"
    n, dim, k, lam = args.rows, args.dim, args.k, args.lambda_mult
    ld = (dim + 63) // 64 * 64
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(rows.data_ptr(), 0, n, dim, 42)
    nq_max = max(args.queries)
    qall = torch.empty((nq_max, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qall.data_ptr(), 0, nq_max, dim, 43)
    torch.cuda.synchronize()
    ix = bsr.Index(dim, max_k=max(args.fetch_k), device=0)
    ix.load(rows)
    del rows

    def outs(nq, kk):
        return (torch.empty((nq, kk), dtype=torch.int64, device=dev), torch.empty((nq, kk), dtype=torch.float32, device=dev),
                torch.empty((nq,), dtype=torch.int32, device=dev))

    configs = []
    for nq in args.queries:
        qdev = qall[:nq].contiguous()
        for fk in args.fetch_k:
            otop, ommr = outs(nq, fk), outs(nq, k)
            orank = torch.empty((nq, k), dtype=torch.int32, device=dev)
            variants = {
                "mmr": lambda: ix.mmr_search_device(qdev, nq, k, fk, lam, *ommr, out_rank=orank),
                "top": lambda: ix.local_top_k_device(qdev, nq, fk, *otop),
            }
            times = {name: [] for name in variants}
            stats = {}
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
                    stats[name] = dict(n_fallback=int(st.n_fallback), search_path=int(st.search_path),
                                       graph_replay=int(st.graph_replay))
            torch.cuda.synchronize()
            # the picks against the candidates they were taken from: pick 0 is the top-1, every pick
            # is the candidate at its rank, bit for bit
            ti, td = otop[0].cpu().numpy(), otop[1].cpu().numpy()
            mi, md, mr = ommr[0].cpu().numpy(), ommr[1].cpu().numpy(), orank.cpu().numpy().astype(np.int64)
            agree = bool(np.array_equal(np.take_along_axis(ti, mr, 1), mi) and (mr[:, 0] == 0).all() and
                         np.array_equal(np.take_along_axis(td, mr, 1).view(np.uint32), md.view(np.uint32)))
            med = {name: statistics.median(t) for name, t in times.items()}
            stage_ms = med["mmr"] - med["top"]
            model_bytes = nq * k * fk * 4 * ld
            c = dict(queries=nq, k=k, fetch_k=fk, lambda_mult=lam,
                     mmr_ms=med["mmr"], top_ms=med["top"], stage_ms=stage_ms,
                     mmr_min_ms=min(times["mmr"]), mmr_max_ms=max(times["mmr"]),
                     top_min_ms=min(times["top"]), top_max_ms=max(times["top"]),
                     model_bytes=model_bytes, model_tb_per_s=(model_bytes / (stage_ms * 1e-3) / 1e12) if stage_ms > 0 else None,
                     picks_are_candidates=agree, picks_differ_from_top_k=int((mr != np.arange(k)).any(axis=1).sum()),
                     mmr=stats["mmr"], top=stats["top"])
            configs.append(c)
            rate = f"{c['model_tb_per_s']:.2f} TB/s of the model" if c["model_tb_per_s"] else "-"
            print(f"nq {nq:5d} fetch_k {fk:3d}: mmr {med['mmr']:.3f} ms  top-{fk} {med['top']:.3f} ms  stage {stage_ms:.3f} ms  "
                  f"{rate}  replay {stats['mmr']['graph_replay']}/{stats['top']['graph_replay']} path {stats['mmr']['search_path']}")
    res = {"rows": n, "dim": dim, "ld": ld, "reps": args.reps, "warmup": args.warmup, "configs": configs}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
