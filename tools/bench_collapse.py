#!/usr/bin/env python3
"""Collapsed search timings: bsr_local_top_k_collapsed over a synthetic shard (default
1M x 768 f32, seed 42) in groups of 10 consecutive rows, for batches of 1000 queries and of 1 query
(seed 43), k = 10, fetch_k in {32, 64, 256}.  Two group shapes:

  a  no query scans: the uniform queries find 10 groups among their first fetch_k rows;
  b  the same with 1% of the queries (at least one) planted: each is a noisy copy of a row that has
     300 near copies (noise 1e-3) elsewhere in the shard, all in one group, so its candidate list is
     one group at every fetch_k and it takes the group scan.

Each next to, measured in the same run on the same batch and index:
  top    bsr_local_top_k with k = fetch_k, the stage's parent cost;
  host   the host alternative: that call, the read-back of its lists and a numpy collapse; for b also
         its second call with k = 256 for the queries whose first list held fewer than k groups (which
         still cannot prove their answer: the planted lists are one group at 256 too).

One process: per configuration the variants run in blocks, each warmed first and then timed, --reps
repetitions over two passes; the host clock runs around calls that end in the library's own wait.
The walk stage is collapsed(a) - top; the scan's share is collapsed(b) - collapsed(a), reported against
its byte model (rounds * n * ld * 4 bytes, rounds = ceil(scanned queries / 8)).

    python tools/bench_collapse.py --out profiles/collapse_bench.json
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


def host_collapse(idx, dist, cnt, rg, k):
    """The numpy collapse of top-fetch_k lists [Q][F] (local ids): the first occurrence of every
    group per row, the first k of them.  Returns (idx [Q][k] with -1 padding, found [Q])."""
    import numpy as np
    Q, Fk = idx.shape
    valid = np.arange(Fk)[None, :] < cnt[:, None]
    g = np.where(valid, rg[np.where(valid, idx, 0)], -1 - np.arange(Fk)[None, :])  # (padding: groups of their own)
    order = np.argsort(g, axis=1, kind="stable")
    gs = np.take_along_axis(g, order, 1)
    first_sorted = np.ones((Q, Fk), bool)
    first_sorted[:, 1:] = gs[:, 1:] != gs[:, :-1]
    first = np.zeros((Q, Fk), bool)
    np.put_along_axis(first, order, first_sorted, 1)
    first &= valid
    rank = np.cumsum(first, axis=1) - 1
    out = np.full((Q, k), -1, np.int64)
    qq, pp = np.nonzero(first & (rank < k))
    out[qq, rank[qq, pp]] = idx[qq, pp]
    return out, np.minimum(first.sum(axis=1), k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, nargs="+", default=[1000, 1])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fetch-k", type=int, nargs="+", default=[32, 64, 256])
    ap.add_argument("--group-rows", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bsr

    dev = "cuda:0"
    n, dim, k = args.rows, args.dim, args.k
    ld = (dim + 63) // 64 * 64
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(rows.data_ptr(), 0, n, dim, 42)
    nq_max = max(args.queries)
    qall = torch.empty((nq_max, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qall.data_ptr(), 0, nq_max, dim, 43)
    # the planted clusters: for planted query j the row 1000 j + 5, 300 near copies of it at spread
    # rows, all in group n_groups_a + j
    n_plant = max(1, nq_max // 100)
    rg = (np.arange(n, dtype=np.int64) // args.group_rows)
    ng = int(rg.max()) + 1
    gen = torch.Generator(device=dev)
    gen.manual_seed(44)
    rng = np.random.default_rng(45)
    spots = rng.choice(np.arange(n_plant * 1000 + 10, n), (n_plant, 300), replace=False)
    qplant = torch.empty((n_plant, dim), dtype=torch.float32, device=dev)
    for j in range(n_plant):
        r = 1000 * j + 5
        s = torch.from_numpy(spots[j]).to(dev)
        rows[s] = rows[r][None, :] + 1e-3 * torch.randn((300, dim), generator=gen, device=dev)
        qplant[j] = rows[r] + 0.3 * torch.randn((dim,), generator=gen, device=dev)
        rg[r] = rg[spots[j]] = ng + j
    ng += n_plant
    torch.cuda.synchronize()
    ix = bsr.Index(dim, max_k=256, device=0)
    ix.load(rows)
    del rows
    rg32 = rg.astype(np.uint32)
    rg_dev = torch.from_numpy(rg32.view(np.int32)).to(dev)

    def outs(nq, kk):
        return (torch.empty((nq, kk), dtype=torch.int64, device=dev), torch.empty((nq, kk), dtype=torch.float32, device=dev),
                torch.empty((nq,), dtype=torch.int32, device=dev))

    configs = []
    for nq in args.queries:
        for shape in ("a", "b"):
            qdev = qall[:nq].clone()
            n_scan = 0
            if shape == "b":
                n_scan = max(1, nq // 100)
                qdev[:n_scan] = qplant[:n_scan]
            for fk in args.fetch_k:
                otop, ocol = outs(nq, fk), outs(nq, k)
                ogrp = torch.empty((nq, k), dtype=torch.int32, device=dev)
                otop2 = {}
                host_state = {}

                def host_alt():
                    ix.local_top_k_device(qdev, nq, fk, *otop)
                    hi, hc = otop[0].cpu().numpy(), otop[2].cpu().numpy()
                    res, found = host_collapse(hi, None, hc, rg, k)
                    short = np.flatnonzero((found < k) & (hc >= fk))
                    if short.size and fk < 256:
                        # the second call of the alternative: the short queries again at k = 256
                        if short.size not in otop2:
                            otop2[short.size] = outs(short.size, 256)
                        o2 = otop2[short.size]
                        ix.local_top_k_device(qdev[torch.from_numpy(short).to(dev)].contiguous(), short.size, 256, *o2)
                        r2, f2 = host_collapse(o2[0].cpu().numpy(), None, o2[2].cpu().numpy(), rg, k)
                        res[short], found[short] = r2, f2
                    host_state["res"], host_state["found"], host_state["short"] = res, found, short.size

                variants = {
                    "collapsed": lambda: ix.collapsed_search_device(qdev, nq, k, fk, rg_dev, ng, *ocol, out_group=ogrp),
                    "top": lambda: ix.local_top_k_device(qdev, nq, fk, *otop),
                    "host": host_alt,
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
                # the host alternative's rows against the call's, where the alternative found k groups
                ci, cc = ocol[0].cpu().numpy(), ocol[2].cpu().numpy()
                full = host_state["found"] >= k
                agree = bool(np.array_equal(host_state["res"][full], ci[full]))
                med = {name: statistics.median(t) for name, t in times.items()}
                c = dict(queries=nq, shape=shape, k=k, fetch_k=fk, scanned_queries=n_scan,
                         collapsed_ms=med["collapsed"], top_ms=med["top"], host_ms=med["host"],
                         stage_ms=med["collapsed"] - med["top"],
                         collapsed_min_ms=min(times["collapsed"]), collapsed_max_ms=max(times["collapsed"]),
                         top_min_ms=min(times["top"]), top_max_ms=max(times["top"]),
                         host_min_ms=min(times["host"]), host_max_ms=max(times["host"]),
                         host_second_call_queries=int(host_state["short"]),
                         host_queries_short_of_k=int((~full).sum()), host_agrees_where_full=agree,
                         counts_all_k=bool((cc == k).all()),
                         scan_bit=bool(stats["collapsed"]["search_path"] & bsr.BSR_PATH_COLLAPSE_SCAN),
                         collapsed=stats["collapsed"], top=stats["top"])
                configs.append(c)
                print(f"nq {nq:5d} {shape} fetch_k {fk:3d}: collapsed {med['collapsed']:.3f} ms  top-{fk} {med['top']:.3f} ms  "
                      f"host {med['host']:.3f} ms  stage {c['stage_ms']:.3f} ms  scan {c['scan_bit']}  "
                      f"replay {stats['collapsed']['graph_replay']}/{stats['top']['graph_replay']}  "
                      f"host short of k: {c['host_queries_short_of_k']}  agree {agree}", flush=True)
    # the scan's share: b against a, per (nq, fetch_k), against its byte model
    by = {(c["queries"], c["shape"], c["fetch_k"]): c for c in configs}
    for c in configs:
        if c["shape"] != "b":
            continue
        a = by[(c["queries"], "a", c["fetch_k"])]
        rounds = (c["scanned_queries"] + 7) // 8
        c["scan_ms"] = c["collapsed_ms"] - a["collapsed_ms"]
        c["scan_rounds"] = rounds
        c["scan_model_bytes"] = rounds * n * ld * 4
        c["scan_tb_per_s"] = c["scan_model_bytes"] / (c["scan_ms"] * 1e-3) / 1e12 if c["scan_ms"] > 0 else None
        print(f"nq {c['queries']:5d} fetch_k {c['fetch_k']:3d}: scan share {c['scan_ms']:.3f} ms over {rounds} round(s), "
              f"{c['scan_tb_per_s'] or 0:.2f} TB/s of the byte model")
    res = {"rows": n, "dim": dim, "ld": ld, "n_groups": ng, "group_rows": args.group_rows, "reps": args.reps,
           "warmup": args.warmup, "configs": configs}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
