#!/usr/bin/env python3
"""Capped search timings: bsr_local_top_k_capped over a synthetic shard (default
1M x 768 f32, seed 42) in groups of 10 consecutive rows, for batches of 1000 queries and of 1 query
(seed 43), k = 10, per_group in {1, 2, 3}, fetch_k in {32, 64}.  tools/bench_collapse.py's protocol
and its two shapes:

  a  no query scans: the uniform queries keep 10 rows among their first fetch_k;
  b  the same with 1% of the queries (at least one) planted: each is a noisy copy of a row that has
     300 near copies (noise 1e-3) elsewhere in the shard, all in one group, so its candidate list is
     one group at every fetch_k, the walk keeps per_group < k rows of it and the query takes the
     capped group scan.

Each next to, measured in the same run on the same batch and index:
  top        bsr_local_top_k with k = fetch_k, the stage's parent cost;
  collapsed  bsr_local_top_k_collapsed, the yardstick of the walk and the scan at per_group = 1
             (the two calls return the same bytes there);
  host       the host alternative as §19 defined it: the top-fetch_k call, the read-back of its
             lists and a numpy pass that caps them; for b also its second call with k = 256 for the
             queries whose first list kept fewer than k rows (which still cannot prove their answer:
             the planted lists are one group at 256 too).

One process: per configuration the variants run in blocks, each warmed first and then timed, --reps
repetitions over two passes; the host clock runs around calls that end in the library's own wait.
The stage is capped(a) - top; the scan's share is capped(b) - capped(a), reported against its byte
model (rounds * n * ld * 4 bytes, rounds = ceil(scanned queries / 8)).

    python tools/bench_cap.py --out profiles/cap_bench.json
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


def host_cap(idx, cnt, rg, k, m):
    """The numpy cap of top-fetch_k lists [Q][F] (local ids): the entries with fewer than m earlier
    entries of their group per row, the first k of them.  Returns (idx [Q][k] with -1 padding,
    kept [Q])."""
    import numpy as np
    Q, Fk = idx.shape
    valid = np.arange(Fk)[None, :] < cnt[:, None]
    g = np.where(valid, rg[np.where(valid, idx, 0)], -1 - np.arange(Fk)[None, :])  # (padding: groups of their own)
    order = np.argsort(g, axis=1, kind="stable")
    gs = np.take_along_axis(g, order, 1)
    start = np.ones((Q, Fk), bool)
    start[:, 1:] = gs[:, 1:] != gs[:, :-1]
    pos = np.broadcast_to(np.arange(Fk)[None, :], (Q, Fk))
    run0 = np.maximum.accumulate(np.where(start, pos, 0), axis=1)  # (where the entry's run of one group starts)
    kept_sorted = pos - run0 < m
    kept = np.zeros((Q, Fk), bool)
    np.put_along_axis(kept, order, kept_sorted, 1)
    kept &= valid
    rank = np.cumsum(kept, axis=1) - 1
    out = np.full((Q, k), -1, np.int64)
    qq, pp = np.nonzero(kept & (rank < k))
    out[qq, rank[qq, pp]] = idx[qq, pp]
    return out, np.minimum(kept.sum(axis=1), k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, nargs="+", default=[1000, 1])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--per-group", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--fetch-k", type=int, nargs="+", default=[32, 64])
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
                for m in args.per_group:
                    otop, ocap, ocol = outs(nq, fk), outs(nq, k), outs(nq, k)
                    gcap = torch.empty((nq, k), dtype=torch.int32, device=dev)
                    gcol = torch.empty((nq, k), dtype=torch.int32, device=dev)
                    otop2 = {}
                    host_state = {}

                    def host_alt():
                        ix.local_top_k_device(qdev, nq, fk, *otop)
                        hi, hc = otop[0].cpu().numpy(), otop[2].cpu().numpy()
                        res, kept = host_cap(hi, hc, rg, k, m)
                        short = np.flatnonzero((kept < k) & (hc >= fk))
                        if short.size and fk < 256:
                            # the second call of the alternative: the short queries again at k = 256
                            if short.size not in otop2:
                                otop2[short.size] = outs(short.size, 256)
                            o2 = otop2[short.size]
                            ix.local_top_k_device(qdev[torch.from_numpy(short).to(dev)].contiguous(), short.size, 256, *o2)
                            r2, f2 = host_cap(o2[0].cpu().numpy(), o2[2].cpu().numpy(), rg, k, m)
                            res[short], kept[short] = r2, f2
                        host_state["res"], host_state["kept"], host_state["short"] = res, kept, short.size

                    variants = {
                        "capped": lambda: ix.capped_search_device(qdev, nq, k, fk, m, rg_dev, ng, *ocap, out_group=gcap),
                        "top": lambda: ix.local_top_k_device(qdev, nq, fk, *otop),
                        "host": host_alt,
                    }
                    if m == 1:
                        variants["collapsed"] = lambda: ix.collapsed_search_device(qdev, nq, k, fk, rg_dev, ng, *ocol,
                                                                                   out_group=gcol)
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
                    # the host alternative's rows against the call's, where the alternative kept k rows
                    ci, cc = ocap[0].cpu().numpy(), ocap[2].cpu().numpy()
                    full = host_state["kept"] >= k
                    agree = bool(np.array_equal(host_state["res"][full], ci[full]))
                    med = {name: statistics.median(t) for name, t in times.items()}
                    c = dict(queries=nq, shape=shape, k=k, per_group=m, fetch_k=fk, scanned_queries=n_scan,
                             capped_ms=med["capped"], top_ms=med["top"], host_ms=med["host"],
                             stage_ms=med["capped"] - med["top"],
                             capped_min_ms=min(times["capped"]), capped_max_ms=max(times["capped"]),
                             top_min_ms=min(times["top"]), top_max_ms=max(times["top"]),
                             host_min_ms=min(times["host"]), host_max_ms=max(times["host"]),
                             host_second_call_queries=int(host_state["short"]),
                             host_queries_short_of_k=int((~full).sum()), host_agrees_where_full=agree,
                             counts_all_k=bool((cc == k).all()),
                             scan_bit=bool(stats["capped"]["search_path"] & bsr.BSR_PATH_CAP_SCAN),
                             capped=stats["capped"], top=stats["top"])
                    if m == 1:
                        same = all(torch.equal(a, b) for a, b in zip(ocap + (gcap,), ocol + (gcol,)))
                        c.update(collapsed_ms=med["collapsed"], collapsed_min_ms=min(times["collapsed"]),
                                 collapsed_max_ms=max(times["collapsed"]), collapsed=stats["collapsed"],
                                 capped_equals_collapsed=bool(same))
                    configs.append(c)
                    print(f"nq {nq:5d} {shape} fetch_k {fk:3d} m {m}: capped {med['capped']:.3f} ms  top-{fk} {med['top']:.3f} ms  "
                          f"host {med['host']:.3f} ms  stage {c['stage_ms']:.3f} ms  scan {c['scan_bit']}  "
                          f"replay {stats['capped']['graph_replay']}/{stats['top']['graph_replay']}  "
                          f"host short of k: {c['host_queries_short_of_k']}  agree {agree}"
                          + (f"  collapsed {med['collapsed']:.3f} ms  same bytes {c['capped_equals_collapsed']}" if m == 1 else ""),
                          flush=True)
    # the scan's share: b against a, per (nq, fetch_k, per_group), against its byte model
    by = {(c["queries"], c["shape"], c["fetch_k"], c["per_group"]): c for c in configs}
    for c in configs:
        if c["shape"] != "b":
            continue
        a = by[(c["queries"], "a", c["fetch_k"], c["per_group"])]
        rounds = (c["scanned_queries"] + 7) // 8
        c["scan_ms"] = c["capped_ms"] - a["capped_ms"]
        c["scan_rounds"] = rounds
        c["scan_model_bytes"] = rounds * n * ld * 4
        c["scan_tb_per_s"] = c["scan_model_bytes"] / (c["scan_ms"] * 1e-3) / 1e12 if c["scan_ms"] > 0 else None
        if "collapsed_ms" in c:
            c["collapsed_scan_ms"] = c["collapsed_ms"] - a["collapsed_ms"]
        print(f"nq {c['queries']:5d} fetch_k {c['fetch_k']:3d} m {c['per_group']}: scan share {c['scan_ms']:.3f} ms over "
              f"{rounds} round(s), {c['scan_tb_per_s'] or 0:.2f} TB/s of the byte model")
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
