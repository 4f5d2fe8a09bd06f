#!/usr/bin/env python3
"""Masked range search timings: bsr_local_range_search_masked over a synthetic
shard (default 1M x 768 f32, seed 42), 256 result slots per query, radius[q] = the exact distance of
query q's 100th neighbour WITHIN ITS MASK (taken from a grouped masked top-k with k = 100).

Cells: one mask of density rho in {1, 1/2, 1/4, 1/16, 1/100, 1/1000} at nq = 1000 and nq = 1; 50
masks of 1/4 and 1000 masks of 1/1000 at nq = 1000 (the queries dealt to the masks in equal
contiguous runs).  Variants per cell: the modes `list`, `filter` and `auto`, the unmasked
bsr_local_range_search of the same batch and radii (what a caller filtering on the host would run;
its counts are over every row), and -- more than one mask -- the loop of one `auto` call per mask.

One process, device-resident queries, radii, masks, mask ids and outputs.  Every variant runs in
blocks of its own, warmed first and then timed, --reps repetitions over two passes so that drift
would show; the host clock runs around calls that end in the library's own wait.  Prints a table and
writes a JSON (median, min, max, the statistics of the last call, whether the modes returned
identical rows).  The numbers are recorded, not gated; the one decision they drive is the
BSR_MASK_AUTO rule: `auto` against the better of `list` and `filter`, per cell.

    python tools/bench_range_masked.py --out profiles/range_masked_bench.json
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

RHOS = [("1", 1.0), ("1/2", 1 / 2), ("1/4", 1 / 4), ("1/16", 1 / 16), ("1/100", 1 / 100), ("1/1000", 1 / 1000)]
# (nq, masks, rho)
CELLS = [(nq, 1, name, rho) for nq in (1000, 1) for name, rho in RHOS] + \
        [(1000, 50, "1/4", 1 / 4), (1000, 1000, "1/1000", 1 / 1000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--neighbour", type=int, default=100, help="the radius is this neighbour's distance within the mask")
    ap.add_argument("--capacity", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import bsr

    dev = "cuda:0"
    n, dim, cap, m = args.rows, args.dim, args.capacity, args.neighbour
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(rows.data_ptr(), 0, n, dim, 42)
    torch.cuda.synchronize()
    ix = bsr.Index(dim, max_k=max(128, m), device=0)
    ix.load(rows)
    del rows
    torch.cuda.empty_cache()
    qmax = max(c[0] for c in CELLS)
    qall = torch.empty((qmax, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qall.data_ptr(), 0, qmax, dim, 43)
    torch.cuda.synchronize()

    words = (n + 63) // 64
    gen = torch.Generator(device=dev)
    gen.manual_seed(42)
    shifts = torch.arange(64, dtype=torch.int64, device=dev)

    def packed_masks(G, rho):
        """[G][words] packed masks built on the device (bit i & 63 of word i >> 6), and every A_g."""
        w = torch.zeros((G, words), dtype=torch.int64, device=dev)
        allowed = []
        for g in range(G):
            bits = torch.zeros(words * 64, dtype=torch.int64, device=dev)
            bits[:n] = 1 if rho >= 1 else (torch.rand(n, generator=gen, device=dev) < rho).to(torch.int64)
            allowed.append(int(bits.sum().item()))
            w[g] = (bits.view(words, 64) << shifts).sum(1)  # (bit 63 wraps into the sign: the same word)
        return w, allowed

    results = []
    for nq, G, rho_name, rho in CELLS:
        w, allowed = packed_masks(G, rho)
        qdev = qall[:nq]
        bounds = [g * nq // G for g in range(G + 1)]
        qm = torch.zeros(nq, dtype=torch.int32, device=dev)
        for g in range(G):
            qm[bounds[g]:bounds[g + 1]] = g
        # the radii: every query's m-th neighbour within its mask
        ti = torch.zeros((nq, m), dtype=torch.int64, device=dev)
        td = torch.zeros((nq, m), dtype=torch.float32, device=dev)
        tc = torch.zeros(nq, dtype=torch.int32, device=dev)
        ix.local_top_k_grouped_device(qdev, nq, m, ti, td, tc, w, qm, mask_mode="auto")
        torch.cuda.synchronize()
        assert int(tc.min()) == m, "every mask holds at least `neighbour` rows"
        radius = td[:, m - 1].contiguous()

        def outs():
            return (torch.zeros((nq, cap), dtype=torch.int64, device=dev), torch.zeros((nq, cap), dtype=torch.float32, device=dev),
                    torch.zeros(nq, dtype=torch.int32, device=dev))

        out = {name: outs() for name in ("list", "filter", "auto", "unmasked", "loop")}
        stats = {}

        def keep(name, st):
            stats[name] = dict(path=int(st.search_path), n_fallback=int(st.n_fallback),
                               n_exact_direct=int(st.n_exact_direct), n_emitted=int(st.n_emitted))

        def masked(mode):
            def fn():
                t0 = time.perf_counter()
                ix.range_search_device(qdev, nq, radius, cap, *out[mode], allow_words=w, query_mask=qm if G > 1 else None,
                                       mask_mode=mode)
                dt = (time.perf_counter() - t0) * 1e3
                keep(mode, ix.last_stats())
                return dt
            return fn

        def unmasked():
            t0 = time.perf_counter()
            ix.range_search_device(qdev, nq, radius, cap, *out["unmasked"])
            dt = (time.perf_counter() - t0) * 1e3
            keep("unmasked", ix.last_stats())
            return dt

        def loop():
            oi, od, oc = out["loop"]
            fb = direct = emitted = 0
            t0 = time.perf_counter()
            for g in range(G):
                a, b = bounds[g], bounds[g + 1]
                if a == b:
                    continue
                ix.range_search_device(qdev[a:b], b - a, radius[a:b], cap, oi[a:b], od[a:b], oc[a:b], allow_words=w[g],
                                       mask_mode="auto")
                st = ix.last_stats()
                fb, direct, emitted = fb + int(st.n_fallback), direct + int(st.n_exact_direct), emitted + int(st.n_emitted)
            dt = (time.perf_counter() - t0) * 1e3
            stats["loop"] = dict(n_fallback=fb, n_exact_direct=direct, n_emitted=emitted)
            return dt

        variants = [("list", masked("list")), ("filter", masked("filter")), ("auto", masked("auto")), ("unmasked", unmasked)]
        if G > 1:
            variants.append(("loop", loop))
        times = {name: [] for name, _ in variants}
        passes = 2
        for _ in range(passes):
            for name, fn in variants:
                for _ in range(args.warmup):
                    fn()
                for _ in range(args.reps // passes):
                    times[name].append(fn())
        torch.cuda.synchronize()
        ref = out["list"]
        same = all(bool(torch.equal(out[v][0], ref[0]) and torch.equal(out[v][1].view(torch.int32), ref[1].view(torch.int32))
                        and torch.equal(out[v][2], ref[2])) for v, _ in variants if v != "unmasked")
        counts = ref[2]
        for name, _ in variants:
            t = times[name]
            row = dict(nq=nq, n_masks=G, rho=rho_name, variant=name, allowed_min=min(allowed), allowed_max=max(allowed),
                       median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), reps=len(t),
                       count_min=int(counts.min()), count_max=int(counts.max()), identical_results=same, **stats[name])
            results.append(row)
            print(f"nq={nq:5d} G={G:5d} rho={rho_name:7s} {name:9s} median {row['median_ms']:9.3f} ms  "
                  f"[{row['min_ms']:.3f}, {row['max_ms']:.3f}]  emitted={row['n_emitted']} fallback={row['n_fallback']} "
                  f"direct={row['n_exact_direct']} path={row.get('path', '-')} same={same}", flush=True)
        del w, out
    res = dict(device=torch.cuda.get_device_name(0), rows=n, dim=dim, capacity=cap, neighbour=m, reps=args.reps,
               results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ix.close()


if __name__ == "__main__":
    main()
