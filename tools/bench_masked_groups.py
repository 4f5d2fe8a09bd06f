#!/usr/bin/env python3
"""Grouped masked search timings: bsr_local_top_k_masked_groups against the only
way to do the same without it -- a loop of bsr_local_top_k_masked calls, one per mask, each over
that mask's queries -- in one process on one box.  Synthetic shard (default 1M x 768 f32, seed 42,
k = 10), random masks of density rho, the queries dealt to the masks in equal contiguous runs, both
variants in BSR_MASK_AUTO.  Cells (nq, G, rho): (1000, 1, 1/2), (1000, 10, 1/2), (1000, 50, 1/4),
(1000, 50, 1/100), (1000, 1000, 1/1000), (16, 16, 1/4).

Device-resident queries, masks, mask ids and outputs; every shape is warmed first, then --reps
timed repetitions in which the two variants alternate; the host clock runs around calls that end
in the library's own wait.  Prints a table and writes a JSON (median, min, max, the grouped call's
statistics and the loop's summed ones).

    python tools/bench_masked_groups.py --out profiles/masked_groups_bench.json
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

CELLS = [(1000, 1, "1/2", 1 / 2), (1000, 10, "1/2", 1 / 2), (1000, 50, "1/4", 1 / 4), (1000, 50, "1/100", 1 / 100),
         (1000, 1000, "1/1000", 1 / 1000), (16, 16, "1/4", 1 / 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

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
    qmax = max(c[0] for c in CELLS)
    qdev = torch.empty((qmax, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qdev.data_ptr(), 0, qmax, dim, 43)
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
            bits[:n] = (torch.rand(n, generator=gen, device=dev) < rho).to(torch.int64)
            allowed.append(int(bits.sum().item()))
            w[g] = (bits.view(words, 64) << shifts).sum(1)  # (bit 63 wraps into the sign: the same word)
        return w, allowed

    results = []
    for nq, G, rho_name, rho in CELLS:
        w, allowed = packed_masks(G, rho)
        # the queries dealt to the masks in equal contiguous runs: the loop searches slices
        bounds = [g * nq // G for g in range(G + 1)]
        qm = torch.zeros(nq, dtype=torch.int32, device=dev)
        for g in range(G):
            qm[bounds[g]:bounds[g + 1]] = g
        oi = torch.zeros((nq, k), dtype=torch.int64, device=dev)
        od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
        oc = torch.zeros(nq, dtype=torch.int32, device=dev)
        li, ld, lc = torch.zeros_like(oi), torch.zeros_like(od), torch.zeros_like(oc)
        torch.cuda.synchronize()
        stats = {}

        def grouped():
            t0 = time.perf_counter()
            ix.local_top_k_grouped_device(qdev, nq, k, oi, od, oc, w, qm, mask_mode="auto")
            dt = (time.perf_counter() - t0) * 1e3
            st = ix.last_stats()
            stats["grouped"] = dict(path=int(st.search_path), n_fallback=int(st.n_fallback),
                                    n_exact_direct=int(st.n_exact_direct), n_emitted=int(st.n_emitted))
            return dt

        def loop():
            fb = direct = 0
            t0 = time.perf_counter()
            for g in range(G):
                a, b = bounds[g], bounds[g + 1]
                if a == b:
                    continue
                ix.local_top_k_device(qdev[a:b], b - a, k, li[a:b], ld[a:b], lc[a:b], allow_words=w[g], mask_mode="auto")
                st = ix.last_stats()
                fb += int(st.n_fallback)
                direct += int(st.n_exact_direct)
            dt = (time.perf_counter() - t0) * 1e3
            stats["loop"] = dict(n_fallback=fb, n_exact_direct=direct)
            return dt

        variants = [("grouped", grouped), ("loop", loop)]
        for _, fn in variants:
            for _ in range(args.warmup):
                fn()
        same = bool(torch.equal(oi, li) and torch.equal(od.view(torch.int32), ld.view(torch.int32)) and torch.equal(oc, lc))
        times = {name: [] for name, _ in variants}
        for _ in range(args.reps):  # the variants alternate
            for name, fn in variants:
                times[name].append(fn())
        for name, _ in variants:
            t = times[name]
            row = dict(nq=nq, n_masks=G, rho=rho_name, variant=name, allowed_min=min(allowed), allowed_max=max(allowed),
                       median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), reps=len(t),
                       identical_results=same, **stats[name])
            results.append(row)
            print(f"nq={nq:5d} G={G:5d} rho={rho_name:7s} {name:8s} median {row['median_ms']:9.3f} ms  "
                  f"[{row['min_ms']:.3f}, {row['max_ms']:.3f}]  fallback={row['n_fallback']} "
                  f"direct={row['n_exact_direct']} path={row.get('path', '-')} same={same}", flush=True)
        del w
    out = dict(device=torch.cuda.get_device_name(0), rows=n, dim=dim, k=k, reps=args.reps, results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    ix.close()


if __name__ == "__main__":
    main()
