#!/usr/bin/env python3
"""Id scoring timings: bsr_local_score_ids and bsr_local_rerank_ids over a synthetic
shard (default 1M x 768 f32, seed 42) at three points -- 1000 queries x m = 100, 1000 x 256 and
100 x 4096 (scores only) -- against the route a caller had before them, where it can run (m <=
256): bsr_local_top_k_masked_groups with one list-mode allow mask per query and k = m, the packed
bitsets built from the id lists on the device inside the timed call (zero, scatter, synchronise).

Every query's list holds m distinct rows of the shard at a stride coprime to the row count (no two
lists share a start or a stride: a gather without reuse).  One process, device-resident queries,
ids and outputs.  Every variant runs in blocks of its own, warmed first and then timed, --reps
repetitions over two passes so that drift would show; the host clock runs around calls that end in
the library's own wait.  The kernel time of bsr_local_score_ids comes from the index's own events
(BSR_FLAG_PROFILE, level 2) in repetitions of their own, and gives the gathered bytes per second:
n_queries * m * ld * 4 bytes of rows over that time.  Prints a table and writes a JSON.  The
numbers are recorded, not gated.

    python tools/bench_score.py --out profiles/score_bench.json
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "better-search-rag-rust_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

# (nq, m, whether the rerank and the baseline run)
POINTS = [(1000, 100, True), (1000, 256, True), (100, 4096, False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default=None, help="recorded in the JSON (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import bsr

    dev = "cuda:0"
    n, dim = args.rows, args.dim
    ld = (dim + 63) // 64 * 64
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(rows.data_ptr(), 0, n, dim, 42)
    torch.cuda.synchronize()
    ix = bsr.Index(dim, max_k=256, device=0, flags=bsr.BSR_FLAG_PROFILE)
    ix.load(rows)
    del rows
    torch.cuda.empty_cache()
    ix.set_profile(0)
    qmax = max(p[0] for p in POINTS)
    qall = torch.empty((qmax, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qall.data_ptr(), 0, qmax, dim, 43)
    torch.cuda.synchronize()
    words = (n + 63) // 64
    gen = torch.Generator(device="cpu")
    gen.manual_seed(42)

    results = []
    for nq, m, full in POINTS:
        qdev = qall[:nq]
        # list q: start_q + j * step_q mod n, step_q coprime to n -- m distinct rows, scattered
        start = torch.randint(0, n, (nq,), generator=gen, dtype=torch.int64)
        step = torch.randint(1, n, (nq,), generator=gen, dtype=torch.int64)
        step = torch.tensor([next(s for s in range(x, x + n) if math.gcd(s, n) == 1) % n for x in step.tolist()],
                            dtype=torch.int64)
        local = ((start[:, None] + torch.arange(m, dtype=torch.int64)[None, :] * step[:, None]) % n).to(dev)
        assert all(len(set(r)) == m for r in local[:8].tolist())
        ids = local.contiguous()  # (global_offset = 0; int64 holds the same bits as the ABI's u64)
        od = torch.zeros((nq, m), dtype=torch.float32, device=dev)
        of = torch.zeros(nq, dtype=torch.int32, device=dev)
        ri = torch.zeros((nq, m), dtype=torch.int64, device=dev)
        rd = torch.zeros((nq, m), dtype=torch.float32, device=dev)
        rc = torch.zeros(nq, dtype=torch.int32, device=dev)
        stats = {}

        def score():
            t0 = time.perf_counter()
            ix.score_ids_device(qdev, nq, ids, m, od, of)
            dt = (time.perf_counter() - t0) * 1e3
            stats["score_ids"] = int(ix.last_stats().search_path)
            return dt

        def rerank():
            t0 = time.perf_counter()
            ix.rerank_device(qdev, nq, ids, m, m, ri, rd, rc)
            dt = (time.perf_counter() - t0) * 1e3
            stats["rerank"] = int(ix.last_stats().search_path)
            return dt

        variants = [("score_ids", score)]
        if full:
            w = torch.zeros((nq, words), dtype=torch.int64, device=dev)
            qm = torch.arange(nq, dtype=torch.int32, device=dev)
            gi = torch.zeros((nq, m), dtype=torch.int64, device=dev)
            gd = torch.zeros((nq, m), dtype=torch.float32, device=dev)
            gc = torch.zeros(nq, dtype=torch.int32, device=dev)
            one = torch.ones((), dtype=torch.int64, device=dev)

            def grouped():
                t0 = time.perf_counter()
                w.zero_()
                w.scatter_add_(1, ids >> 6, one << (ids & 63))  # (distinct bits: the sum is the OR)
                torch.cuda.synchronize()
                ix.local_top_k_grouped_device(qdev, nq, m, gi, gd, gc, w, qm, mask_mode="list")
                dt = (time.perf_counter() - t0) * 1e3
                stats["grouped_list"] = int(ix.last_stats().search_path)
                return dt

            variants += [("rerank", rerank), ("grouped_list", grouped)]
        times = {name: [] for name, _ in variants}
        passes = 2
        for _ in range(passes):
            for name, fn in variants:
                for _ in range(args.warmup):
                    fn()
                for _ in range(args.reps // passes):
                    times[name].append(fn())
        torch.cuda.synchronize()
        same = None
        if full:  # the three routes agree: the rerank is the baseline's rows, the scores are its distances
            same = bool(torch.equal(ri, gi) and torch.equal(rd.view(torch.int32), gd.view(torch.int32))
                        and torch.equal(rc, gc) and int(of.min()) == m
                        and torch.equal(od.sort(1).values.view(torch.int32), gd.view(torch.int32)))
        # the kernel time of the scores, from the index's own events, in repetitions of their own
        ix.set_profile(2)
        ix.profile(reset=True)
        for _ in range(args.reps // 2):
            ix.score_ids_device(qdev, nq, ids, m, od, of)
        prof = ix.profile(reset=True)
        ix.set_profile(0)
        kernel_ms = prof.rescore_ms / max(prof.rescore_launches, 1)
        gathered = nq * m * ld * 4
        for name, _ in variants:
            t = times[name]
            row = dict(nq=nq, m=m, variant=name, median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t),
                       reps=len(t), search_path=stats[name], identical_results=same)
            if name == "score_ids":
                row.update(kernel_ms=kernel_ms, gathered_bytes=gathered,
                           gathered_tb_per_s_kernel=gathered / (kernel_ms * 1e-3) / 1e12 if kernel_ms else None,
                           gathered_tb_per_s_call=gathered / (row["median_ms"] * 1e-3) / 1e12)
            results.append(row)
            extra = f"  kernel {kernel_ms:.3f} ms, {row['gathered_tb_per_s_kernel']:.3f} TB/s gathered" \
                if name == "score_ids" and kernel_ms else ""
            print(f"nq={nq:5d} m={m:5d} {name:13s} median {row['median_ms']:9.3f} ms  "
                  f"[{row['min_ms']:.3f}, {row['max_ms']:.3f}]  same={same}{extra}", flush=True)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            commit = ""
    res = dict(device=torch.cuda.get_device_name(0), commit=commit or None, rows=n, dim=dim, ld=ld, reps=args.reps,
               warmup=args.warmup, copy_ceiling_tb_per_s=[6.1, 6.3], results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ix.close()


if __name__ == "__main__":
    main()
