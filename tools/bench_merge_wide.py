#!/usr/bin/env python3
"""Wide device merge timings: bsr_global_top_k / bsr_global_top_k_capped with every
array in device memory (k_merge_wide) at (P, nq, k_in, k) = (8, 1000, 1000, 1000) and
(8, 1000, 257, 257), and capped at (8, 1000, 100, 100) with per_group = 3, against the path device
lists had before it: the gathered lists copied to (pinned) host memory, the host merge, and the
result copied back.  The lists are what 8 ranks return: each sorted by distance, U(0.6, 1) with
ties, disjoint index ranges; groups are index mod 1000.

One process: each variant is warmed, then timed --reps times over two alternating passes; the host
clock runs around calls that end in a wait for the device.  The two results are compared once.
Prints the medians and the bytes of list entries the device merge has to read at least once
(12 B an entry, 16 B capped) per second, and writes a JSON with them.

    python tools/bench_merge_wide.py --out profiles/merge_wide_bench.json
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bsr

    dev = "cuda:0"
    rng = np.random.default_rng(46)
    res = {"reps": args.reps, "shapes": {}}
    for name, P, nq, k_in, k, per_group in (("plain_1000", 8, 1000, 1000, 1000, 0), ("plain_257", 8, 1000, 257, 257, 0),
                                            ("capped_100", 8, 1000, 100, 100, 3)):
        ld = np.sort(rng.choice(np.linspace(0.6, 1, 1 << 16, dtype=np.float32), (P, nq, k_in)), axis=2)
        li = rng.integers(0, 1 << 20, (P, nq, k_in)).astype(np.int64) + (np.arange(P, dtype=np.int64) << 20)[:, None, None]
        lg = (li % 1000).astype(np.int32)
        lc = np.full((P, nq), k_in, np.int32)
        d = [torch.from_numpy(x).to(dev) for x in ((li, ld, lg, lc) if per_group else (li, ld, lc))]
        h = [torch.empty(x.shape, dtype=x.dtype).pin_memory() for x in d]
        types = (torch.int64, torch.float32, torch.int32) if per_group else (torch.int64, torch.float32)
        o = [torch.empty((nq, k), dtype=t, device=dev) for t in types] + [torch.empty(nq, dtype=torch.int32, device=dev)]
        o2 = [torch.empty_like(x) for x in o]

        def device():
            if per_group:
                bsr.merge_top_k_lists_capped_device(*d, k, per_group, *o)
            else:
                bsr.merge_top_k_lists_device(*d, k, *o)

        def host():
            for a, b in zip(h, d):
                a.copy_(b)
            n = [x.numpy() for x in h]
            if per_group:
                r = bsr.merge_top_k_lists_capped(n[0].view(np.uint64), n[1], n[2].view(np.uint32), n[3].view(np.uint32),
                                                 k, per_group)
                r = (r[0], r[1], r[2], r[3])
            else:
                r = bsr.merge_top_k_lists(n[0].view(np.uint64), n[1], n[2].view(np.uint32), k)
            for a, b in zip(o2, r):
                a.copy_(torch.from_numpy(b.view(np.int64) if b.dtype == np.uint64 else
                                         b.view(np.int32) if b.dtype == np.uint32 else b))
            torch.cuda.synchronize()

        times = {"device": [], "host": []}
        for _ in range(2):
            for tag, fn in (("device", device), ("host", host)):
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                for _ in range(max(1, args.reps // 2)):
                    t0 = time.perf_counter()
                    fn()
                    times[tag].append((time.perf_counter() - t0) * 1e3)
        equal = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(o, o2))
        entry_bytes = P * nq * k_in * (16 if per_group else 12)
        med = {tag: statistics.median(t) for tag, t in times.items()}
        res["shapes"][name] = dict(P=P, nq=nq, k_in=k_in, k=k, per_group=per_group, equal=equal, entry_bytes=entry_bytes,
                                   device_ms=med["device"], device_min_ms=min(times["device"]),
                                   device_max_ms=max(times["device"]), host_ms=med["host"], host_min_ms=min(times["host"]),
                                   host_max_ms=max(times["host"]), device_gb_per_s=entry_bytes / med["device"] / 1e6)
        print(f"{name:12s} device {med['device']:8.3f} ms  host path {med['host']:8.3f} ms  "
              f"{entry_bytes / med['device'] / 1e6:7.1f} GB/s of entries  equal={equal}", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
