"""Diagnostic (tooling): the group search's timings for DESIGN.md §23 -- 1M x 768 synthetic rows in 100k
groups (row i in group i % 100000), 1000 queries, k = 10, fetch_k = 64, group_size = 3, everything in
device buffers.  Host clock around calls that end in a device synchronise, warm-up first, the
variants interleaved round by round, medians.
  (a) group_search against collapsed_search, the same arguments;
  (b) on the first --small queries: group_search against collapsed_search + one grouped masked search
      of Q k "queries" with one mask per returned document (the masks built on the host, timed apart);
  (c) the bytes of the rows the fill reads (the sizes of every query's result groups x ld x 4) -- divide
      by the kernel time of k_groups_fill: `rocprofv3 --kernel-trace --output-format csv -d DIR --
      python tools/diag/groups_timing.py --fill-only`, then `--kernel-stats DIR` (no GPU) prints the
      times of the group search's kernels in that trace.
usage: python tools/diag/groups_timing.py [--rounds R] [--small Q] [--fill-only] [--collapsed-only]
       python tools/diag/groups_timing.py --kernel-stats DIR"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "better-search-rag-rust_amd"))
import bsr  # noqa: E402

N, D, G, Q, K, FK, M = 1_000_000, 768, 100_000, 1000, 10, 64, 3


def timed(f):
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_stats(d):
    """Microseconds of every k_groups_* / k_collapse_walk launch in a rocprofv3 kernel trace (csv)."""
    by = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0]
            if "k_groups" in name or "k_collapse_walk" in name:
                by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(json.dumps({n: dict(calls=len(v), median_us=round(statistics.median(v), 2), min_us=round(min(v), 2),
                              max_us=round(max(v), 2)) for n, v in sorted(by.items())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-stats", metavar="DIR", help="no GPU: summarise a rocprofv3 kernel trace")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--small", type=int, default=32)
    ap.add_argument("--fill-only", action="store_true")
    ap.add_argument("--collapsed-only", action="store_true", help="the parent commit's half of (a)")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats)
    dev = torch.device("cuda:0")
    corpus = torch.empty((N, D), dtype=torch.float32, device=dev)
    bsr.synth_uniform(corpus.data_ptr(), 0, N, D, 42)
    qs = torch.empty((Q, D), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qs.data_ptr(), 0, Q, D, 43)
    ix = bsr.Index(D, max_k=256, device=0)
    ix.load(corpus, 0)
    rg = (torch.arange(N, device=dev, dtype=torch.int64) % G).to(torch.int32)

    def buffers(nq, k, m=None):
        shape = (nq, k) if m is None else (nq, k, m)
        return (torch.empty(shape, dtype=torch.int64, device=dev), torch.empty(shape, dtype=torch.float32, device=dev),
                torch.empty(nq, dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.int32, device=dev))

    ci, cd, cc, cg = buffers(Q, K)
    gi, gd, gc, gg = buffers(Q, K, M)
    grows = torch.empty((Q, K), dtype=torch.int32, device=dev)

    def collapsed(nq=Q):
        ix.collapsed_search_device(qs, nq, K, FK, rg, G, ci, cd, cc, out_group=cg)

    def groups(nq=Q):
        ix.group_search_device(qs, nq, K, M, FK, rg, G, gi, gd, gc, out_group=gg, out_rows=grows)

    out = {"shape": dict(n=N, dim=D, groups=G, queries=Q, k=K, fetch_k=FK, group_size=M)}
    if a.fill_only:
        for _ in range(5):
            groups()
        sizes = torch.bincount(rg.long(), minlength=G)[gg.long().clamp(0, G - 1)]
        out["fill_rows_read"] = int(sizes.sum())
        out["fill_bytes_read"] = int(sizes.sum()) * D * 4
        print(json.dumps(out))
        return
    variants = {"collapsed": collapsed} if a.collapsed_only else {"collapsed": collapsed, "groups": groups}
    for f in variants.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, f in variants.items():
            ms[name].append(timed(f))
    out["a_ms_median"] = {name: round(statistics.median(v), 3) for name, v in ms.items()}
    out["a_ms_min_max"] = {name: [round(min(v), 3), round(max(v), 3)] for name, v in ms.items()}
    if not a.collapsed_only:
        assert torch.equal(gi[:, :, 0], ci) and torch.equal(gg, cg), "slot [g][0] is not the collapsed head"
        out["search_path"] = int(ix.last_stats().search_path)
        nq = a.small
        words = (N + 63) // 64
        rg_h = rg.cpu().numpy()
        mi, md, mc = (torch.empty((nq * K, M), dtype=t, device=dev) for t in (torch.int64, torch.float32, torch.int32))
        mc = mc[:, 0].contiguous()
        q_rep = qs[:nq].repeat_interleave(K, dim=0).contiguous()
        qm = torch.arange(nq * K, dtype=torch.int32, device=dev)
        tb, ts, tg = [], [], []
        for r in range(a.rounds + 2):
            t0 = time.perf_counter()
            collapsed(nq)
            docs = cg[:nq].cpu().numpy().reshape(-1)
            t1 = time.perf_counter()
            bits = np.packbits(rg_h[None, :] == docs[:, None].astype(rg_h.dtype), axis=1, bitorder="little")
            masks = np.zeros((nq * K, words * 8), np.uint8)
            masks[:, :bits.shape[1]] = bits
            mdev = torch.from_numpy(masks.view(np.uint64).view(np.int64)).to(dev)
            t2 = time.perf_counter()
            ix.local_top_k_grouped_device(q_rep, nq * K, M, mi, md, mc, mdev, qm)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            g_ms = timed(lambda: groups(nq))
            if r >= 2:
                tb.append((t2 - t1) * 1e3)
                ts.append((t1 - t0 + t3 - t2) * 1e3)
                tg.append(g_ms)
        assert torch.equal(mi.view(nq, K, M), gi[:nq]), "the masked searches and the group search differ"
        out["b_batch"] = nq
        out["b_ms_median"] = dict(collapsed_plus_masked=round(statistics.median(ts), 3),
                                  mask_build_host=round(statistics.median(tb), 3), groups=round(statistics.median(tg), 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
