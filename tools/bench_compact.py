#!/usr/bin/env python3
"""Compaction timings: a synthetic shard (default 1M x 768 f32, seed 42, k = 10) with
10 / 50 / 90 / 98 % of its rows deleted at random.  Per point:

  (a) bsr_local_top_k for batches of 1000 and 1 queries on three indexes that alternate in one
      process, in every order in turn: the tombstoned index, the same index after
      bsr_index_compact, and a fresh index loaded with the live rows (the compacted and the fresh
      index must answer bit for bit alike: asserted);
  (b) the wall time of the compaction, without and with BSR_COMPACT_SHRINK (the id map written to
      a device buffer), against the route a caller had before: bsr_index_get_many of the whole
      shard into a device buffer, a device gather of the live rows, bsr_index_load.  Every
      repetition starts from a fresh tombstoned index; the routes alternate;
  (c) the stages of traced compactions (BSR_COMPACT_TRACE=1: host clocks around the call's own
      waits; the median per stage): list + id map, the move, index_finish_load's rebuild.

Everything is warmed first; the host clock runs around calls that end in a device wait.  Prints a
table and writes a JSON with the two comparisons stated as measured.

    python tools/bench_compact.py --out profiles/compact_bench.json
"""
import argparse
import ctypes
import itertools
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "better-search-rag-rust_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

FRACTIONS = [0.1, 0.5, 0.9, 0.98]


def _stderr_of(fn):
    """Run fn with file descriptor 2 redirected; -> what the library wrote there."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tf:
        os.dup2(tf.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        return tf.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1000, 1])
    ap.add_argument("--fractions", type=float, nargs="+", default=FRACTIONS)
    ap.add_argument("--reps", type=int, default=24, help="timed searches per index and batch size")
    ap.add_argument("--fixed-order", action="store_true", help="the same order of the indexes in every repetition")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--compact-reps", type=int, default=5, help="timed compactions per route")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bsr

    dev = "cuda:0"
    L = bsr.lib()
    n, dim, k = args.rows, args.dim, args.k
    rows = torch.empty((n, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(rows.data_ptr(), 0, n, dim, 42)
    qmax = max(args.batches)
    qdev = torch.empty((qmax, dim), dtype=torch.float32, device=dev)
    bsr.synth_uniform(qdev.data_ptr(), 0, qmax, dim, 43)
    torch.cuda.synchronize()

    def check(status):
        if status != 0:
            raise RuntimeError(L.bsr_last_error().decode())

    rng = np.random.default_rng(42)
    searches, compactions, stages = [], [], []
    for frac in args.fractions:
        dead = rng.random(n) < frac
        n_live = int(n - dead.sum())
        dead_ids = torch.from_numpy(np.flatnonzero(dead)).to(dev)
        live_ids = torch.from_numpy(np.flatnonzero(~dead)).to(dev)
        ids_out = torch.empty(n_live, dtype=torch.int64, device=dev)

        def tombstoned():
            ix = bsr.Index(dim, max_k=64, device=0)
            ix.load(rows)
            assert ix.delete(dead_ids) == int(dead.sum())
            return ix

        def compact(ix, shrink):
            cnt = ctypes.c_uint64(0)
            check(L.bsr_index_compact(ix._h, 0, bsr.BSR_COMPACT_SHRINK if shrink else 0, ids_out.data_ptr(), n_live,
                                      ctypes.byref(cnt)))
            assert cnt.value == n_live

        def reload(ix):
            buf = torch.empty((n, dim), dtype=torch.float32, device=dev)
            check(L.bsr_index_get_many(ix._h, 0, n, buf.data_ptr()))
            live_rows = buf.index_select(0, live_ids)
            torch.cuda.synchronize()
            ix.load(live_rows)

        # ---- (a) searches ----
        tomb = tombstoned()
        comp = tombstoned()
        compact(comp, False)
        assert bool((ids_out == live_ids).all())
        fresh = bsr.Index(dim, max_k=64, device=0)
        live_rows = rows.index_select(0, live_ids)
        torch.cuda.synchronize()
        fresh.load(live_rows)
        del live_rows
        index_of = {"tombstones": tomb, "compacted": comp, "fresh": fresh}
        for nq in args.batches:
            out = {name: (torch.zeros((nq, k), dtype=torch.int64, device=dev),
                          torch.zeros((nq, k), dtype=torch.float32, device=dev),
                          torch.zeros(nq, dtype=torch.int32, device=dev)) for name in index_of}

            def run(name):
                t0 = time.perf_counter()
                index_of[name].local_top_k_device(qdev, nq, k, *out[name])
                return (time.perf_counter() - t0) * 1e3

            stats, times = {}, {}
            for name, ix in index_of.items():
                for _ in range(args.warmup):
                    run(name)
                st = ix.last_stats()
                stats[name] = dict(path=int(st.search_path), graph_replay=int(st.graph_replay),
                                   n_rescued=int(st.n_rescued), n_fallback=int(st.n_fallback),
                                   n_exact_direct=int(st.n_exact_direct), n_emitted=int(st.n_emitted),
                                   row_ebound=float(st.row_ebound))
                times[name] = []
            for a, b in zip(out["compacted"], out["fresh"]):  # the same state: the same bits
                assert torch.equal(a, b), (frac, nq)
            for key in ("path", "row_ebound"):
                assert stats["compacted"][key] == stats["fresh"][key], (key, stats["compacted"], stats["fresh"])
            # The indexes alternate, in every order in turn: a search that follows the tombstoned
            # index's finds the caches swept by that search's stream of the whole operand, one that
            # follows a small index's may find its own rows still there (--fixed-order: the first
            # form of this tool, tombstones -> compacted -> fresh in every repetition).
            orders = [tuple(index_of)] if args.fixed_order else list(itertools.permutations(index_of))
            for rep in range(args.reps):
                for name in orders[rep % len(orders)]:
                    times[name].append(run(name))
            lo, hi = min(times["fresh"]), max(times["fresh"])
            for name in index_of:
                t = times[name]
                row = dict(deleted_fraction=frac, nq=nq, variant=name, live=n_live, median_ms=statistics.median(t),
                           min_ms=min(t), max_ms=max(t), reps=len(t), **stats[name])
                if name == "compacted":
                    row["median_inside_fresh_min_max"] = bool(lo <= row["median_ms"] <= hi)
                searches.append(row)
                print(f"deleted={frac:4.0%} nq={nq:5d} {name:11s} live={n_live:8d} median {row['median_ms']:8.3f} ms "
                      f"[{row['min_ms']:.3f}, {row['max_ms']:.3f}] replay={row['graph_replay']} "
                      f"fallback={row['n_fallback']}"
                      + (f" inside fresh [min, max]: {row['median_inside_fresh_min_max']}" if name == "compacted" else ""),
                      flush=True)
        for ix in index_of.values():
            ix.close()
        torch.cuda.empty_cache()

        # ---- (b) the compaction against the reload route ----
        routes = {"compact": lambda ix: compact(ix, False), "compact_shrink": lambda ix: compact(ix, True),
                  "reload": reload}
        times = {name: [] for name in routes}
        for rep in range(args.compact_reps + 1):  # (repetition 0 warms: code objects, the allocators)
            for name, fn in routes.items():
                ix = tombstoned()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(ix)
                dt = (time.perf_counter() - t0) * 1e3
                assert ix.get_count() == ix.live_count() == n_live
                ix.close()
                if rep:
                    times[name].append(dt)
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            row = dict(deleted_fraction=frac, route=name, live=n_live, median_ms=med[name], min_ms=min(t), max_ms=max(t),
                       reps=len(t))
            if name != "reload":
                row["median_not_above_reload"] = bool(med[name] <= med["reload"])
            compactions.append(row)
            print(f"deleted={frac:4.0%} {name:14s} live={n_live:8d} median {med[name]:8.3f} ms "
                  f"[{min(t):.3f}, {max(t):.3f}]"
                  + (f" not above reload: {row['median_not_above_reload']}" if name != "reload" else ""), flush=True)

        # ---- (c) the stages of one compaction ----
        for shrink in (False, True):
            seen = []
            for _ in range(args.compact_reps):
                ix = tombstoned()
                os.environ["BSR_COMPACT_TRACE"] = "1"
                try:
                    text = _stderr_of(lambda: compact(ix, shrink))
                finally:
                    del os.environ["BSR_COMPACT_TRACE"]
                ix.close()
                m = re.search(r"first=(\d+) list_ms=([\d.]+) move_ms=([\d.]+) rebuild_ms=([\d.]+)", text)
                if not m:
                    raise RuntimeError(f"no trace line in: {text!r}")
                seen.append([float(x) for x in m.groups()])
            med = [statistics.median(c) for c in zip(*seen)]  # (per stage, over the traced calls)
            row = dict(deleted_fraction=frac, shrink=shrink, live=n_live, first_moved_row=int(med[0]),
                       list_ms=med[1], move_ms=med[2], rebuild_ms=med[3], traced_calls=len(seen))
            stages.append(row)
            print(f"deleted={frac:4.0%} stages shrink={int(shrink)}: list + ids {row['list_ms']:.3f} ms, move "
                  f"{row['move_ms']:.3f} ms, rebuild {row['rebuild_ms']:.3f} ms", flush=True)
        del dead_ids, live_ids, ids_out
        torch.cuda.empty_cache()

    out = dict(device=torch.cuda.get_device_name(0), rows=n, dim=dim, k=k, reps=args.reps,
               search_order="fixed" if args.fixed_order else "every permutation in turn",
               compact_reps=args.compact_reps, searches=searches, compactions=compactions, stages=stages,
               compacted_median_inside_fresh_min_max_everywhere=all(
                   r["median_inside_fresh_min_max"] for r in searches if r["variant"] == "compacted"),
               compact_median_not_above_reload_everywhere=all(
                   r["median_not_above_reload"] for r in compactions if r["route"] != "reload"))
    print(json.dumps({k_: out[k_] for k_ in ("compacted_median_inside_fresh_min_max_everywhere",
                                             "compact_median_not_above_reload_everywhere")}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
