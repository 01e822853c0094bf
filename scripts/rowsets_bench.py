#!/usr/bin/env python3
"""Batching-mode scoring: every tree on a minibatch of its own (srhip_eval_loss_rowsets).

Float32, 5 features, 100k rows, C2's random trees, 50-row sets drawn with replacement.  Per case the
median wall time of 20 runs after at least 50 ms of warm-up:

  loop      K eval_loss(idx=...) calls on K one-tree programs (the form before the rowsets call)
  rowsets   one eval_loss_rowsets on the K-tree program (+ the rowsets kernel's srhip_last_kernel_ms)
  coalescer K requests with distinct idx through Coalescer(max_batch=K), submitted from one thread

for K in --sets (default 1 2 3 4 8 16 64 256 1024; the coalescer case at --requests, default 256).
A library without the rowsets entry (SRHIP_LIB = an older build) runs the loop and the coalescer only.
One JSON object per line on stdout.

    python scripts/rowsets_bench.py [--sets 64 1024] [--requests 256] [--runs 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "symbolicregression.jl_amd"))

import srhip  # noqa: E402
from srhip import workloads  # noqa: E402


def timed(fn, runs, warm_s=0.05):
    t0 = time.perf_counter()
    while True:  # at least 50 ms and two calls of warm-up
        fn()
        fn()
        if time.perf_counter() - t0 >= warm_s:
            break
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts) * 1e3, min(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, nargs="*", default=[1, 2, 3, 4, 8, 16, 64, 256, 1024])
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    kmax = max(a.sets + [a.requests])
    opts, X, y, trees, nodes, offs = workloads.c2(0, kmax, a.rows)
    ctx = srhip.get_context(0)
    ds = srhip.DeviceDataset(ctx, X, y)
    loss = srhip.L2DistLoss()
    rng = np.random.default_rng(11)
    idxs = [rng.integers(0, a.rows, size=a.batch_size) for _ in range(kmax)]
    has_rowsets = hasattr(srhip._lib.load(), "srhip_eval_loss_rowsets")
    singles = [srhip.Program(ctx, nodes[offs[t]:offs[t + 1]], np.array([0, offs[t + 1] - offs[t]]), opts, np.float32)
               for t in range(kmax)]
    for k in a.sets:
        def loop():
            return [singles[t].eval_loss(ds, loss, idx=idxs[t]) for t in range(k)]

        med, best = timed(loop, a.runs)
        rec = {"case": "sets", "sets": k, "rows_per_set": a.batch_size, "loop_ms": round(med, 4), "loop_min_ms": round(best, 4)}
        if has_rowsets:
            prog = srhip.Program(ctx, nodes[:offs[k]], offs[:k + 1], opts, np.float32)
            ref = loop()
            got = prog.eval_loss_rowsets(ds, loss, idxs[:k])
            same = all(np.float64(r[0][0]).view(np.uint64) == np.float64(g).view(np.uint64) and bool(r[1][0]) == bool(o)
                       for r, g, o in zip(ref, got[0], got[1]))
            med, best = timed(lambda: prog.eval_loss_rowsets(ds, loss, idxs[:k]), a.runs)
            rec.update(rowsets_ms=round(med, 4), rowsets_min_ms=round(best, 4), rowsets_kernel_ms=round(ctx.last_kernel_ms(), 4),
                       speedup=round(rec["loop_ms"] / med, 2), same_bits=bool(same), trees_ok=int(got[1].sum()))
            prog.close()
        print(json.dumps(rec), flush=True)
    k = a.requests
    co = srhip.Coalescer(ctx, ds, opts, loss, max_batch=k, max_wait_us=2_000_000)

    def flush():
        tickets = [co.submit(nodes[offs[t]:offs[t + 1]], idxs[t]) for t in range(k)]
        return [co.wait(t) for t in tickets]

    med, best = timed(flush, a.runs)
    st = co.stats()
    co.close()
    print(json.dumps({"case": "coalescer", "requests": k, "rows_per_set": a.batch_size, "flush_ms": round(med, 4),
                      "flush_min_ms": round(best, 4), "launches_per_flush": round(st["launches"] / (st["requests"] / k), 2),
                      "rowsets_entry": has_rowsets}), flush=True)


if __name__ == "__main__":
    main()
