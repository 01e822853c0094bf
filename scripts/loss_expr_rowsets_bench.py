#!/usr/bin/env python3
"""Batching mode under a loss given as an expression: every tree on a minibatch of its own (DESIGN.md 3.8,
srhip_eval_loss_expr_rowsets / srhip_optimize_constants_expr_rowsets).

Float32, 5 features, 100k rows, C2's random trees, 50-row sets drawn with replacement, the loss
abs(p - t)^2.5.  Per case the median wall time (and min / max) after at least 50 ms of warm-up -- 20 runs for
scoring, 7 for the optimiser (iterations=8, nrestarts=2, per-tree seeds; every run starts from the same
constants, restored outside the timed region):

  loop      K one-tree single-idx calls: eval_loss(expr, idx=...) / optimize_constants(expr, idx=..., seed=...)
  rowsets   the one call on the K-tree program

for K in --trees (default 1 4 16 64 256 1024).  The outputs of both forms must be bit-identical before
anything is reported, and at the largest K the one call must be faster than the loop, for scoring and for the
optimiser (exit status 1 otherwise; the ratio is reported, not required).  A library without the entry
points (SRHIP_LIB = an older build) runs the loops only.  One JSON object per line on stdout.

    python scripts/loss_expr_rowsets_bench.py [--trees 16 1024] [--skip-optim]
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
    """fn() returns the seconds it timed itself; (median, min, max) in ms."""
    t0 = time.perf_counter()
    while True:  # at least 50 ms and two calls of warm-up
        fn()
        fn()
        if time.perf_counter() - t0 >= warm_s:
            break
    ts = [fn() * 1e3 for _ in range(runs)]
    return statistics.median(ts), min(ts), max(ts)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, nargs="*", default=[1, 4, 16, 64, 256, 1024])
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--score-runs", type=int, default=20)
    ap.add_argument("--optim-runs", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--nrestarts", type=int, default=2)
    ap.add_argument("--skip-optim", action="store_true")
    a = ap.parse_args()
    kmax = max(a.trees)
    opts, X, y, trees, nodes, offs = workloads.c2(0, kmax, a.rows)
    ctx = srhip.get_context(0)
    ds = srhip.DeviceDataset(ctx, X, y)
    lopts = srhip.Options(binary_operators=("-", "^"), unary_operators=("abs",))
    loss = srhip.ExprLoss(srhip.Node("abs", srhip.Node(feature=1) - srhip.Node(feature=2)) ** 2.5, lopts)
    rng = np.random.default_rng(11)
    idxs = [rng.integers(0, a.rows, size=a.batch_size) for _ in range(kmax)]
    seeds = [int(s) for s in rng.integers(0, 2 ** 63 - 1, size=kmax)]
    kw = dict(iterations=a.iterations, nrestarts=a.nrestarts)
    has_entry = hasattr(srhip._lib.load(), "srhip_eval_loss_expr_rowsets")
    singles = [srhip.Program(ctx, nodes[offs[t]:offs[t + 1]], np.array([0, offs[t + 1] - offs[t]]), opts, np.float32)
               for t in range(kmax)]
    x0s = [p.get_constants()[0].copy() for p in singles]
    failed = False
    for k in a.trees:
        prog = srhip.Program(ctx, nodes[:offs[k]], offs[:k + 1], opts, np.float32) if has_entry else None
        x0 = np.concatenate(x0s[:k])

        # ---- scoring ----
        def score_loop():
            t0 = time.perf_counter()
            out = [singles[t].eval_loss(ds, loss, idx=idxs[t]) for t in range(k)]
            dt = time.perf_counter() - t0
            score_loop.out = [(bits(o[0])[0], bool(o[1][0])) for o in out]
            return dt

        med, lo, hi = timed(score_loop, a.score_runs)
        rec = {"case": "score", "trees": k, "rows_per_set": a.batch_size, "loop_ms": round(med, 3),
               "loop_min_ms": round(lo, 3), "loop_max_ms": round(hi, 3)}
        if has_entry:
            def score_one():
                t0 = time.perf_counter()
                l, ok = prog.eval_loss_rowsets(ds, loss, idxs[:k])
                dt = time.perf_counter() - t0
                score_one.out = [(bits(l[t:t + 1])[0], bool(ok[t])) for t in range(k)]
                return dt

            med1, lo1, hi1 = timed(score_one, a.score_runs)
            if score_one.out != score_loop.out:
                print(json.dumps({"case": "score", "trees": k, "error": "outputs differ"}), flush=True)
                return 1
            rec.update(rowsets_ms=round(med1, 3), rowsets_min_ms=round(lo1, 3), rowsets_max_ms=round(hi1, 3),
                       speedup=round(med / med1, 2), same_bits=True, fallback_trees=ctx.rowsets_fallback_trees(),
                       kernel_ms=round(ctx.last_kernel_ms(), 4))
            if k == kmax and not med1 < med:
                failed = True
        print(json.dumps(rec), flush=True)
        if a.skip_optim:
            continue

        # ---- the optimiser ----
        def optim_loop():
            for t in range(k):
                singles[t].set_constants(x0s[t])
            t0 = time.perf_counter()
            out = [singles[t].optimize_constants(ds, loss, idx=idxs[t], seed=seeds[t], **kw) for t in range(k)]
            dt = time.perf_counter() - t0
            optim_loop.out = [(bits(o[0])[0], bool(o[1][0]), int(o[2][0]), bits(singles[t].get_constants()[0]))
                              for t, o in enumerate(out)]
            return dt

        med, lo, hi = timed(optim_loop, a.optim_runs)
        for t in range(k):
            singles[t].set_constants(x0s[t])
        rec = {"case": "optimize", "trees": k, "rows_per_set": a.batch_size, "loop_ms": round(med, 3),
               "loop_min_ms": round(lo, 3), "loop_max_ms": round(hi, 3)}
        if has_entry:
            def optim_one():
                prog.set_constants(x0)
                t0 = time.perf_counter()
                l, imp, fc = prog.optimize_constants_rowsets(ds, loss, idxs[:k], seeds=seeds[:k], **kw)
                dt = time.perf_counter() - t0
                c = prog.get_constants()
                optim_one.out = [(bits(l[t:t + 1])[0], bool(imp[t]), int(fc[t]), bits(c[t])) for t in range(k)]
                return dt

            med1, lo1, hi1 = timed(optim_one, a.optim_runs)
            if optim_one.out != optim_loop.out:
                print(json.dumps({"case": "optimize", "trees": k, "error": "outputs differ"}), flush=True)
                return 1
            rec.update(rowsets_ms=round(med1, 3), rowsets_min_ms=round(lo1, 3), rowsets_max_ms=round(hi1, 3),
                       speedup=round(med / med1, 2), same_bits=True, improved=int(sum(o[1] for o in optim_one.out)),
                       fallback_trees=ctx.rowsets_fallback_trees())
            if k == kmax and not med1 < med:
                failed = True
        print(json.dumps(rec), flush=True)
        if prog is not None:
            prog.close()
    if failed:
        print(json.dumps({"error": "at %d sets the one call is not faster than the loop" % kmax}), flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
