#!/usr/bin/env python3
"""Loss expressions in one launch on the C2 workload (srhip_eval_loss_expr_fused):
srhip/workloads.py c2 -- 1024 random trees x 1M rows x 5 features, Float32 -- under square(p - t) and
abs(p - t)^2.5.  In one process, after a warm-up of every call, the median (and minimum) wall time of --steps
calls, host clock around calls that end in a device synchronise, taken in turns (a, b, c, d, a, b, c, d, ...):

  (a) srhip_eval_loss             the built-in L2DistLoss, fused into the interpreter (the yardstick)
  (b) srhip_eval_loss_expr        the existing two-pass route: prediction launch, host decision, loss pass
  (c) srhip_eval_loss_expr_fused  the one-launch form
  (d) submit / wait               (c) pipelined: three populations submitted behind one another, then waited
                                  for in order; time per population

and a coalescer flush of 24 trees over 100 rows (24 requests queued, one wait) against a loop of 24 one-tree
srhip_eval_loss_expr calls.  Outputs are compared bit for bit: (c) and (d) against (b), every flushed request
against its one-tree call.  One condition is checked: (c) is below (b) and the flush is below the loop -- (b)
is the existing route, not the code under test.  The script fails without a device.  One JSON object on
stdout.

    python scripts/loss_expr_fused_bench.py [--steps 20] [--trees 1024] [--rows 1000000] [--out FILE]
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


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def _same(x, y):
    return bool(np.array_equal(x[1], y[1]) and np.array_equal(_bits(x[0]), _bits(y[0])))


def bench_population(ctx, a, name, expr):
    opts, X, y, trees, nodes, offs = workloads.c2(0, a.trees, a.rows)
    ds = srhip.DeviceDataset(ctx, X, y)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
    l2 = srhip.L2DistLoss()
    kms = {"b": [], "c": []}

    def run_b():
        out = prog.eval_loss(ds, expr)
        kms["b"].append(ctx.last_kernel_ms())
        return out

    def run_c():
        out = prog.eval_loss_fused(ds, expr)
        kms["c"].append(ctx.last_kernel_ms())
        return out

    calls = {"a": lambda: prog.eval_loss(ds, l2), "b": run_b, "c": run_c}
    for _ in range(a.warmup):  # clocks, code objects, buffers
        for f in calls.values():
            f()
        prog.eval_loss_submit(ds, expr).wait()
    ref = calls["b"]()
    same_c = _same(calls["c"](), ref)
    work = ctx.last_work()
    for v in kms.values():
        v.clear()
    ts = {k: [] for k in ("a", "b", "c", "d")}
    same_d = True
    for _ in range(a.steps):
        for k, f in calls.items():
            t = time.perf_counter()
            f()
            ts[k].append((time.perf_counter() - t) * 1e3)
        # (d): three populations queued behind one another, then waited for in order: time per population
        t = time.perf_counter()
        tickets = [prog.eval_loss_submit(ds, expr) for _ in range(3)]
        outs = [tk.wait() for tk in tickets]
        ts["d"].append((time.perf_counter() - t) * 1e3 / 3)
        same_d &= all(_same(o, ref) for o in outs)
    med = {k: statistics.median(v) for k, v in ts.items()}
    rec = {
        "loss": name, "live_trees": int(ref[1].sum()),
        "a_eval_loss_l2_ms": round(med["a"], 3), "b_two_pass_ms": round(med["b"], 3), "c_fused_ms": round(med["c"], 3),
        "d_submit_wait_ms_per_population": round(med["d"], 3),
        "min_ms": {k: round(min(v), 3) for k, v in ts.items()},
        "b_loss_pass_kernel_ms": round(statistics.median(kms["b"]), 4),
        "c_fused_kernel_ms": round(statistics.median(kms["c"]), 4), "c_fused_kernel_min_ms": round(min(kms["c"]), 4),
        "c_over_a": round(med["c"] / med["a"], 2), "b_over_c": round(med["b"] / med["c"], 2),
        "c_bits_equal_b": same_c, "d_bits_equal_b": bool(same_d), "c_below_b": bool(med["c"] < med["b"]),
        "fused_last_work": work,
    }
    prog.close()
    ds.close()
    return rec


def bench_flush(a, expr):
    """24 single-tree requests over 100 rows in one flush against 24 one-tree two-pass calls."""
    opts, X, y, trees, nodes, offs = workloads.c2(0, 24, 100)
    ref_ctx = srhip.Context(0)
    ref_ds = srhip.DeviceDataset(ref_ctx, X, y)
    progs = [srhip.Program(ref_ctx, nodes[offs[i]:offs[i + 1]], np.array([0, offs[i + 1] - offs[i]], np.int64), opts,
                           np.float32) for i in range(24)]
    ctx = srhip.Context(0)
    ds = srhip.DeviceDataset(ctx, X, y)
    co = srhip.Coalescer(ctx, ds, opts, expr, max_batch=24, max_wait_us=100000, nclients=24)

    def loop():
        return [p.eval_loss(ref_ds, expr) for p in progs]

    def flush():
        tk = [co.submit(nodes[offs[i]:offs[i + 1]]) for i in range(24)]
        return [co.wait(t) for t in tk]

    for _ in range(a.warmup):
        loop()
        flush()
    want, got = loop(), flush()
    same = all(bool(w[1][0]) == g[1] and _bits(w[0][0]) == _bits(g[0]) for w, g in zip(want, got))
    before = co.stats()
    ts = {"loop": [], "flush": []}
    for _ in range(a.steps):
        for k, f in (("loop", loop), ("flush", flush)):
            t = time.perf_counter()
            f()
            ts[k].append((time.perf_counter() - t) * 1e3)
    st = co.stats()
    co.close()
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {
        "workload": "24 trees x 100 rows x 5 features, Float32",
        "loop_of_one_tree_two_pass_calls_ms": round(med["loop"], 4), "coalescer_flush_ms": round(med["flush"], 4),
        "min_ms": {k: round(min(v), 4) for k, v in ts.items()},
        "launches_per_flush": (st["launches"] - before["launches"]) / a.steps,
        "loop_over_flush": round(med["loop"] / med["flush"], 2), "bits_equal": bool(same),
        "flush_below_loop": bool(med["flush"] < med["loop"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trees", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps: medians of at least 20 steps")
    lopts = srhip.Options(binary_operators=("-", "^"), unary_operators=("square", "abs"))
    diff = lambda: srhip.Node(feature=1) - srhip.Node(feature=2)  # noqa: E731
    losses = [("square(p - t)", srhip.ExprLoss(srhip.Node("square", diff()), lopts)),
              ("abs(p - t)^2.5", srhip.ExprLoss(srhip.Node("abs", diff()) ** srhip.Node(val=2.5), lopts))]
    ctx = srhip.get_context(0)
    rec = {"workload": f"c2: {a.trees} trees x {a.rows} rows x 5 features, Float32", "steps": a.steps,
           "populations": [bench_population(ctx, a, n, e) for n, e in losses],
           "flush": bench_flush(a, losses[1][1])}
    rec["condition_holds"] = bool(all(p["c_below_b"] for p in rec["populations"]) and rec["flush"]["flush_below_loop"])
    rec["bits_equal"] = bool(all(p["c_bits_equal_b"] and p["d_bits_equal_b"] for p in rec["populations"])
                             and rec["flush"]["bits_equal"])
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not rec["bits_equal"]:
        print("FAIL: the one-launch form's outputs differ from srhip_eval_loss_expr's", file=sys.stderr)
        sys.exit(1)
    if not rec["condition_holds"]:
        print("FAIL: the one-launch form is not below the two-pass route (see the record's counters)", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
