#!/usr/bin/env python3
"""Constant optimisation under a loss expression on the C4 shape (512 fixed-size-20 trees x 100k Float64 rows,
8 iterations, 2 restarts), one device, one process:

  (a) Program.optimize_constants with the built-in L2DistLoss                (srhip_optimize_constants)
  (b) Program.optimize_constants with ExprLoss square(p - t)                  (srhip_optimize_constants_expr)
  (c) the route such a loss took before the device gradient existed: api._optimize_constants_host (finite
      differences over eval_loss, one tree at a time) on the first --host-trees trees, reported per tree
  and srhip_last_kernel_ms of one eval_loss_grad launch over the population under L2 and under the expression.

(a) and (b) alternate after a warm-up of each; medians over --steps runs.  Prints one JSON line.

usage: scripts/loss_expr_grad_bench.py [--steps 7] [--warmup 2] [--host-trees 8] [--ntrees 512] [--rows 100000]
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
from srhip import api, workloads  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-trees", type=int, default=8)
    ap.add_argument("--ntrees", type=int, default=512)
    ap.add_argument("--rows", type=int, default=100_000)
    args = ap.parse_args()

    opts, X, y, trees, nodes, offs = workloads.c4(args.ntrees, args.rows)
    ctx = srhip.get_context(0)
    ds = srhip.DeviceDataset(ctx, X, y)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float64)
    x0 = np.concatenate(prog.get_constants())
    p, t = srhip.Node(feature=1), srhip.Node(feature=2)
    lopts = srhip.Options(binary_operators=("-",), unary_operators=("square",))
    losses = {"builtin_l2": srhip.L2DistLoss(), "expr_l2": srhip.ExprLoss(srhip.Node("square", p - t), lopts)}

    def optimise(loss):
        prog.set_constants(x0)
        ctx.synchronize()
        t0 = time.perf_counter()
        out = prog.optimize_constants(ds, loss, iterations=8, nrestarts=2, seed=7)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(args.warmup):
        for loss in losses.values():
            optimise(loss)
    ms = {k: [] for k in losses}
    last = {}
    for _ in range(args.steps):
        for k, loss in losses.items():  # alternated
            dt, last[k] = optimise(loss)
            ms[k].append(dt)
    consts = {}
    for k, loss in losses.items():
        optimise(loss)
        consts[k] = np.concatenate(prog.get_constants())

    # one gradient launch over the population
    prog.set_constants(x0)
    kms = {k: [] for k in losses}
    for _ in range(args.warmup + args.steps):
        for k, loss in losses.items():
            prog.eval_loss_grad(ds, loss)
            kms[k].append(ctx.last_kernel_ms())
    kms = {k: v[args.warmup:] for k, v in kms.items()}

    # (c) the host route on a subset, with the expression as the elementwise loss
    nh = max(0, min(args.host_trees, args.ntrees))
    host_ms = None
    if nh:
        from srhip.options import Options

        hopts = Options(elementwise_loss=losses["expr_l2"], **workloads.C4_OPS)
        dataset = srhip.Dataset(X, y)
        sub = [tr.copy() for tr in trees[:nh]]
        api._optimize_constants_host(dataset, sub[:1], hopts, np.random.default_rng(0), None)  # warm-up
        sub = [tr.copy() for tr in trees[:nh]]
        t0 = time.perf_counter()
        api._optimize_constants_host(dataset, sub, hopts, np.random.default_rng(0), None)
        host_ms = (time.perf_counter() - t0) * 1e3 / nh

    a, b = statistics.median(ms["builtin_l2"]), statistics.median(ms["expr_l2"])
    line = {
        "workload": f"C4: {args.ntrees} trees x {args.rows} rows Float64, 8 iterations, 2 restarts",
        "steps": args.steps, "warmup": args.warmup,
        "a_builtin_l2_ms": a, "a_runs_ms": ms["builtin_l2"],
        "b_expr_l2_ms": b, "b_runs_ms": ms["expr_l2"],
        "b_over_a": b / a,
        "b_per_tree_ms": b / args.ntrees,
        "c_host_route_per_tree_ms": host_ms, "c_trees": nh,
        "same_constants": bool(np.array_equal(consts["builtin_l2"].view(np.uint64), consts["expr_l2"].view(np.uint64))),
        "same_fcalls": bool(np.array_equal(last["builtin_l2"][2], last["expr_l2"][2])),
        "grad_launch_builtin_l2_ms": statistics.median(kms["builtin_l2"]),
        "grad_launch_expr_l2_ms": statistics.median(kms["expr_l2"]),
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
