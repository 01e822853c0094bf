#!/usr/bin/env python3
"""Loss expressions on the C2 workload (srhip_eval_loss_expr): srhip/workloads.py c2 --
1024 random trees x 1M rows x 5 features, Float32.  In one process, after a warm-up of every call, the
median wall time of --steps calls (host clock around calls that end in a device synchronise), taken in
turns (a, b, c, a, b, c, ...):

  (a) eval_loss      srhip_eval_loss with the built-in L2DistLoss (fused into the interpreter)
  (b) eval_loss_expr srhip_eval_loss_expr with square(p - t): the prediction launch, predictions left
                     on the device, the loss pass over them
  (c) eval_predict   srhip_eval_predict: the prediction launch and the copy of every prediction to the host

and the loss pass alone (srhip_last_kernel_ms after (b): HIP events around the loss kernel and its finish
kernel) with the bytes it must read, live trees x rows x 4 B of predictions, over that time, beside the HBM
peak (MI355X: 8.0 TB/s specified, 6.29 TB/s measured with a float4 copy).  One condition is checked: (b) is
below (c) -- (b) does (c)'s launch and replaces its copy to the host by a pass on the device.  The script
fails without a device.  One JSON object on stdout.

    python scripts/loss_expr_bench.py [--steps 20] [--trees 1024] [--rows 1000000] [--out FILE]
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

HBM_PEAK_SPEC_TBS = 8.0
HBM_PEAK_MEASURED_TBS = 6.29


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
    opts, X, y, trees, nodes, offs = workloads.c2(0, a.trees, a.rows)
    ctx = srhip.get_context(0)
    ds = srhip.DeviceDataset(ctx, X, y)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
    l2 = srhip.L2DistLoss()
    lopts = srhip.Options(binary_operators=("-",), unary_operators=("square",))
    expr = srhip.ExprLoss(srhip.Node("square", srhip.Node(feature=1) - srhip.Node(feature=2)), lopts)
    pass_ms = []

    def run_b():
        out = prog.eval_loss(ds, expr)
        pass_ms.append(ctx.last_kernel_ms())
        return out

    calls = {"a": lambda: prog.eval_loss(ds, l2), "b": run_b, "c": lambda: prog.eval_predict(ds)}
    for _ in range(a.warmup):  # clocks, code objects, buffers
        for f in calls.values():
            f()
    la, oka = calls["a"]()
    lb, okb = calls["b"]()
    live = int(okb.sum())
    both = oka & okb & np.isfinite(la) & np.isfinite(lb)  # (a succeeding tree's loss may overflow to +Inf in both)
    rel = np.abs(la[both] - lb[both]) / np.maximum(np.abs(la[both]), 1e-300)
    same_nonfinite = bool(np.array_equal(np.isfinite(la[oka & okb]), np.isfinite(lb[oka & okb])))
    pass_ms.clear()
    ts = {k: [] for k in calls}
    for _ in range(a.steps):
        for k, f in calls.items():
            t = time.perf_counter()
            f()
            ts[k].append((time.perf_counter() - t) * 1e3)
    med = {k: statistics.median(v) for k, v in ts.items()}
    pm = statistics.median(pass_ms)
    nbytes = live * a.rows * 4
    rec = {
        "workload": f"c2: {a.trees} trees x {a.rows} rows x 5 features, Float32", "steps": a.steps,
        "a_eval_loss_l2_ms": round(med["a"], 3), "b_eval_loss_expr_ms": round(med["b"], 3),
        "c_eval_predict_ms": round(med["c"], 3),
        "min_ms": {k: round(min(v), 3) for k, v in ts.items()},
        "b_over_a": round(med["b"] / med["a"], 2), "b_below_c": bool(med["b"] < med["c"]),
        "loss_pass_ms": round(pm, 4), "loss_pass_min_ms": round(min(pass_ms), 4),
        "live_trees": live, "loss_pass_pred_bytes": nbytes,
        "loss_pass_tb_per_s": round(nbytes / (pm * 1e-3) / 1e12, 3),
        "hbm_peak_tb_per_s": {"spec": HBM_PEAK_SPEC_TBS, "measured_copy": HBM_PEAK_MEASURED_TBS},
        "loss_pass_share_of_measured_hbm_peak": round(nbytes / (pm * 1e-3) / 1e12 / HBM_PEAK_MEASURED_TBS, 3),
        "did_succeed_masks_equal": bool(np.array_equal(oka, okb)),
        "max_rel_diff_expr_vs_builtin": float(rel.max()) if rel.size else 0.0,
        "non_finite_losses_agree": same_nonfinite,
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not rec["b_below_c"]:
        print("FAIL: eval_loss_expr is not below eval_predict: the loss pass is broken", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
