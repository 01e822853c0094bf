"""The persistent launch's last round in equal shares against whole-block claiming,
on C2 populations over datasets of fewer row blocks than a device has CUs and over the headline's 1M
rows: per configuration the median wall per srhip_eval_loss and the interpreter's kernel time
(probe + persistent launch, device events); losses and masks must be bitwise equal.

  python scripts/tail_balance_sweep.py [--rows 100000,300000,1000000] [--ntrees 1024] [--reps K] > out.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "symbolicregression.jl_amd")]

import srhip  # noqa: E402
from srhip import workloads  # noqa: E402

ENVS = "SRHIP_TAIL_BALANCE=0,default,SRHIP_TAIL_SLICES=32,SRHIP_TAIL_SLICES=128,SRHIP_TAIL_SHARE_ROUNDS=2"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,300000,1000000")
    ap.add_argument("--ntrees", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=41)
    ap.add_argument("--envs", default=ENVS, help="comma-separated NAME=VALUE settings ('default': none)")
    args = ap.parse_args()
    ctx = srhip.get_context(0)
    loss = srhip.L2DistLoss()
    for rows in [int(r) for r in args.rows.split(",")]:
        opts, X, y, trees, nodes, offs = workloads.c2(0, args.ntrees, rows)
        ds = srhip.DeviceDataset(ctx, X, y)
        prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
        ref = None
        for env in args.envs.split(","):
            kv = None if env == "default" else env.split("=", 1)
            if kv:
                os.environ[kv[0]] = kv[1]
            try:
                for _ in range(10):
                    prog.eval_loss(ds, loss)
                walls, kms = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    l, ok = prog.eval_loss(ds, loss)
                    walls.append(time.perf_counter() - t0)
                    kms.append(ctx.last_kernel_ms())
            finally:
                if kv:
                    del os.environ[kv[0]]
            same = None
            if ref is None:
                ref = (l.copy(), ok.copy())
            else:
                same = bool(np.array_equal(ref[0].view(np.uint64), l.view(np.uint64)) and np.array_equal(ref[1], ok))
            print(json.dumps({"rows": rows, "ntrees": args.ntrees, "env": env,
                              "wall_us": 1e6 * float(np.median(walls)), "kernel_us": 1e3 * float(np.median(kms)),
                              "kernel_us_min": 1e3 * float(np.min(kms)), "same_bits": same}), flush=True)
        prog.close()
        ds.close()


if __name__ == "__main__":
    main()
