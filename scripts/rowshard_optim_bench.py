#!/usr/bin/env python3
"""Row-sharded constant optimisation on the C4 shape (srhip_optimize_constants_sharded).

C4's population (512 fixed-size-20 trees with >= 2 constants, Float64, 5 features, 100k rows), iterations=8,
nrestarts=2, the rows split over the ranks.  A step is one optimize_constants_sharded from the same constants
(restored outside the timed region); reported: the median of --runs steps with their min / max, and from
srhip_comm_stats the exchanges per step and the host ms per exchange.

  world 1      python scripts/rowshard_optim_bench.py
               three GPU steps, each a child process of its own under its own time limit (--step-timeout
               seconds, default 240; a step that exceeds it, or ends on a signal, ends the run: nothing more is
               started on the GPU): the sharded call, optimize_constants with SRHIP_OPTIM_SPLIT=1 -- the mode
               the sharded call equals bit for bit -- and optimize_constants in its default (split) mode.  The
               parent touches no GPU; it compares the steps' outcome digests and prints the merged record.
               --only CASE runs one step in this process (what the children do; a profiler run of one case).
  N ranks      timeout -k 10 300 python -m torch.distributed.run --nproc_per_node N scripts/rowshard_optim_bench.py
               one GPU per rank (LOCAL_RANK), the communicator id broadcast over the process group; the ranks
               are one step, and the time limit is the caller's, around the launcher as shown; every rank
               reports, and checks that all ranks ended with the same constants

One JSON object per line on stdout.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "symbolicregression.jl_amd"))

import srhip  # noqa: E402
from srhip import parallel, workloads  # noqa: E402


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = [fn() * 1e3 for _ in range(runs)]
    return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def digest(out, consts):
    """The outcome of one optimiser call (losses, improved, fcalls) and the constants it left, as one hash."""
    h = hashlib.sha256()
    for a in (bits(out[0]), np.asarray(out[1], np.uint8), np.asarray(out[2], np.int64), bits(consts)):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def run_steps(a):
    """World 1: every case a child process under its own time limit; the merged record."""
    rec = {}
    for case in ("sharded", "split1", "default"):
        cmd = [sys.executable, os.path.abspath(__file__), "--only", case, "--trees", str(a.trees), "--rows", str(a.rows),
               "--runs", str(a.runs), "--warmup", str(a.warmup), "--iterations", str(a.iterations),
               "--nrestarts", str(a.nrestarts)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {case}: no result in {a.step_timeout} s; nothing more is started")
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit(f"step {case}: exit status {r.returncode}; nothing more is started")
        rec[case] = json.loads(lines[-1])
    out = dict(rec["sharded"])
    for case in ("split1", "default"):
        for k in ("ms", "min_ms", "max_ms"):
            out[f"optimize_constants_{case}_{k}"] = rec[case][k]
    out["same_bits_as_split1"] = rec["sharded"]["digest"] == rec["split1"]["digest"]
    out["sharded_minus_split1_ms"] = round(out["ms"] - rec["split1"]["ms"], 3)
    out["sharded_minus_default_ms"] = round(out["ms"] - rec["default"]["ms"], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=512)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--nrestarts", type=int, default=2)
    ap.add_argument("--only", choices=("sharded", "split1", "default"), default=None,
                    help="world 1: run this one step in this process")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="world 1: seconds each GPU step may take")
    a = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 and a.only is None:
        return run_steps(a)
    rank = int(os.environ.get("RANK", "0"))
    device = int(os.environ.get("LOCAL_RANK", "0"))
    opts, X, y, trees, nodes, offs = workloads.c4(a.trees, a.rows)
    ctx = srhip.get_context(device)
    if world > 1:
        import torch
        import torch.distributed as dist

        torch.cuda.set_device(device)
        dist.init_process_group("nccl")
        comm = parallel.NativeComm.from_process_group(ctx)
    else:
        comm = parallel.NativeComm(ctx, 1, 0, parallel.NativeComm.unique_id())
    if a.only in ("split1", "default"):  # a one-device call alone: unsplit (what the sharded call equals), or default
        if a.only == "split1":
            os.environ["SRHIP_OPTIM_SPLIT"] = "1"
        else:
            os.environ.pop("SRHIP_OPTIM_SPLIT", None)
        ds = srhip.DeviceDataset(ctx, X, y)
        prog = srhip.Program(ctx, nodes, offs, opts, np.float64)
        x0 = np.concatenate(prog.get_constants())
        last = {}

        def single():
            prog.set_constants(x0)
            ctx.synchronize()
            t0 = time.perf_counter()
            last["out"] = prog.optimize_constants(ds, srhip.L2DistLoss(), iterations=a.iterations,
                                                  nrestarts=a.nrestarts, seed=7)
            return time.perf_counter() - t0

        m, lo_, hi_ = timed(single, a.runs, a.warmup)
        print(json.dumps({"case": "optimize_constants_" + a.only, "ms": m, "min_ms": lo_, "max_ms": hi_,
                          "digest": digest(last["out"], np.concatenate(prog.get_constants()))}), flush=True)
        comm.close()
        return
    lo, hi = parallel.shard_rows(a.rows, rank, world)
    shard = srhip.DeviceDataset(ctx, np.ascontiguousarray(X[:, lo:hi]), y[lo:hi])
    loss = srhip.L2DistLoss()
    kw = dict(iterations=a.iterations, nrestarts=a.nrestarts, seed=7)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float64)
    x0 = np.concatenate(prog.get_constants())
    last = {}

    def sharded():
        prog.set_constants(x0)
        ctx.synchronize()
        t0 = time.perf_counter()
        last["sharded"] = comm.optimize_constants_sharded(prog, shard, loss, **kw)
        return time.perf_counter() - t0

    for _ in range(a.warmup):
        sharded()
    _, ms0, calls0 = comm.stats()
    ts = [sharded() * 1e3 for _ in range(a.runs)]
    _, ms1, calls1 = comm.stats()
    med, tmin, tmax = round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)
    ex = (calls1 - calls0) / max(1, a.runs)
    rec = {"case": "optimize_constants_sharded", "world": world, "rank": rank, "trees": a.trees, "rows": a.rows,
           "shard_rows": hi - lo, "ms": med, "min_ms": tmin, "max_ms": tmax,
           "exchanges_per_step": round(ex, 1), "ms_per_exchange": round((ms1 - ms0) / max(1, calls1 - calls0), 4),
           "exchange_ms_per_step": round((ms1 - ms0) / max(1, a.runs), 3),
           "improved": int(last["sharded"][1].sum()), "fcalls": int(last["sharded"][2].sum())}
    consts = np.concatenate(prog.get_constants())
    rec["digest"] = digest(last["sharded"], consts)
    if world > 1:
        import torch
        import torch.distributed as dist

        mine = torch.from_numpy(bits(consts).view(np.int64).copy()).cuda()
        got = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(got, mine)
        rec["same_constants_on_all_ranks"] = bool(all(torch.equal(g, got[0]) for g in got))
        print(json.dumps(rec), flush=True)
        dist.barrier()
        comm.close()
        dist.destroy_process_group()
        return
    print(json.dumps(rec), flush=True)
    comm.close()


if __name__ == "__main__":
    main()
