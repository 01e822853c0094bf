#!/usr/bin/env python3
"""Batching-mode constant optimisation: every tree on a minibatch of its own (DESIGN.md 3.5,
srhip_optimize_constants_rowsets).

Float32, 5 features, 100k rows, C2's random trees, 50-row sets drawn with replacement, iterations=8,
nrestarts=2, per-tree seeds.  Per case the median wall time of --runs runs (and their min / max) after at
least 50 ms of warm-up; only the optimiser calls are timed (every run starts from the same constants,
restored outside the timed region):

  loop      K optimize_constants(idx=..., seed=...) calls on K one-tree programs (api.optimize_constants'
            batching-mode form before the one-call entry point)
  rowsets   one optimize_constants_rowsets on the K-tree program

for K in --trees (default 1 4 16 64 256 1024), with a bit-equality check of both forms' outputs, and each
form's optimiser launch rounds (the library's SRHIP_OPTIM_TIMING line, one untimed run).  At the largest K
that line's split of the one call is reported too.  A library without the entry point (SRHIP_LIB = an
older build) runs the loop only.  One JSON object per line on stdout.

    python scripts/rowsets_optim_bench.py [--trees 16 1024] [--runs 7]
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
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


def library_stderr(fn):
    """What the library writes to stderr (file descriptor 2) while fn() runs."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, nargs="*", default=[1, 4, 16, 64, 256, 1024])
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--nrestarts", type=int, default=2)
    a = ap.parse_args()
    kmax = max(a.trees)
    opts, X, y, trees, nodes, offs = workloads.c2(0, kmax, a.rows)
    ctx = srhip.get_context(0)
    ds = srhip.DeviceDataset(ctx, X, y)
    loss = srhip.L2DistLoss()
    rng = np.random.default_rng(11)
    idxs = [rng.integers(0, a.rows, size=a.batch_size) for _ in range(kmax)]
    seeds = [int(s) for s in rng.integers(0, 2 ** 63 - 1, size=kmax)]
    kw = dict(iterations=a.iterations, nrestarts=a.nrestarts)
    has_entry = hasattr(srhip._lib.load(), "srhip_optimize_constants_rowsets")
    singles = [srhip.Program(ctx, nodes[offs[t]:offs[t + 1]], np.array([0, offs[t + 1] - offs[t]]), opts, np.float32)
               for t in range(kmax)]
    x0s = [p.get_constants()[0].copy() for p in singles]
    for k in a.trees:
        def loop():
            for t in range(k):
                singles[t].set_constants(x0s[t])
            t0 = time.perf_counter()
            out = [singles[t].optimize_constants(ds, loss, idx=idxs[t], seed=seeds[t], **kw) for t in range(k)]
            dt = time.perf_counter() - t0
            loop.out = [(bits(o[0])[0], bool(o[1][0]), int(o[2][0]), bits(singles[t].get_constants()[0])) for t, o in enumerate(out)]
            return dt

        med, lo, hi = timed(loop, a.runs)
        os.environ["SRHIP_OPTIM_TIMING"] = "1"
        log = library_stderr(loop)
        del os.environ["SRHIP_OPTIM_TIMING"]
        rec = {"case": "optimize", "trees": k, "rows_per_set": a.batch_size, "loop_ms": round(med, 3),
               "loop_min_ms": round(lo, 3), "loop_max_ms": round(hi, 3),
               "loop_launch_rounds": sum(int(n) for n in re.findall(r"(\d+) launches", log))}
        if has_entry:
            prog = srhip.Program(ctx, nodes[:offs[k]], offs[:k + 1], opts, np.float32)
            x0 = np.concatenate(x0s[:k]) if k else np.zeros(0)

            def one():
                prog.set_constants(x0)
                t0 = time.perf_counter()
                l, imp, fc = prog.optimize_constants_rowsets(ds, loss, idxs[:k], seeds=seeds[:k], **kw)
                dt = time.perf_counter() - t0
                c = prog.get_constants()
                one.out = [(bits(l[t:t + 1])[0], bool(imp[t]), int(fc[t]), bits(c[t])) for t in range(k)]
                return dt

            med1, lo1, hi1 = timed(one, a.runs)
            os.environ["SRHIP_OPTIM_TIMING"] = "1"
            log = library_stderr(one)
            del os.environ["SRHIP_OPTIM_TIMING"]
            rec.update(rowsets_ms=round(med1, 3), rowsets_min_ms=round(lo1, 3), rowsets_max_ms=round(hi1, 3),
                       rowsets_launch_rounds=sum(int(n) for n in re.findall(r"(\d+) launches", log)),
                       speedup=round(med / med1, 2), same_bits=bool(one.out == loop.out),
                       improved=int(sum(o[1] for o in one.out)))
            if k == kmax:
                m = re.search(r"srhip optim rowsets: (.*)", log)
                rec["rowsets_split"] = m.group(1) if m else None
            prog.close()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
