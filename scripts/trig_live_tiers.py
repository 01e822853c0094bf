"""Which leaf body do the cos arguments of C2's LIVE trees take, and what does the quadrant word save?

scripts/trig_arg_tiers.py counts every cos node of the bench population.  A tree that fails (a non-finite
value) leaves the persistent launch at its first failing tile, so this script keeps the trees the oracle
evaluates to the end, and for each of their cos nodes whose argument is an operator output (cos of a
feature is a derived column, computed once per row block) classifies the argument by the device's rule --
a wave's body is chosen by the largest |x| of its 1024-row tile (srhip_eval_impl.h jtrigf_rows):
  A     all |x| < Float32(pi)/4            B    all |x| <= 9pi/4
  C     all |x| < SRM_JQW_MAXF (the quadrant word's range, |fn| < 2^20; before: < 2^28 pi/2)
  slow  the rest: its rows below 2^28 pi/2 take the fast row with the wide word, the others Payne-Hanek
and prints the shares per tile and per 64-row register slot (a slot's own largest |x|: what a finer choice
would see), the slots that take Payne-Hanek, and the predicted drop of the main launch's VALU count:
(2 x tier-B rows + 3 x tier-C rows) / 64 wave instructions per step, cos's saving per row in each tier
(scripts/trig_body_valu.py; 2 more per fast row of a slow tile, printed apart).
python scripts/trig_live_tiers.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "symbolicregression.jl_amd")]
import oracle  # noqa: E402
from srhip import workloads  # noqa: E402
from srhip.node import flatten  # noqa: E402

TILE, SLOT = 1024, 64
PIO4, B_END, C_END, C_END_OLD = np.float32(0.78539819), np.pi * 9 / 4, np.float32(1647098.625), 421657440.0

opts, X, y, trees, nodes, offs = workloads.c2(0, 1024, 1_000_000)
cos_idx = [i + 1 for i, u in enumerate(opts.unary_operators) if u == "cos"][0]


def cos_args(n, out):
    if n.degree == 1:
        op = n.op if isinstance(n.op, int) else opts.unary_operators.index(n.op) + 1
        if op == cos_idx and n.l.degree > 0:
            out.append(n.l)
        cos_args(n.l, out)
    elif n.degree == 2:
        cos_args(n.l, out)
        cos_args(n.r, out)
    return out


def tiers(m):
    """rows -> per group of rows (m: groups x rows) the body index 0..3 (A, B, C, slow) and the old C / slow split"""
    mx = np.max(np.where(np.isnan(m), np.inf, m), axis=1)
    new = np.where(mx < PIO4, 0, np.where(mx <= B_END, 1, np.where(mx < C_END, 2, 3)))
    old_slow = ~(mx < C_END_OLD)
    return new, old_slow


nrows = X.shape[1]
pad = (-nrows) % TILE
live = nargs = 0
tile_rows, slot_rows = np.zeros(4, np.int64), np.zeros(4, np.int64)
old_slow_tile_slots = ph_slots = moved_slots = slow_fast_rows = 0
for t in range(len(trees)):
    _, ok = oracle.eval_tree(nodes[offs[t]:offs[t + 1]], opts.binop_codes, opts.unaop_codes, X)
    if not ok:
        continue
    live += 1
    for a in cos_args(trees[t], []):
        nargs += 1
        nd, _ = flatten([a], opts, np.float32)
        out, _ = oracle.eval_tree(nd, opts.binop_codes, opts.unaop_codes, X)
        m = np.abs(np.concatenate([out, np.zeros(pad, out.dtype)]))
        tt, told = tiers(m.reshape(-1, TILE))
        ss, _ = tiers(m.reshape(-1, SLOT))
        tile_rows += np.bincount(tt, minlength=4) * TILE
        slot_rows += np.bincount(ss, minlength=4) * SLOT
        per_tile = TILE // SLOT
        old_slow_tile_slots += int(told.sum()) * per_tile
        moved_slots += int(((tt == 3) & ~told).sum()) * per_tile
        big = ~(m < C_END_OLD)
        ph_slots += int(big.reshape(-1, SLOT).any(axis=1).sum())
        slow_fast_rows += int((~big).reshape(-1, TILE)[tt == 3].sum())
nslots = tile_rows.sum() // SLOT
print("live trees: %d of %d; cos-of-operator nodes in them: %d; 64-row slots: %d" % (live, len(trees), nargs, nslots))
print("rows by the tile's body   A / B / C / slow: %s  shares %s" % (tile_rows.tolist(), np.round(tile_rows / tile_rows.sum(), 4).tolist()))
print("rows by the slot's own max A / B / C / slow: %s  shares %s" % (slot_rows.tolist(), np.round(slot_rows / slot_rows.sum(), 4).tolist()))
print("slots in tiles that were slow before (a row >= 2^28 pi/2 or non-finite): %d (%.4f %%); slots that take Payne-Hanek: %d (%.4f %%)"
      % (old_slow_tile_slots, 100.0 * old_slow_tile_slots / nslots, ph_slots, 100.0 * ph_slots / nslots))
print("slots of tier C before that now take the slow body (a row >= SRM_JQW_MAXF): %d (%.3f %% of tier C's slots before)"
      % (moved_slots, 100.0 * moved_slots / max(1, moved_slots + tile_rows[2] // SLOT)))
pred = (2 * tile_rows[1] + 3 * tile_rows[2]) / 64
print("predicted VALU drop per step: (2 x %d + 3 x %d) / 64 = %.4g wave instructions (+ %.3g for the slow tiles' fast rows)"
      % (tile_rows[1], tile_rows[2], pred, 2 * slow_fast_rows / 64))
