"""Shared by tests/test_gpu_loss_expr_rowsets.py and tests/test_loss_expr_rowsets_api.py: caps, row sets and
the per-tree loops that the row-set entry points for a loss expression replace."""
import numpy as np

import srhip

import loss_expr_common as X
import loss_expr_grad_common as G
from loss_expr_grad_common import bits, program

LDS_BUDGET = 40 * 1024  # bytes of a set's columns a wave stages (include/srhip.h)
GRAD_RB = 256


def score_cap(dtype, nfeat, weighted):
    """srhip_eval_loss_expr_rowsets' cap, as include/srhip.h states it: whole tiles under the budget."""
    es = np.dtype(dtype).itemsize
    tile = 64 * (8 if es == 4 else 4)
    return LDS_BUDGET // ((nfeat + 1 + (1 if weighted else 0)) * es) // tile * tile


def grad_cap(dtype, nfeat, weighted):
    """srhip_eval_loss_grad_expr_rowsets' cap: whole 256-row blocks, at most 64 of them."""
    return min(score_cap(dtype, nfeat, weighted), 64 * GRAD_RB) // GRAD_RB * GRAD_RB


def lp_expr(weighted=False):
    e = X.N("abs", X.diff()) ** X.C(2.5)
    return srhip.ExprLoss(X.W() * e if weighted else e, X.options())


def draw_sets(rng, n, lengths):
    """One set per length, drawn with replacement."""
    return [rng.integers(0, n, size=int(m)).astype(np.int64) for m in lengths]


def repeated(trees, count):
    return [trees[k % len(trees)].copy() for k in range(count)]


def loop_loss(ctx, trees, dtype, ds, loss, sets, which=None, opts=None):
    """The loop the one call replaces: one-tree Program.eval_loss(ds, loss, idx=set_t)."""
    out = {}
    for t in (range(len(trees)) if which is None else which):
        p = program(ctx, [trees[t]], dtype, opts)
        l, ok = p.eval_loss(ds, loss, idx=sets[t])
        out[t] = (int(bits(l)[0]), bool(ok[0]))
        p.close()
    return out


def loop_grad(ctx, trees, dtype, ds, loss, sets, which=None, opts=None):
    out = {}
    for t in (range(len(trees)) if which is None else which):
        p = program(ctx, [trees[t]], dtype, opts)
        l, g, ok = p.eval_loss_grad(ds, loss, idx=sets[t])
        out[t] = (int(bits(l)[0]), bits(g[0]).tolist(), bool(ok[0]))
        p.close()
    return out


def rowsets_loss(prog, ds, loss, sets, which=None):
    l, ok = prog.eval_loss_rowsets(ds, loss, sets)
    return {t: (int(bits(l)[t]), bool(ok[t])) for t in (range(len(sets)) if which is None else which)}


def rowsets_grad(prog, ds, loss, sets, which=None):
    l, g, ok = prog.eval_loss_grad_rowsets(ds, loss, sets)
    return {t: (int(bits(l)[t]), bits(g[t]).tolist(), bool(ok[t])) for t in (range(len(sets)) if which is None else which)}


def loop_optim(ctx, trees, dtype, ds, loss, sets, seeds, opts=None, **kw):
    """One-tree optimize_constants(loss, idx=set_t, seed=seed_t, return_starts=True) per tree."""
    out = {}
    for t in range(len(trees)):
        p = program(ctx, [trees[t]], dtype, opts)
        l, imp, fc, st = p.optimize_constants(ds, loss, idx=sets[t], seed=seeds[t], return_starts=True, **kw)
        out[t] = (int(bits(l)[0]), bool(imp[0]), int(fc[0]), bits(p.get_constants()[0]).tolist(), bits(st).ravel().tolist())
        p.close()
    return out


def rowsets_optim(prog, ds, loss, sets, seeds, **kw):
    l, imp, fc, st = prog.optimize_constants_rowsets(ds, loss, sets, seeds=seeds, return_starts=True, **kw)
    consts = prog.get_constants()
    co = np.concatenate([[0], np.cumsum([len(c) for c in consts])]).astype(int)
    return {t: (int(bits(l)[t]), bool(imp[t]), int(fc[t]), bits(consts[t]).tolist(),
                bits(st[:, co[t]:co[t + 1]]).ravel().tolist()) for t in range(len(consts))}
