"""One row subset per member in the constant optimiser (the batching mode's per-member minibatch): the
parts that need no device -- the two C ABI entries, and api.optimize_constants' host path (a user
loss_function) in batching mode, which keeps its per-member loop: the same results and the same
consumption of the random generator as a hand-written restatement of that loop."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ENTRIES = ("srhip_eval_loss_grad_rowsets", "srhip_optimize_constants_rowsets")


def _sr():
    import srhip

    return srhip


def test_header_declares_and_library_exports_the_entry_points():
    sr = _sr()
    header = open(os.path.join(ROOT, "include", "srhip.h")).read()
    lib = ctypes.CDLL(sr.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in sr._lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(sr._lib.SIGNATURES["srhip_eval_loss_grad_rowsets"][1]) == 9
    assert len(sr._lib.SIGNATURES["srhip_optimize_constants_rowsets"][1]) == 13
    assert hasattr(sr.Program, "eval_loss_grad_rowsets") and hasattr(sr.Program, "optimize_constants_rowsets")


def _setup():
    sr = _sr()

    def loss_of_idx(tree, dataset, options, idx):
        # deterministic in (constants, idx): no evaluation, no device; a bowl around 0.5 in every constant
        idx = np.arange(dataset.n) if idx is None else np.asarray(idx)
        c = np.asarray(sr.get_constants(tree), dtype=np.float64)
        return float(np.sum((c - 0.5) ** 2)) + float(sr.count_nodes(tree)) + float(np.sum(idx * np.arange(1, len(idx) + 1)) % 1009) / 1009.0

    opts = sr.Options(binary_operators=("+", "*"), unary_operators=("cos",), loss_function=loss_of_idx,
                      batching=True, batch_size=7)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((3, 200))
    ds = sr.Dataset(X, X[0] * 2.0)
    trees = sr.random_population(9, opts, 3, np.float64, 5, 12)
    return sr, opts, ds, trees


def _loop(sr, ds, trees, opts, rng, subsets=None):
    """api.optimize_constants' batching-mode host loop, restated: every member's batch_sample first, then
    per member the host optimiser on its subset (which draws its restarts from rng)."""
    from srhip.api import _optimize_constants_host, batch_sample

    if subsets is None:
        subsets = [batch_sample(ds, opts, rng) for _ in trees]
    num_evals = 0.0
    for t, idx in zip(trees, subsets):
        (ok, c, _, fc), = _optimize_constants_host(ds, [t], opts, rng, idx)
        num_evals += float(fc) * (opts.batch_size / ds.n)
        if ok:
            sr.set_constants(t, c)
    return num_evals


def test_host_loss_batching_list_keeps_its_loop_and_generator_state():
    sr, opts, ds, trees = _setup()
    ta, tb = [t.copy() for t in trees], [t.copy() for t in trees]
    rng_a, rng_b = np.random.default_rng(7), np.random.default_rng(7)
    out, evals_a = sr.optimize_constants(ds, ta, opts, rng=rng_a)
    evals_b = _loop(sr, ds, tb, opts, rng_b)
    assert out is not None and evals_a == evals_b and evals_a > 0
    ca = [list(sr.get_constants(t)) for t in ta]
    assert ca == [list(sr.get_constants(t)) for t in tb]
    assert ca != [list(sr.get_constants(t)) for t in trees]  # something was optimised
    assert rng_a.integers(0, 1 << 30) == rng_b.integers(0, 1 << 30)  # the same generator state afterwards


def test_idxs_gives_the_subsets_without_a_draw():
    sr, opts, ds, trees = _setup()
    idxs = [np.arange(t + 1, t + 8) for t in range(len(trees))]
    ta, tb = [t.copy() for t in trees], [t.copy() for t in trees]
    rng_a, rng_b = np.random.default_rng(11), np.random.default_rng(11)
    _, evals_a = sr.optimize_constants(ds, ta, opts, rng=rng_a, idxs=idxs)
    evals_b = _loop(sr, ds, tb, opts, rng_b, subsets=idxs)
    assert evals_a == evals_b
    assert [list(sr.get_constants(t)) for t in ta] == [list(sr.get_constants(t)) for t in tb]
    assert rng_a.integers(0, 1 << 30) == rng_b.integers(0, 1 << 30)


def test_idxs_with_the_wrong_count_raises():
    sr, opts, ds, trees = _setup()
    idxs = [np.arange(5) for _ in trees]
    with pytest.raises(ValueError, match="8 row subsets for 9 members"):
        sr.optimize_constants(ds, trees, opts, rng=np.random.default_rng(1), idxs=idxs[:-1])
    with pytest.raises(ValueError, match="exclusive"):
        sr.optimize_constants(ds, trees, opts, rng=np.random.default_rng(1), idx=np.arange(5), idxs=idxs)
    with pytest.raises(ValueError, match="8 row subsets for 9 trees"):
        sr.eval_grad_loss_batch(trees, ds, opts, idxs=idxs[:-1])
