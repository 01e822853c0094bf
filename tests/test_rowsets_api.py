"""One row subset per tree (the batching mode's fresh minibatch per score): the parts that need no
device -- the C ABI entry, the packing of ragged subsets, and the host fall-back of
eval_loss_rowsets_batch / score_func_batched_batch for a user loss_function, which must equal the
per-member loops over eval_loss / score_func_batched and consume the random generator alike."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _sr():
    import srhip

    return srhip


def test_header_declares_and_library_exports_rowsets():
    sr = _sr()
    header = open(os.path.join(ROOT, "include", "srhip.h")).read()
    assert re.search(r"\bint\s+srhip_eval_loss_rowsets\s*\(", header)
    assert "srhip_eval_loss_rowsets" in sr._lib.SIGNATURES
    lib = ctypes.CDLL(sr.LIB_PATH)
    assert hasattr(lib, "srhip_eval_loss_rowsets")


def test_pack_rowsets():
    from srhip.device import pack_rowsets

    offs, rows = pack_rowsets([[3, 3, 1], np.array([7]), np.arange(4, dtype=np.int32)])
    assert offs.dtype == np.int64 and rows.dtype == np.int64
    assert offs.tolist() == [0, 3, 4, 8]
    assert rows.tolist() == [3, 3, 1, 7, 0, 1, 2, 3]
    offs, rows = pack_rowsets([np.array([5, 6])], ntrees=1)
    assert offs.tolist() == [0, 2] and rows.tolist() == [5, 6]
    with pytest.raises(ValueError, match="tree 1 is empty"):
        pack_rowsets([[1], [], [2]])
    with pytest.raises(ValueError, match="2 row subsets for 3 trees"):
        pack_rowsets([[1], [2]], ntrees=3)


def _setup():
    sr = _sr()

    def loss_of_idx(tree, dataset, options, idx):
        # deterministic in (tree size, idx): no evaluation, no device
        idx = np.arange(dataset.n) if idx is None else np.asarray(idx)
        return float(sr.count_nodes(tree)) + float(np.sum(idx * np.arange(1, len(idx) + 1)) % 1009) / 1009.0

    opts = sr.Options(binary_operators=("+", "*"), unary_operators=("cos",), loss_function=loss_of_idx,
                      batching=True, batch_size=7)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((3, 200))
    ds = sr.Dataset(X, X[0] * 2.0)
    trees = sr.random_population(9, opts, 3, np.float64, 5, 12)
    return sr, opts, ds, trees


def test_score_func_batched_batch_equals_the_loop_and_consumes_rng_alike():
    sr, opts, ds, trees = _setup()
    rng_a, rng_b = np.random.default_rng(7), np.random.default_rng(7)
    scores, losses = sr.score_func_batched_batch(ds, trees, opts, rng=rng_a)
    loop = [sr.score_func_batched(ds, t, opts, rng=rng_b) for t in trees]
    assert scores.dtype == ds.loss_type and losses.dtype == ds.loss_type
    assert [float(s) for s in scores] == [float(s) for s, _ in loop]
    assert [float(l) for l in losses] == [float(l) for _, l in loop]
    assert len(set(float(l) for l in losses)) > 1
    assert rng_a.integers(0, 1 << 30) == rng_b.integers(0, 1 << 30)  # the same generator state afterwards
    # explicit subsets: no draw
    idxs = [np.arange(t + 1, t + 5) for t in range(len(trees))]
    rng_c = np.random.default_rng(11)
    s2, l2 = sr.score_func_batched_batch(ds, trees, opts, idxs=idxs, rng=rng_c)
    assert rng_c.integers(0, 1 << 30) == np.random.default_rng(11).integers(0, 1 << 30)
    assert [float(l) for l in l2] == [float(sr.score_func_batched(ds, t, opts, idx=i)[1]) for t, i in zip(trees, idxs)]


def test_eval_loss_rowsets_batch_host_fallback_equals_eval_loss():
    sr, opts, ds, trees = _setup()
    idxs = [np.random.default_rng(20 + t).integers(0, ds.n, size=1 + 3 * t) for t in range(len(trees))]
    out, ok = sr.eval_loss_rowsets_batch(trees, ds, opts, idxs)
    want = [float(sr.eval_loss(t, ds, opts, idx=i)) for t, i in zip(trees, idxs)]
    assert out.dtype == np.float64 and out.tolist() == want and ok.all()
    with pytest.raises(ValueError):
        sr.eval_loss_rowsets_batch(trees, ds, opts, idxs[:-1])
