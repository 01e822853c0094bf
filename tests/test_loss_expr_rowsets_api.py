"""The row-set entry points for a loss expression without a device: the exported symbols and their null
checks, the predicate of srhip/losses.py and the routing of the three mirror functions (Program's device calls
patched out, in the manner of tests/test_loss_expr_grad_api.py)."""
import ctypes

import numpy as np
import pytest

import srhip
from srhip import _lib, api, host_optim, losses

import loss_expr_grad_common as G
import loss_expr_rowsets_common as R
from loss_expr_grad_common import x

SYMBOLS = ("srhip_eval_loss_expr_rowsets", "srhip_eval_loss_grad_expr_rowsets", "srhip_optimize_constants_expr_rowsets",
           "srhip_rowsets_fallback_trees")


def test_symbols_are_exported_and_reject_null_arguments():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    h = G.l2_expr().handle(np.float32)
    off, rows = np.array([0, 1], np.int64), np.array([0], np.int64)
    out, ok, grad = np.empty(1), np.empty(1, np.uint8), np.empty(1)
    imp, fc = np.empty(1, np.uint8), np.empty(1, np.int64)
    opt = _lib.OptimOptions(2, 1, 0, 1e-8)
    p = _lib.ptr
    # a null context / dataset / program
    assert lib.srhip_eval_loss_expr_rowsets(None, None, None, h, p(off), p(rows), p(out), p(ok)) == _lib.ERR_INVALID
    assert "null" in lib.srhip_last_error().decode()
    assert lib.srhip_eval_loss_grad_expr_rowsets(None, None, None, h, p(off), p(rows), p(out), p(grad), p(ok)) == _lib.ERR_INVALID
    assert lib.srhip_optimize_constants_expr_rowsets(None, None, None, h, p(off), p(rows), ctypes.byref(opt), None, None, None,
                                                     p(out), p(imp), p(fc)) == _lib.ERR_INVALID
    # null pointers: the expression, the row sets, the outputs, the options
    assert lib.srhip_eval_loss_expr_rowsets(None, None, None, None, p(off), p(rows), p(out), p(ok)) == _lib.ERR_INVALID
    assert "null loss expression" in lib.srhip_last_error().decode()
    assert lib.srhip_eval_loss_expr_rowsets(None, None, None, h, None, p(rows), p(out), p(ok)) == _lib.ERR_INVALID
    assert lib.srhip_eval_loss_expr_rowsets(None, None, None, h, p(off), None, p(out), p(ok)) == _lib.ERR_INVALID
    assert lib.srhip_eval_loss_expr_rowsets(None, None, None, h, p(off), p(rows), None, p(ok)) == _lib.ERR_INVALID
    assert lib.srhip_eval_loss_grad_expr_rowsets(None, None, None, h, p(off), p(rows), p(out), None, p(ok)) == _lib.ERR_INVALID
    assert lib.srhip_optimize_constants_expr_rowsets(None, None, None, h, p(off), p(rows), None, None, None, None,
                                                     p(out), p(imp), p(fc)) == _lib.ERR_INVALID
    assert lib.srhip_rowsets_fallback_trees(None) < 0
    # the caps the GPU tests are built around, as include/srhip.h gives them
    assert R.score_cap(np.float32, 1, False) == 5120 and R.score_cap(np.float32, 8, True) == 1024
    assert R.grad_cap(np.float32, 5, False) == 1536 and R.grad_cap(np.float64, 5, False) == 768
    for dt in (np.float32, np.float64):
        for nf in (1, 3, 5, 8):
            for w in (False, True):
                assert 0 < R.grad_cap(dt, nf, w) <= R.score_cap(dt, nf, w)


def _python_loss(p, t):
    return (p - t) * (p - t)


def test_has_device_rowsets():
    assert losses.has_device_rowsets(srhip.L2DistLoss())
    assert losses.has_device_rowsets(srhip.HuberLoss(1.0))
    assert losses.has_device_rowsets(G.l2_expr())
    assert losses.has_device_rowsets(R.lp_expr(weighted=True))
    assert not losses.has_device_rowsets(_python_loss)
    assert not losses.has_device_rowsets(None)
    assert not losses.is_device_loss(G.l2_expr())  # unchanged


class _FakeProgram:
    """compile_trees' result with the device calls recorded instead of made."""
    log = []

    def __init__(self, trees):
        self.trees = trees
        self.ntrees = len(trees)

    def _note(self, name, loss, rowsets):
        _FakeProgram.log.append((name, self.ntrees, type(loss).__name__, rowsets))

    def eval_loss(self, ds, loss, idx=None):
        self._note("eval_loss", loss, False)
        return np.full(self.ntrees, 0.5), np.ones(self.ntrees, bool)

    def eval_loss_rowsets(self, ds, loss, idxs):
        self._note("eval_loss_rowsets", loss, len(idxs))
        return np.full(self.ntrees, 0.5), np.ones(self.ntrees, bool)

    def eval_loss_grad(self, ds, loss, idx=None):
        self._note("eval_loss_grad", loss, False)
        return np.full(self.ntrees, 0.5), [np.zeros(1)] * self.ntrees, np.ones(self.ntrees, bool)

    def eval_loss_grad_rowsets(self, ds, loss, idxs):
        self._note("eval_loss_grad_rowsets", loss, len(idxs))
        return np.full(self.ntrees, 0.5), [np.zeros(1)] * self.ntrees, np.ones(self.ntrees, bool)

    def optimize_constants(self, ds, loss, **kw):
        self._note("optimize_constants", loss, kw.get("idx") is not None)
        return np.full(self.ntrees, 0.25), np.ones(self.ntrees, bool), np.full(self.ntrees, 7)

    def optimize_constants_rowsets(self, ds, loss, idxs, **kw):
        self._note("optimize_constants_rowsets", loss, len(idxs))
        assert len(kw["seeds"]) == self.ntrees
        return np.full(self.ntrees, 0.25), np.ones(self.ntrees, bool), np.full(self.ntrees, 7)

    def get_constants(self):
        return [np.asarray(srhip.get_constants(t), dtype=np.float64) + 1.0 for t in self.trees]

    def close(self):
        pass


@pytest.fixture
def routed(monkeypatch):
    _FakeProgram.log = []
    monkeypatch.setattr(api, "compile_trees", lambda trees, options, dtype: _FakeProgram(list(trees)))
    monkeypatch.setattr(api, "_ctx", lambda options: None)
    monkeypatch.setattr(srhip.Dataset, "device", lambda self, ctx: None)
    host = []

    def fake_host(objective, x0, **kw):
        host.append(len(x0))
        return x0, 0.5, False, 3, None

    monkeypatch.setattr(host_optim, "optimize", fake_host)
    rng = np.random.default_rng(0)
    Xd = rng.standard_normal((2, 120))
    dataset = srhip.Dataset(Xd, 2.0 * Xd[0] + 1.0)
    dataset.baseline_loss, dataset.use_baseline = 1.0, True
    return dataset, host


def _trees():
    return [x(1) * 1.2 + 0.3, x(1) * 0.7, x(1) + x(2) * 0.4 + 0.1]


def _options(loss, **kw):
    return srhip.Options(elementwise_loss=loss, **G.TREE_OPS, **kw)


IDXS = [np.arange(5), np.arange(40), np.array([3, 3, 7])]


def test_scoring_and_gradient_take_one_rowsets_call(routed):
    dataset, _ = routed
    opts = _options(R.lp_expr())
    out, ok = api.eval_loss_rowsets_batch(_trees(), dataset, opts, IDXS)
    assert _FakeProgram.log == [("eval_loss_rowsets", 3, "ExprLoss", 3)] and out.tolist() == [0.5] * 3 and ok.all()
    _FakeProgram.log = []
    api.eval_grad_loss_batch(_trees(), dataset, opts, idxs=IDXS)
    assert _FakeProgram.log == [("eval_loss_grad_rowsets", 3, "ExprLoss", 3)]
    _FakeProgram.log = []
    members = [G.Member(t) for t in _trees()]
    api.score_func_batched_batch(dataset, members, opts, idxs=IDXS)
    assert _FakeProgram.log == [("eval_loss_rowsets", 3, "ExprLoss", 3)]


def test_optimiser_with_idxs_takes_one_rowsets_call(routed):
    dataset, host = routed
    members = [G.Member(t) for t in _trees()]
    _, evals = api.optimize_constants(dataset, members, _options(R.lp_expr()), rng=np.random.default_rng(1), idxs=IDXS)
    assert host == [] and _FakeProgram.log == [("optimize_constants_rowsets", 3, "ExprLoss", 3)]
    assert evals == 3 * 7
    for m, c0 in zip(members, ([2.2, 1.3], [1.7], [1.4, 1.1])):
        assert np.allclose(srhip.get_constants(m.tree), c0) and float(m.loss) == 0.25 and m.birth != -1


def test_self_drawn_batching_branch_keeps_per_member_calls(routed):
    """The one remaining step: where api.optimize_constants draws the minibatches itself, an ExprLoss still takes
    one single-idx device call per member (tests/test_loss_expr_grad_api.py pins the same routing)."""
    dataset, host = routed
    assert losses.has_device_rowsets(R.lp_expr())  # the device has the row-set form; this branch does not use it yet
    members = [G.Member(t) for t in _trees()]
    api.optimize_constants(dataset, members, _options(R.lp_expr(), batching=True, batch_size=40), rng=np.random.default_rng(1))
    assert host == [] and _FakeProgram.log == [("optimize_constants", 1, "ExprLoss", True)] * 3


def test_a_python_loss_still_takes_the_loops(routed, monkeypatch):
    dataset, host = routed
    assert not losses.has_device_rowsets(_python_loss)
    monkeypatch.setattr(api, "eval_loss", lambda *a, **k: 0.5)
    out, ok = api.eval_loss_rowsets_batch(_trees(), dataset, _options(_python_loss), IDXS)
    assert _FakeProgram.log == [] and out.tolist() == [0.5] * 3
    api.optimize_constants(dataset, [G.Member(t) for t in _trees()], _options(_python_loss), rng=np.random.default_rng(1),
                           idxs=IDXS)
    assert _FakeProgram.log == [] and host == [2, 1, 2]
