"""The Python mirror of the device gradient under a loss expression, without a device: the predicates of
srhip/losses.py and the routing decisions of api.optimize_constants (Program's device calls patched out)."""
import numpy as np
import pytest

import srhip
from srhip import api, host_optim, losses

import loss_expr_common as X
import loss_expr_grad_common as G
from loss_expr_grad_common import x


def _python_loss(p, t):
    return (p - t) * (p - t)


def test_has_device_gradient():
    assert losses.has_device_gradient(srhip.L2DistLoss())
    assert losses.has_device_gradient(srhip.HuberLoss(1.0))
    assert losses.has_device_gradient(G.l2_expr())
    assert losses.has_device_gradient(G.l2_expr(weighted=True))
    assert not losses.has_device_gradient(_python_loss)
    assert not losses.has_device_gradient(None)


def test_is_device_loss_is_unchanged():
    assert losses.is_device_loss(srhip.L2DistLoss())
    assert not losses.is_device_loss(G.l2_expr())
    assert not losses.is_device_loss(_python_loss)


class _FakeProgram:
    """compile_trees' result with the device calls recorded instead of made."""
    log = []

    def __init__(self, trees):
        self.trees = trees
        self.ntrees = len(trees)

    def optimize_constants(self, ds, loss, **kw):
        _FakeProgram.log.append(("optimize_constants", self.ntrees, type(loss).__name__, kw.get("idx") is not None))
        return np.full(self.ntrees, 0.25), np.ones(self.ntrees, bool), np.full(self.ntrees, 7)

    def optimize_constants_rowsets(self, ds, loss, idxs, **kw):
        _FakeProgram.log.append(("optimize_constants_rowsets", self.ntrees, type(loss).__name__, True))
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


def _members():
    return [G.Member(x(1) * 1.2 + 0.3), G.Member(x(1) * 0.7), G.Member(x(1) + x(2) * 0.4 + 0.1)]


def _options(loss, **kw):
    return srhip.Options(elementwise_loss=loss, **G.TREE_OPS, **kw)


@pytest.mark.parametrize("batching", [False, True])
def test_an_expression_loss_takes_the_device_optimiser(routed, batching):
    dataset, host = routed
    opts = _options(G.lp_expr(), batching=batching, batch_size=40)
    members = _members()
    _, evals = api.optimize_constants(dataset, members, opts, rng=np.random.default_rng(1))
    assert host == []
    if batching:  # no row-set form under an expression: one single-idx device call per member
        assert _FakeProgram.log == [("optimize_constants", 1, "ExprLoss", True)] * 3
        assert evals == sum(7 * (40 / 120) for _ in range(3))
    else:
        assert _FakeProgram.log == [("optimize_constants", 3, "ExprLoss", False)]
        assert evals == 3 * 7
    for m, c0 in zip(members, ([2.2, 1.3], [1.7], [1.4, 1.1])):
        assert np.allclose(srhip.get_constants(m.tree), c0)  # the device's constants were installed
        assert float(m.loss) == 0.25 and m.birth != -1       # and its loss taken, not re-evaluated on the host


def test_one_member_under_an_expression_loss(routed):
    dataset, host = routed
    m = _members()[0]
    got, evals = api.optimize_constants(dataset, m, _options(G.lp_expr()), rng=np.random.default_rng(1))
    assert got is m and host == [] and evals == 7
    assert _FakeProgram.log == [("optimize_constants", 1, "ExprLoss", False)]


def test_builtin_and_python_losses_route_as_before(routed, monkeypatch):
    dataset, host = routed
    api.optimize_constants(dataset, _members(), _options(srhip.L2DistLoss()), rng=np.random.default_rng(1))
    assert _FakeProgram.log == [("optimize_constants", 3, "L2DistLoss", False)] and host == []
    _FakeProgram.log = []
    api.optimize_constants(dataset, _members(), _options(srhip.L2DistLoss(), batching=True, batch_size=40),
                           rng=np.random.default_rng(1))
    assert _FakeProgram.log == [("optimize_constants_rowsets", 3, "L2DistLoss", True)] and host == []
    _FakeProgram.log = []
    monkeypatch.setattr(api, "eval_loss", lambda *a, **k: 0.5)
    api.optimize_constants(dataset, _members(), _options(_python_loss), rng=np.random.default_rng(1))
    assert _FakeProgram.log == [] and host == [2, 1, 2]
