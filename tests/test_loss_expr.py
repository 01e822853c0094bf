"""Elementwise losses given as expressions, without a device: srhip_loss_expr_create's validation, the host
interpreter (srhip_loss_expr_eval_host) against the oracle and against the numpy forms of srhip/losses.py,
and ExprLoss as a callable loss."""
import ctypes

import numpy as np
import pytest

import srhip
from srhip import _lib
from srhip import api

import loss_expr_common as X

F32_REL = 1e-6   # the project's standing bars (tests/test_gpu_parity.py)
F64_REL = 1e-12

LEAF_P = (0, 0, 0, 1, -1, -1, 0.0)
LEAF_T = (0, 0, 0, 2, -1, -1, 0.0)


def _bin(name, opts):
    return opts.binary_index(name)


def _una(name, opts):
    return opts.unary_index(name)


def _abs_chain(n_abs, opts):
    """abs(abs(... (p - t))): n_abs + 3 nodes."""
    rows = [(1, 0, _una("abs", opts), 0, i + 1, -1, 0.0) for i in range(n_abs)]
    k = n_abs
    rows += [(2, 0, _bin("-", opts), 0, k + 1, k + 2, 0.0), LEAF_P, LEAF_T]
    return X.node_table(rows)


def _shared_ladder(levels, opts):
    """levels binary nodes, each with both children the next node, over one leaf: stack need levels + 1."""
    rows = [(2, 0, _bin("+", opts), 0, i + 1, i + 1, 0.0) for i in range(levels)]
    rows.append(LEAF_P)
    return X.node_table(rows)


# ---- validation -----------------------------------------------------------------------------------
def test_accepts_64_nodes_and_rejects_65():
    opts = X.options()
    rc, h, _ = X.create_raw(_lib.F32, _abs_chain(61, opts), opts, 2)
    assert rc == _lib.OK and h.value
    pred, y = np.array([3.0, -1.0], np.float32), np.array([1.0, 1.0], np.float32)
    out = np.empty(2, np.float32)
    assert _lib.load().srhip_loss_expr_eval_host(h, _lib.ptr(pred), _lib.ptr(y), None, 2, _lib.ptr(out)) == _lib.OK
    assert out.tolist() == [2.0, 2.0]
    X.destroy(h)
    rc, h, msg = X.create_raw(_lib.F32, _abs_chain(62, opts), opts, 2)
    assert rc == _lib.ERR_INVALID and not h.value
    assert "65 nodes" in msg and "at most 64 nodes" in msg


def test_rejects_a_stack_need_of_nine():
    opts = X.options()
    rc, h, msg = X.create_raw(_lib.F64, _shared_ladder(8, opts), opts, 2)
    assert rc == _lib.ERR_INVALID and not h.value
    assert "9 stack slots" in msg and "at most 8" in msg
    # a shared subtree counts once per use: 6 levels are 127 nodes written out
    rc, h, msg = X.create_raw(_lib.F64, _shared_ladder(6, opts), opts, 2)
    assert rc == _lib.ERR_INVALID and "127 nodes" in msg and "at most 64 nodes" in msg
    rc, h, _ = X.create_raw(_lib.F64, _shared_ladder(5, opts), opts, 2)  # 63 nodes, need 6
    assert rc == _lib.OK
    pred, y = np.array([1.5]), np.array([0.0])
    out = np.empty(1)
    assert _lib.load().srhip_loss_expr_eval_host(h, _lib.ptr(pred), _lib.ptr(y), None, 1, _lib.ptr(out)) == _lib.OK
    assert out[0] == 1.5 * 32
    X.destroy(h)


@pytest.mark.parametrize("feature,nargs", [(3, 2), (0, 2), (4, 3), (0, 3)])
def test_rejects_feature_outside_nargs(feature, nargs):
    opts = X.options()
    nodes = X.node_table([(2, 0, _bin("-", opts), 0, 1, 2, 0.0), LEAF_P, (0, 0, 0, feature, -1, -1, 0.0)])
    rc, h, msg = X.create_raw(_lib.F32, nodes, opts, nargs)
    assert rc == _lib.ERR_INVALID and not h.value
    assert f"feature index {feature}" in msg and f"1..{nargs}" in msg


def test_feature_three_needs_nargs_three():
    opts = X.options()
    nodes = X.node_table([(2, 0, _bin("*", opts), 0, 1, 2, 0.0), (0, 0, 0, 3, -1, -1, 0.0), LEAF_P])
    rc, h, _ = X.create_raw(_lib.F32, nodes, opts, 3)
    assert rc == _lib.OK
    X.destroy(h)


def test_rejects_operator_index_out_of_range():
    opts = X.options()
    for deg, op, word in ((2, opts.nbin + 1, "binary"), (2, 0, "binary"), (1, opts.nuna + 1, "unary")):
        nodes = X.node_table([(deg, 0, op, 0, 1, 2 if deg == 2 else -1, 0.0), LEAF_P, LEAF_T])
        rc, h, msg = X.create_raw(_lib.F32, nodes, opts, 2)
        assert rc == _lib.ERR_INVALID and not h.value
        assert f"{word} operator index {op}" in msg


def test_rejects_non_finite_constants():
    opts = X.options()
    for dtype, val in ((_lib.F32, np.nan), (_lib.F64, np.inf), (_lib.F32, 1e39)):  # 1e39 is Inf in Float32
        nodes = X.node_table([(2, 0, _bin("-", opts), 0, 1, 2, 0.0), LEAF_P, (0, 1, 0, 0, -1, -1, val)])
        rc, h, msg = X.create_raw(dtype, nodes, opts, 2)
        assert rc == _lib.ERR_INVALID and not h.value and "non-finite constant" in msg
    nodes = X.node_table([(2, 0, _bin("-", opts), 0, 1, 2, 0.0), LEAF_P, (0, 1, 0, 0, -1, -1, 1e39)])
    rc, h, _ = X.create_raw(_lib.F64, nodes, opts, 2)
    assert rc == _lib.OK
    X.destroy(h)


def test_rejects_int32_null_pointers_and_malformed_trees():
    opts = X.options()
    nodes = _abs_chain(1, opts)
    rc, h, msg = X.create_raw(_lib.I32, nodes, opts, 2)
    assert rc == _lib.ERR_UNSUPPORTED and "Int32" in msg
    assert X.create_raw(7, nodes, opts, 2)[0] == _lib.ERR_INVALID
    assert X.create_raw(_lib.F32, nodes, opts, 4)[0] == _lib.ERR_INVALID
    assert X.create_raw(_lib.F32, nodes, opts, 2, nnodes=0)[0] == _lib.ERR_INVALID
    lib = _lib.load()
    ops = opts.c_operators()
    h = ctypes.c_void_p()
    assert lib.srhip_loss_expr_create(_lib.F32, None, 3, ctypes.byref(ops), 2, ctypes.byref(h)) == _lib.ERR_INVALID
    assert lib.srhip_loss_expr_create(_lib.F32, _lib.ptr(nodes), len(nodes), None, 2, ctypes.byref(h)) == _lib.ERR_INVALID
    assert lib.srhip_loss_expr_create(_lib.F32, _lib.ptr(nodes), len(nodes), ctypes.byref(ops), 2, None) == _lib.ERR_INVALID
    # a child index out of range, and a node that is its own descendant
    bad = X.node_table([(2, 0, _bin("-", opts), 0, 1, 5, 0.0), LEAF_P, LEAF_T])
    rc, _, msg = X.create_raw(_lib.F32, bad, opts, 2)
    assert rc == _lib.ERR_INVALID and "child index" in msg
    loop = X.node_table([(1, 0, _una("abs", opts), 0, 1, -1, 0.0), (1, 0, _una("abs", opts), 0, 0, -1, 0.0)])
    rc, _, msg = X.create_raw(_lib.F32, loop, opts, 2)
    assert rc == _lib.ERR_INVALID and "descendant" in msg
    # the evaluator's own arguments
    rc, h, _ = X.create_raw(_lib.F32, nodes, opts, 2)
    assert rc == _lib.OK
    a = np.zeros(4, np.float32)
    assert lib.srhip_loss_expr_eval_host(None, _lib.ptr(a), _lib.ptr(a), None, 4, _lib.ptr(a)) == _lib.ERR_INVALID
    assert lib.srhip_loss_expr_eval_host(h, None, _lib.ptr(a), None, 4, _lib.ptr(a)) == _lib.ERR_INVALID
    assert lib.srhip_loss_expr_eval_host(h, _lib.ptr(a), _lib.ptr(a), None, 4, None) == _lib.ERR_INVALID
    assert lib.srhip_loss_expr_eval_host(h, _lib.ptr(a), _lib.ptr(a), None, 0, None) == _lib.OK
    X.destroy(h)
    lib.srhip_loss_expr_destroy(None)
    w3 = X.node_table([(2, 0, _bin("*", opts), 0, 1, 2, 0.0), (0, 0, 0, 3, -1, -1, 0.0), LEAF_P])
    rc, h, _ = X.create_raw(_lib.F32, w3, opts, 3)
    assert lib.srhip_loss_expr_eval_host(h, _lib.ptr(a), _lib.ptr(a), None, 4, _lib.ptr(a)) == _lib.ERR_INVALID
    X.destroy(h)


def test_block_rows_getter_matches_the_header_constant():
    # csrc/srhip_lossx.h: LOSSX_BLOCK_ROWS = 256 threads x 4 rows per lane x 4 passes
    assert _lib.load().srhip_lossx_block_rows() == 4096


def test_compile_unit_calls_no_hip_runtime():
    """csrc/srhip_lossx_compile.cpp is device-free, like the tree compiler (tests/test_abi.py)."""
    import os
    import re
    import subprocess

    obj = os.path.join(os.path.dirname(_lib.LIB_PATH), "srhip_lossx_compile.o")
    assert os.path.isfile(obj), f"{obj} is missing: the build makes it"
    out = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout
    undefined = [ln.split()[-1] for ln in out.splitlines() if ln.split()]
    assert undefined and not [s for s in undefined if re.match(r"^hip[A-Z]", s)], undefined


# ---- the host evaluator ---------------------------------------------------------------------------
def _weighted(expr):
    return X.W() * expr


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", X.CASES, ids=X.CASE_IDS)
def test_host_evaluator_equals_oracle_bit_for_bit(oracle, case, dtype):
    """srhip_loss_expr_eval_host = oracle.eval_tree of the same node table on X' = [pred; y; w]."""
    name, _, build, _, family = case
    opts = X.options()
    pred, y, w = X.inputs(family, dtype)
    Xp = np.stack([pred, y, w])
    for tree, args in ((build(), (pred, y)), (_weighted(build()), (pred, y, w))):
        loss = srhip.ExprLoss(tree, opts)
        got = loss(*args)
        nodes, _ = srhip.flatten([tree], opts, dtype)
        want, ok = oracle.eval_tree(nodes, opts.binop_codes, opts.unaop_codes, Xp)
        assert ok and np.all(np.isfinite(want)), name
        assert got.dtype == dtype and np.array_equal(X.bits(got), X.bits(want)), name


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", X.CASES, ids=X.CASE_IDS)
def test_host_evaluator_against_losses_py(case, dtype):
    """The same expressions against the numpy forms of srhip/losses.py: the exact class of DESIGN.md 4 bit
    for bit, the others within F32_REL / F64_REL per row."""
    name, ref, build, exact, family = case
    pred, y, _ = X.inputs(family, dtype)
    got = srhip.ExprLoss(build(), X.options())(pred, y)
    want = np.asarray(ref(pred, y))
    assert want.dtype == dtype and np.all(np.isfinite(want))
    if exact:
        # (a zero of either sign is the same loss: the numpy forms select with where, the expressions add
        # the unselected branch's signed zero)
        assert np.array_equal(X.bits(got + dtype(0)), X.bits(want + dtype(0))), name
    else:
        rel = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.maximum(np.abs(want.astype(np.float64)), 1e-300)
        assert rel.max() <= (F32_REL if dtype == np.float32 else F64_REL), (name, rel.max())


def test_piecewise_cases_take_every_branch():
    """The general inputs reach both sides of every threshold the piecewise expressions select on."""
    pred, y, _ = X.inputs("dist", np.float64)
    d = np.abs(pred - y)
    assert (d < 0.5).any() and ((d > 0.5) & (d < 1)).any() and (d > 1).any() and ((pred - y) < 0).any()
    pred, y, _ = X.inputs("margin", np.float64)
    a = pred * y
    assert (a < -1).any() and ((a > -1) & (a < 0)).any() and ((a > 0.5) & (a < 1)).any() and (a > 1).any()
    pred, y, _ = X.inputs("margin_cond", np.float64)
    a = pred * y
    assert (a < 0).any() and ((a > 0) & (a < 0.5)).any() and (a > 0.5).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reference_lp_loss(dtype):
    """abs(p - t)^2.5 (the reference's own test of a function loss, test/test_losses.jl)."""
    pred, y, w = X.inputs("dist", dtype)
    opts = X.options()
    got = srhip.ExprLoss(X.N("abs", X.diff()) ** X.C(2.5), opts)(pred, y)
    d = (pred - y).astype(np.float64)  # the difference as T computes it
    want = np.abs(d) ** 2.5
    assert np.allclose(got, want, rtol=F32_REL if dtype == np.float32 else F64_REL, atol=0)
    gw = srhip.ExprLoss(X.W() * (X.N("abs", X.diff()) ** X.C(2.5)), opts)(pred, y, w)
    assert np.array_equal(X.bits(gw), X.bits(w * got))


def test_safe_operator_semantics():
    """Loss expressions use the device's operators: ^ is safe_pow, log is safe_log, sqrt is safe_sqrt."""
    opts = X.options()
    pred, y = np.array([-2.0, 2.0, 0.0]), np.array([0.0, 0.0, 0.0])
    assert np.isnan(srhip.ExprLoss(X.diff() ** X.C(2.5), opts)(pred, y)).tolist() == [True, False, False]
    assert np.isnan(srhip.ExprLoss(X.N("log", X.diff()), opts)(pred, y)).tolist() == [True, False, True]
    assert np.isnan(srhip.ExprLoss(X.N("sqrt", X.diff()), opts)(pred, y)).tolist() == [True, False, False]
    out = srhip.ExprLoss(X.C(1.0) / (X.P() - X.P()), opts)(pred, y)
    assert np.all(np.isposinf(out))


# ---- ExprLoss as a callable --------------------------------------------------------------------------
def test_expr_loss_is_a_callable_loss():
    opts = X.options()
    loss = srhip.ExprLoss(X.N("abs", X.diff()) ** X.C(2.5), opts)
    wloss = srhip.ExprLoss(X.W() * (X.N("abs", X.diff()) ** X.C(2.5)), opts)
    assert loss.nargs == 2 and wloss.nargs == 3
    for dtype in (np.float32, np.float64):
        pred, y, w = X.inputs("dist", dtype)
        vals = loss(pred, y)
        assert isinstance(loss(pred[0], y[0]), dtype) and loss(pred[0], y[0]) == vals[0]
        got = api._host_elementwise_loss(pred, y, None, loss)
        assert got == float(np.sum(vals.astype(np.float64)) / len(pred))
        gotw = api._host_elementwise_loss(pred, y, w, wloss)
        assert gotw == float(np.sum(wloss(pred, y, w).astype(np.float64)) / np.sum(w.astype(np.float64)))
        with pytest.raises(TypeError):
            wloss(pred, y)
    o = srhip.Options(binary_operators=("+", "*"), elementwise_loss=loss)
    assert o.elementwise_loss is loss and not srhip.losses.is_device_loss(loss)
    with pytest.raises(srhip.SrhipError) as ei:
        loss.handle(np.int32)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    import pickle

    again = pickle.loads(pickle.dumps(loss))
    assert again(np.float32(3.0), np.float32(1.0)) == loss(np.float32(3.0), np.float32(1.0))
