"""Loss expressions against exact math, without a device: the host interpreter (srhip_loss_expr_eval_host) on
every form of tests/loss_expr_ops_common.py against tests/golden/forward_values.npz under the table's own class
bars, the compiled program of every form (srhip_loss_expr_instructions: the slots of the instruction under
test and the program's need), the coverage of every operator at every reachable slot in both operand orders,
and the slots no expression can reach."""
import numpy as np
import pytest

from srhip import _lib

import forward_values_common as fv
import loss_expr_common as X
import loss_expr_ops_common as ops

DTS = ("f32", "f64")


# ---- the host evaluator against the table ---------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_host_evaluator_meets_the_class_bars_in_every_form(dt):
    """Every form on the 191 general points and on the special block: exact and rounded-once operators bit for
    bit, Float32 exp sin cos tan within 1 ulp, Float64 non-exact operators at 1e-14 (1e-13 for gamma and ^),
    NaN exactly where the table has NaN (forward_values_common.failing_rows).  A constant form counts only the
    general row its constant restates; the weight forms run here alone."""
    bad, checked, worst = [], 0, {}
    for form in ops.forms(dt):
        for which in ("general", "special"):
            pred, y, w, want, mask = ops.columns(form, dt, which)
            if not mask.any():
                assert form["row"] is not None and which == "special"
                continue
            got = ops.host_values(form, pred, y, w)
            assert got.dtype == fv.NP[dt]
            rows = fv.failing_rows(form["op"], dt, got, want, mask)
            bad += [(form["label"], which, int(r), float(pred[r]), float(y[r]), float(got[r]), float(want[r])) for r in rows[:3]]
            checked += int(mask.sum())
            worst[form["op"]] = max(worst.get(form["op"], 0.0), ops.worst_ulp(got, want, mask))
    for op in ops.UN_OPS + ops.BIN_OPS:
        print(f"LOSSX_ERR host value {op} {dt} {worst[op]:.0f} ulp")
    assert not bad, (len(bad), bad[:10])
    assert checked > 100000


def test_the_forms_are_the_ones_described():
    """Sizes and needs from the trees alone: op(p) at base 5 is the node limit exactly, p op t at base 4 has 63
    nodes, the swapped form at base 3 has 33 (base 4 would have 65)."""
    forms = ops.forms("f32")
    by = {f["label"]: f for f in forms}
    assert [ops.size(by[f"sin.p@{k}"]["tree"]) for k in ops.UN_BASES] == [2, 4, 8, 16, 32, 64]
    assert [ops.size(by[f"-.pt@{k}"]["tree"]) for k in ops.BIN_BASES] == [3, 7, 15, 31, 63]
    assert [ops.size(by[f"-.t(p1)@{k}"]["tree"]) for k in ops.SWAP_BASES] == [5, 9, 17, 33]
    assert all(ops.size(ops.G(n)) == 2 ** n - 1 and ops.need(ops.G(n)) == n for n in range(1, 7))
    assert all(ops.need(f["tree"]) == f["need"] and ops.size(f["tree"]) <= ops.MAX_NODES for f in forms)
    assert len(forms) == 33 * (6 + 1 + 3) + 13 * (2 * 5 + 2 * 4 + 2 * 3 + 2)
    assert {n for f in forms for n in (f["p"], f["t"], f["w"])} == {"a", "b", None}


# ---- the compiled program -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_every_form_compiles_to_its_slots(dt):
    """(op, dst, a, b) of the instruction under test and the program's need, for every form; over all forms
    together every operator code appears with dst at each of 0 .. 5 and with its second operand at each of
    1 .. 5 in natural order and 0 .. 3 in swapped order; a constant form's immediate is the constant in T."""
    seen_dst, seen_b_nat, seen_b_swap = {}, {}, {}
    for form in ops.forms(dt):
        (op, dst, a, b), nd = ops.instruction_under_test(form, dt)
        code = ops.opcode(form["op"])
        assert (op, (dst, a, b), nd) == (code, form["ins"], form["need"]), form["label"]
        seen_dst.setdefault(code, set()).add(dst)
        if form["kind"] == "bin":
            (seen_b_swap if a > b else seen_b_nat).setdefault(code, set()).add(b)
            assert (a > b) == (form["order"] == "swap"), form["label"]
        ins, _ = ops.expr(form).instructions(fv.NP[dt])
        assert all(i[0] < ops.LX_LOAD_PRED or i[0] in (ops.LX_LOAD_PRED, ops.LX_LOAD_Y, ops.LX_LOAD_W, ops.LX_LOAD_CONST)
                   for i in ins) and len(ins) == ops.size(form["tree"]) and ins[-1][1] == 0
        if form["order"] == "const":
            consts = [imm for o, _, _, _, imm in ins if o == ops.LX_LOAD_CONST]
            a_, b_, _, _ = ops.operands(form["kind"], form["op"], dt, "general")
            c = (b_ if form["p"] == "a" and form["kind"] == "bin" else a_)[form["row"]]
            assert consts == [int(X.bits(np.array([c], fv.NP[dt]))[0])], form["label"]
    codes = {ops.opcode(o) for o in ops.UN_OPS + ops.BIN_OPS}
    assert len(codes) == 46 and set(seen_dst) == codes
    for op in ops.UN_OPS + ops.BIN_OPS:
        code = ops.opcode(op)
        assert seen_dst[code] >= set(range(6)) if op in ops.UN_OPS else seen_dst[code] == set(range(5)), op
        if op in ops.BIN_OPS:
            assert seen_b_nat[code] == {1, 2, 3, 4, 5} and seen_b_swap[code] == {0, 1, 2, 3}, op
    # a binary operator's dst stops at 4: dst = 5 would need slot 6 for its second operand, see below


def test_accessor_arguments():
    lib = _lib.load()
    form = ops.forms("f32")[0]
    h = ops.expr(form).handle(np.float32)
    import ctypes

    n, nd = ctypes.c_int32(), ctypes.c_int32()
    assert lib.srhip_loss_expr_instructions(None, None, None, None, None, None, 0, ctypes.byref(n), None) == _lib.ERR_INVALID
    assert lib.srhip_loss_expr_instructions(h, None, None, None, None, None, 0, None, None) == _lib.ERR_INVALID
    assert lib.srhip_loss_expr_instructions(h, None, None, None, None, None, -1, ctypes.byref(n), None) == _lib.ERR_INVALID
    assert lib.srhip_loss_expr_instructions(h, None, None, None, None, None, 0, ctypes.byref(n), ctypes.byref(nd)) == _lib.OK
    assert (n.value, nd.value) == (2, 1)
    op = np.full(3, 999, np.uint32)
    assert lib.srhip_loss_expr_instructions(h, _lib.ptr(op), None, None, None, None, 1, ctypes.byref(n), None) == _lib.OK
    assert op.tolist() == [ops.LX_LOAD_PRED, 999, 999]  # never past cap


# ---- the slots no expression reaches --------------------------------------------------------------------------
def _ladder(levels, opts):
    """`levels` binary nodes, each with both children the next node, over one leaf: need levels + 1 and
    2^(levels + 1) - 1 nodes with the shared subtrees written out."""
    rows = [(2, 0, opts.binary_index("+"), 0, i + 1, i + 1, 0.0) for i in range(levels)]
    rows.append((0, 0, 0, 1, -1, -1, 0.0))
    return X.node_table(rows)


@pytest.mark.parametrize("dtype", [_lib.F32, _lib.F64], ids=DTS)
def test_slots_six_and_seven_are_unreachable(dtype):
    """An expression has at most 64 nodes, shared subtrees written out, and a tree of stack need n has at
    least 2^n - 1 nodes (need n takes two children of need n - 1): 63 for n = 6, 127 for n = 7.  So no
    accepted expression needs more than 6 slots: cases 6 and 7 of the five kernels' slot switches are dead
    code, and the stack message's "at most 8" is never the binding limit.  The shared ladders are the smallest
    trees of their needs; each is refused, 6 and 7 levels (needs 7 and 8) by the node limit and 8 levels (need
    9, 511 nodes) by the stack limit, which is tested first."""
    opts = ops.options()
    rc, h, _ = X.create_raw(dtype, _ladder(5, opts), opts, 2)
    assert rc == _lib.OK
    import ctypes

    n, nd = ctypes.c_int32(), ctypes.c_int32()
    assert _lib.load().srhip_loss_expr_instructions(h, None, None, None, None, None, 0, ctypes.byref(n), ctypes.byref(nd)) == 0
    assert (n.value, nd.value) == (63, ops.MAX_REACHABLE_NEED)
    X.destroy(h)
    for levels, nodes in ((6, 127), (7, 255)):
        rc, h, msg = X.create_raw(dtype, _ladder(levels, opts), opts, 2)
        assert rc == _lib.ERR_INVALID and not h.value
        assert f"{nodes} nodes" in msg and "at most 64 nodes" in msg and "stack" not in msg
    rc, h, msg = X.create_raw(dtype, _ladder(8, opts), opts, 2)
    assert rc == _lib.ERR_INVALID and not h.value and "9 stack slots" in msg and "at most 8" in msg
    # every accepted form stays within 6, and the deepest ones use all 6
    dt = "f32" if dtype == _lib.F32 else "f64"
    needs = [ops.expr(f).instructions(fv.NP[dt])[1] for f in ops.forms(dt)]
    assert max(needs) == ops.MAX_REACHABLE_NEED
    for f in ops.forms(dt):
        ins, _ = ops.expr(f).instructions(fv.NP[dt])
        assert max(max(i[1:4]) for i in ins) < ops.MAX_REACHABLE_NEED, f["label"]


def test_the_64_node_form_is_the_limit():
    """op(p) at base 5 has exactly 64 nodes and is accepted; one more abs on it is refused by the node limit."""
    import srhip

    form = next(f for f in ops.forms("f64") if f["label"] == "abs.p@5")
    assert ops.size(form["tree"]) == 64
    ins, nd = ops.expr(form).instructions(np.float64)
    assert len(ins) == 64 and nd == 6
    more = srhip.ExprLoss(ops.N("abs", form["tree"]), ops.options())
    with pytest.raises(srhip.SrhipError) as ei:
        more.handle(np.float64)
    assert ei.value.code == _lib.ERR_INVALID and "65 nodes" in str(ei.value) and "at most 64 nodes" in str(ei.value)


# ---- the points of the row-position test ----------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_position_points_resolve_one_float32_ulp(dt):
    """The points tests/test_gpu_loss_expr_ops.py tiles, from the table alone: for every exact-class operator
    (whose device values are exactly the tabulated ones) and every tiled size no row's |l| is under
    m 2^-28 sum|l|, so the derived bound on the mean resolves the last Float32 bit of every row; an odd number
    of points, at least 3.  The other operators keep all 191 points."""
    for kind, names in (("un", ops.UN_OPS), ("bin", ops.BIN_OPS)):
        for op in names:
            pts = ops.position_points(op, kind, dt)
            assert len(pts) % 2 == 1 and len(pts) >= 3, (op, len(pts))
            want = ops.operands(kind, op, dt, "general")[2]
            if fv.GEN.op_class(op) != "exact":
                assert len(pts) == fv.P
                continue
            for m in ops.POSITION_SIZES + (5120,):
                assert ops.small_rows(want[pts[np.arange(m) % len(pts)]], m) == 0, (op, m)
