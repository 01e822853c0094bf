"""Shared by tests/test_loss_expr_ops_table.py (no device) and tests/test_gpu_loss_expr_ops.py: loss
expressions that put every operator, at every value slot the loss compiler can reach and in both operand
orders, in front of the golden tables of exact forward values and exact derivatives.  Not a test module.

Every form is an ExprLoss over p = Node(feature=1) (prediction), t = Node(feature=2) (target) and, on the host
only, w = Node(feature=3), under one option set that names all 13 binary and 33 unary operators.  Operands
reach the operator under test unchanged, through identities that are exact for every value (-0.0, subnormals,
Inf and NaN included): `x * 1.0` and `cond(1.0, x)`.

Slots (csrc/srhip_lossx_compile.cpp emit; the scheme of tests/forward_values_common.py restated for this
compiler): every leaf takes a slot, a binary operator evaluates the child of greater need first (the left one
on a tie) into slot `base` and the other into base + 1, and the loss compiler folds no constant, so depth is
built from constants:

    G(n)     a complete tree of `*` over C(1.0) leaves: need n, 2^n - 1 nodes, value 1
    lift(T)  cond(G(need(T)), T): equal needs, so G goes first and T runs one slot up; the value is T's
    op(p) at base k = 0 .. 5         2, 4, 8, 16, 32, 64 nodes: base 5 is the node limit exactly
    p op t, t op p at base 0 .. 4    3, 7, 15, 31, 63 nodes; the operator reads slots base and base + 1
    p op (t * 1), t op (p * 1) at base 0 .. 3   the left need 1 is below the right need 2: the right child
                                     goes first and the instruction carries a = base + 1, b = base
    p op C(c), C(c) op p, op(C(c))   c restating the table's operand at the rows of CONST_ROWS (only that row
                                     counts): LX_LOAD_CONST's immediate in T
    p op w, w op p                   nargs = 3, host only (on the device a weighted mean divides by sum w)

Each form carries the (dst, a, b) the compiler must give the instruction under test, and the program's need.
"""
import numpy as np

import srhip

import derivative_rules_common as dr
import forward_values_common as fv

NP = fv.NP
UN_OPS, BIN_OPS = fv.UN_OPS, fv.BIN_OPS
CONST_ROWS = fv.CONST_ROWS
UN_BASES, BIN_BASES, SWAP_BASES = range(6), range(5), range(4)
MAX_NODES = 64            # csrc/srhip_lossx.h LOSSX_MAX_NODES
MAX_REACHABLE_NEED = 6    # a tree of need n has at least 2^n - 1 nodes: 63 for n = 6, 127 for n = 7
LX_LOAD_PRED, LX_LOAD_Y, LX_LOAD_W, LX_LOAD_CONST = 0x100, 0x101, 0x102, 0x103

_OPTS = None


def options():
    global _OPTS
    if _OPTS is None:
        _OPTS = srhip.Options(binary_operators=tuple(BIN_OPS), unary_operators=tuple(UN_OPS))
    return _OPTS


def opcode(op):
    """The device code of an operator name, as the compiled program carries it."""
    o = options()
    if op in BIN_OPS:
        return int(o.binop_codes[o.binary_index(op) - 1])
    return int(o.unaop_codes[o.unary_index(op) - 1])


def N(op, *args):
    return srhip.Node(op, *args)


def C(v):
    return srhip.Node(val=float(v))


def P():
    return srhip.Node(feature=1)


def T_():
    return srhip.Node(feature=2)


def W():
    return srhip.Node(feature=3)


def need(t):
    """The loss compiler's stack need: 1 for a leaf, one more than two equal children's."""
    if t.degree == 0:
        return 1
    if t.degree == 1:
        return need(t.l)
    a, b = need(t.l), need(t.r)
    return a + 1 if a == b else max(a, b)


def size(t):
    return 1 + sum(size(c) for c in (t.l, t.r)[:t.degree])


def G(n):
    return C(1.0) if n == 1 else N("*", G(n - 1), G(n - 1))


def lift(t):
    return N("cond", G(need(t)), t)


def at_base(t, k):
    for _ in range(k):
        t = lift(t)
    return t


# ---- the forms over the forward table -------------------------------------------------------------------------
_FORMS = {}


def forms(dt):
    """Every form as a dict: label, kind ("un" / "bin"), op, order ("nat" / "swap" / "const" / "weight"), base,
    tree, p / t / w (which table operand the argument carries: "a" (a unary operator's x too), "b" or None),
    row (None, or the one general row that counts), ins (the expected (dst, a, b) of the instruction under
    test, which is instruction len - 1 - base: the lifts' conds follow it), need, nargs."""
    if dt in _FORMS:
        return _FORMS[dt]
    z = fv.table()
    out = []

    def add(label, kind, op, order, base, tree, p, t, ins, w=None, row=None):
        out.append(dict(label=f"{op}.{label}", kind=kind, op=op, order=order, base=base, tree=at_base(tree, base), p=p, t=t,
                        w=w, row=row, ins=ins, need=need(tree) + base, nargs=3 if w else 2))

    for i, op in enumerate(UN_OPS):
        x = z[f"un_x_{dt}"][z["un_set"][i]]
        for k in UN_BASES:
            add(f"p@{k}", "un", op, "nat", k, N(op, P()), "a", None, (k, k, 0))
        add("t@0", "un", op, "nat", 0, N(op, T_()), None, "a", (0, 0, 0))
        for j in CONST_ROWS:
            add(f"C@{j}", "un", op, "const", 0, N(op, C(x[j])), "a", None, (0, 0, 0), row=j)
    for i, op in enumerate(BIN_OPS):
        s = z["bin_set"][i]
        a, b = z[f"bin_a_{dt}"][s], z[f"bin_b_{dt}"][s]
        for k in BIN_BASES:
            add(f"pt@{k}", "bin", op, "nat", k, N(op, P(), T_()), "a", "b", (k, k, k + 1))
            add(f"tp@{k}", "bin", op, "nat", k, N(op, T_(), P()), "b", "a", (k, k, k + 1))
        for k in SWAP_BASES:
            add(f"p(t1)@{k}", "bin", op, "swap", k, N(op, P(), N("*", T_(), C(1.0))), "a", "b", (k, k + 1, k))
            add(f"t(p1)@{k}", "bin", op, "swap", k, N(op, T_(), N("*", P(), C(1.0))), "b", "a", (k, k + 1, k))
        for j in CONST_ROWS:
            add(f"pC@{j}", "bin", op, "const", 0, N(op, P(), C(b[j])), "a", None, (0, 0, 1), row=j)
            add(f"Cp@{j}", "bin", op, "const", 0, N(op, C(a[j]), P()), "b", None, (0, 0, 1), row=j)
        add("pw", "bin", op, "weight", 0, N(op, P(), W()), "a", None, (0, 0, 1), w="b")
        add("wp", "bin", op, "weight", 0, N(op, W(), P()), "b", None, (0, 0, 1), w="a")
    _FORMS[dt] = out
    return out


def expr(form):
    """The form's ExprLoss, made once."""
    if "loss" not in form:
        form["loss"] = srhip.ExprLoss(form["tree"], options())
        assert form["loss"].nargs == form["nargs"]
    return form["loss"]


def operands(kind, op, dt, which):
    """(a, b or None, tabulated values, rows that count) of one operator: which = "general" (191 points) or
    "special" (the special block, with the table's mask)."""
    z = fv.table()
    if kind == "un":
        i = UN_OPS.index(op)
        if which == "general":
            return z[f"un_x_{dt}"][z["un_set"][i]], None, z[f"un_y_{dt}"][i], np.ones(fv.P, bool)
        return z[f"un_sx_{dt}"], None, z[f"un_sy_{dt}"][i], z[f"un_sm_{dt}"][i].astype(bool)
    i = BIN_OPS.index(op)
    if which == "general":
        s = z["bin_set"][i]
        return z[f"bin_a_{dt}"][s], z[f"bin_b_{dt}"][s], z[f"bin_y_{dt}"][i], np.ones(fv.P, bool)
    return z[f"bin_sa_{dt}"], z[f"bin_sb_{dt}"], z[f"bin_sy_{dt}"][i], z[f"bin_sm_{dt}"][i].astype(bool)


def columns(form, dt, which):
    """(pred, y, w or None, tabulated values, rows that count) of one form on one block: an argument that
    carries no operand is a column of zeros; a constant form counts only its own general row."""
    a, b, want, mask = operands(form["kind"], form["op"], dt, which)
    col = {"a": a, "b": b, None: np.zeros(len(a), NP[dt])}
    if form["row"] is not None:
        mask = mask & (np.arange(len(a)) == form["row"]) if which == "general" else np.zeros(len(a), bool)
    return col[form["p"]], col[form["t"]], (col[form["w"]] if form["w"] else None), want, mask


def host_values(form, pred, y, w=None):
    """srhip_loss_expr_eval_host of the form's program."""
    return expr(form)(pred, y, w) if form["w"] else expr(form)(pred, y)


def instruction_under_test(form, dt):
    """((op, dst, a, b), need) of the compiled program's instruction under test."""
    ins, nd = expr(form).instructions(NP[dt])
    op, dst, a, b, _ = ins[len(ins) - 1 - form["base"]]
    return (op, dst, a, b), nd


def worst_ulp(got, want, mask):
    """Worst error in ulp over the rows that count where both values are finite."""
    m = mask & np.isfinite(want) & np.isfinite(got)
    return float(fv.ulp_distance(np.ascontiguousarray(got), np.ascontiguousarray(want))[m].max()) if m.any() else 0.0


# ---- the forms over the derivative table ----------------------------------------------------------------------
_GRAD_FORMS = {}


def grad_forms(dt):
    """Forms whose d l / d p is one tabulated partial, as dicts: label, name (the rule, for reports), op, tree,
    p / t (the prediction's and the target's column, [300] in T; the target of a unary form is zeros), want
    (the partial in Float64), exact (a partial that is exactly 0 or +-1, or `*`'s: bit-exact), base, order.
    op(p) is the unary rule; p op t gives d/da, t op p gives d/db; swapped orders and bases as in forms()."""
    if dt in _GRAD_FORMS:
        return _GRAD_FORMS[dt]
    out = []

    def add(label, name, op, order, base, tree, p, t, want, exact):
        out.append(dict(label=f"{name}.{label}", name=name, op=op, order=order, base=base, tree=at_base(tree, base), p=p, t=t,
                        want=want, exact=exact, nargs=2))

    for op in dr.UN_OPS:
        X, df = dr.unary_inputs(op, dt)
        for k in UN_BASES:
            add(f"p@{k}", op, op, "nat", k, N(op, P()), X[0], np.zeros_like(X[0]), df, op in dr.EXACT_UN)
    for case in dr.BIN_CASES:
        a, b, fa, fb = dr.binary_inputs(case, dt)
        op = dr.binop_name(case)
        exact = case in dr.EXACT_BIN or case == "*"
        for k in BIN_BASES:
            add(f"pt@{k}", case, op, "nat", k, N(op, P(), T_()), a, b, fa, exact)
            add(f"tp@{k}", case, op, "nat", k, N(op, T_(), P()), b, a, fb, exact)
        for k in SWAP_BASES:
            add(f"p(t1)@{k}", case, op, "swap", k, N(op, P(), N("*", T_(), C(1.0))), a, b, fa, exact)
            add(f"t(p1)@{k}", case, op, "swap", k, N(op, T_(), N("*", P(), C(1.0))), b, a, fb, exact)
    _GRAD_FORMS[dt] = out
    return out


def shifted_tree():
    """x1 + 0.5 (tests/derivative_rules_common.py): over the feature x - 0.5 the prediction is the tabulated x
    exactly (every input is a grid point below 8) and d pred / d c is exactly 1."""
    return N("+", srhip.Node(feature=1), C(0.5))


# ---- row positions (test (c)) ---------------------------------------------------------------------------------
POSITION_SIZES = (50, 257, 4096 + 65)
DEEP = ("neg.p@5", "log.p@5", "sin.p@5", "-.pt@4", "atan2.tp@4")   # each class at the deepest base, both kinds


def position_forms(dt):
    """Every operator once at base 0, every binary operator once in swapped order, each operator class once at
    the deepest base."""
    pick = {f"{op}.p@0" for op in UN_OPS} | {f"{op}.pt@0" for op in BIN_OPS} | {f"{op}.p(t1)@0" for op in BIN_OPS}
    pick |= set(DEEP)
    sel = [f for f in forms(dt) if f["label"] in pick]
    assert len(sel) == len(pick)
    return sel


GRAD_DEEP = ("tanh.p@5", "abs.p@5", "/.tp@4", "-.pt@4")


def position_grad_forms(dt):
    """Every rule once at base 0, every binary case once in swapped order (there d/db), smooth and exact rules
    once at the deepest base."""
    pick = {f"{op}.p@0" for op in dr.UN_OPS} | {f"{c}.pt@0" for c in dr.BIN_CASES} | {f"{c}.t(p1)@0" for c in dr.BIN_CASES}
    pick |= set(GRAD_DEEP)
    sel = [f for f in grad_forms(dt) if f["label"] in pick]
    assert len(sel) == len(pick)
    return sel


def small_rows(values, bound_rows):
    """How many of `values` (one set's per-row losses) lie under m 2^-28 sum|l|: rows whose last Float32 bit
    the derived bound m 2^-52 sum|l| / m on the mean cannot see."""
    v = np.abs(np.asarray(values, np.float64))
    return int((v < bound_rows * 2.0 ** -28 * v.sum()).sum())


def position_points(op, kind, dt, max_rows=5120):
    """The general points that test (c) tiles for one operator, from the table alone.  An exact-class operator
    keeps the points whose tabulated |value| is at least m 2^-28 sum|l| for every tiling up to max_rows rows
    (5120: the largest row set of a one-feature Float32 dataset), so that in Float32 the derived bound resolves
    one ulp of every row; an odd number of them, so that a cyclic tiling walks each point through every lane,
    register row and pass.  The general points span 36 binades, so `square cube /` keep the upper few.  Every
    other operator keeps all 191 (exp, sinh, gamma, ^ ... would keep one point): the bound then sees the large
    rows only, and the test prints how many rows lie under it."""
    want = np.abs(operands(kind, op, dt, "general")[2].astype(np.float64))
    assert np.isfinite(want).all()
    if fv.GEN.op_class(op) != "exact":
        return np.arange(fv.P)
    keep = np.nonzero(want > 0)[0]
    while True:
        # a tiling of m rows holds each point at most m / len + 1 times
        thr = max_rows * 2.0 ** -28 * (max_rows / len(keep) + 1) * want[keep].sum()
        nxt = keep[want[keep] >= thr]
        if len(nxt) % 2 == 0:
            nxt = nxt[nxt != nxt[np.argmin(want[nxt])]]
        if len(nxt) == len(keep):
            return keep
        keep = nxt
