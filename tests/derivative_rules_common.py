"""Shared by tests/test_oracle_grad_rules.py (no device) and tests/test_gpu_derivative_rules.py: the golden
table of exact derivatives and the trees that put every rule of csrc/srhip_grad_impl.h, in every operand
form of csrc/srhip_grad_tile.inc, in front of it.  Not a test module.

Operand forms (csrc/srhip_compile.cpp emit; a gradient program has no leaf-leaf superinstructions at the
build's default SRHIP_GRAD_SUPER_LEVEL, and never folds a constant subtree, whose constants need tangents):
a binary operator whose right operand is a leaf runs as `A op X` / `A op c` after its left operand was
left in the accumulator A (a leaf left operand is loaded into A first), one whose left operand alone is a
leaf as `X op A` / `c op A`, and one of two subtrees as `S[k] op A`, or `A op S[k]` when the right subtree
needs the deeper stack and is therefore evaluated first; k is the number of enclosing operators that were
themselves evaluated second.  The heavy operators (^ mod atan2) take a leaf operand through a stack slot.
"""
import importlib.util
import os

import numpy as np

from conftest import GOLDEN

EPS = {"f32": float(np.finfo(np.float32).eps), "f64": float(np.finfo(np.float64).eps)}
NP = {"f32": np.float32, "f64": np.float64}
BAR = 128  # eps(T), relative: see test_unary_domain_is_well_conditioned


def _rules_module():
    spec = importlib.util.spec_from_file_location("make_derivative_rules",
                                                  os.path.join(GOLDEN, "make_derivative_rules.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RULES = _rules_module()
UN_OPS = [o for o, _ in RULES.UN_OPS]
BIN_CASES = [c for c, _ in RULES.BIN_CASES]
LOSS_KINDS = RULES.DIST + RULES.MARG
# derivatives that are exactly 0 or +-1 (times an operand, for *): bit-exact on every path
EXACT_UN = {"neg", "abs", "relu", "sign", "floor", "ceil", "round"}
EXACT_BIN = {"+", "-", "mod", "max", "min", "greater", "cond", "logical_or", "logical_and"}
CONST_ROWS = (0, 100, 255, 299)  # rows whose operand a constant form's constant restates (block end, tail end)

_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = RULES.load_table()
        assert list(_TABLE["un_ops"]) == UN_OPS and list(_TABLE["bin_cases"]) == BIN_CASES
        assert list(_TABLE["loss_kinds"]) == LOSS_KINDS
    return _TABLE


def rel_err(got, want):
    """|got - want| / |want| (an exact zero must be matched exactly: 0 there, inf otherwise)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(got - want) / np.abs(want)
    return np.where(want == 0, np.where(got == 0, 0.0, np.inf), e)


def binop_name(case):
    return case.replace("^neg", "^")


def loss_object(sr, kind):
    cls = getattr(sr, kind + "Loss", None) or getattr(sr, kind + "DistLoss")
    return cls(RULES.LOSS_P0[kind]) if kind in RULES.LOSS_P0 else cls()


# ---- unary ------------------------------------------------------------------------------------------
def unary_inputs(op, dt):
    """(X [3, 300] = (x, x / 2, 0), U'(x) [300]) for one operator."""
    z = table()
    i = UN_OPS.index(op)
    x = z[f"un_x_{dt}"][z["un_dom"][i]]
    return np.stack([x, x / NP[dt](2), np.zeros_like(x)]), z[f"un_df_{dt}"][i]


def unary_trees(sr, op, x):
    """U(x1); U(2 * x2) (x2 = x1 / 2: the same argument, exactly); U(c) * x1 for two tabulated c, the
    constant-subtree form that is evaluated once per lane; U(x1) * 2, an operator of a feature in a tree
    with a constant: what a constant-gradient launch reads from the derived view (csrc/srhip_host.cpp
    grad_derived_spec) when the operator is not an inline one."""
    N = sr.Node
    x1, x2 = N(feature=1), N(feature=2)
    return [N(op, x1), N(op, N("*", N(val=2.0), x2)),
            N("*", N(op, N(val=float(x[0]))), x1), N("*", N(op, N(val=float(x[-1]))), x1),
            N("*", N(op, N(feature=1)), N(val=2.0))]


# the operators whose gradient rule is inlined (csrc/srhip_isa.h un_grad_inline): never derived columns
INLINE_UN = {"neg", "square", "cube", "abs", "relu", "sign", "round", "floor", "ceil"}


# ---- binary -----------------------------------------------------------------------------------------
def binary_inputs(case, dt):
    """(a, b, dB/da, dB/db) [300] each."""
    z = table()
    i = BIN_CASES.index(case)
    s = z["bin_set"][i]
    return z[f"bin_a_{dt}"][s], z[f"bin_b_{dt}"][s], z[f"bin_fa_{dt}"][i], z[f"bin_fb_{dt}"][i]


def _zero(sr, depth):
    """A subtree that is 0 on every row and needs `depth` stack slots: sums of the constant subtree
    0.0 + 0.0 (a gradient program keeps it: need 0), 2^depth of them."""
    N = sr.Node
    if depth == 0:
        return N("+", N(val=0.0), N(val=0.0))
    return N("+", _zero(sr, depth - 1), _zero(sr, depth - 1))


def binary_trees(sr, case, a, b):
    """Every operand form of one binary operator B, as a list of (form, dataset, tree, rows, var, const):

    dataset 0 has the features (a - 0.5, b, b - 0.5), dataset 1 (a, b, b - 0.5): `x + 0.5` has derivative
    exactly 1 and restores the tabulated operand exactly, so each partial of B appears unscaled.
    rows: None (every row sees tabulated operands) or the one row j whose operand the tree's constant is.
    var: per feature, which partial d tree / d x_f is ("a", "b") or None for exactly 0.
    const: per constant in get_constants order, "a", "b", or 1 for a derivative of exactly 1; for the
    constant-subtree form B(c1, c2) * x1 the partials are scaled by x1 ("ax", "bx").
    """
    N = sr.Node
    op = binop_name(case)
    x1, x2, x3 = (lambda: N(feature=1)), (lambda: N(feature=2)), (lambda: N(feature=3))
    A = lambda: N("+", x1(), N(val=0.5))   # noqa: E731  dataset 0: a
    Bn = lambda: N("+", x3(), N(val=0.5))  # noqa: E731  b
    out = [
        ("AF", 0, N(op, A(), x2()), None, ("a", "b", None), ("a",)),
        ("SA0", 0, N(op, A(), Bn()), None, ("a", None, "b"), ("a", "b")),
        # the right operand needs one slot, the left none: right first, then `A op S[0]`
        ("AS0", 0, N(op, A(), N("+", N("+", x3(), N(val=0.25)), N("+", N(val=0.25), N(val=0.0)))), None,
         ("a", None, "b"), ("a", "b", "b", "b")),
        ("FA", 1, N(op, x1(), Bn()), None, ("a", None, "b"), ("b",)),
        ("FF", 1, N(op, x1(), x2()), None, ("a", "b", None), ()),
    ]
    # a right-leaning ladder Z3 + (Z2 + (Z1 + B(..))): each Z needs as many slots as what follows it, so it
    # goes first and B's operands land in slots 1, 2, 3
    for k in (1, 2, 3):
        t = N(op, A(), Bn())
        for d in range(1, k + 1):
            t = N("+", _zero(sr, d), t)
        nz = sum(2 ** (d + 1) for d in range(1, k + 1))
        out.append((f"SA{k}", 0, t, None, ("a", None, "b"), (1,) * nz + ("a", "b")))
    for j in CONST_ROWS:
        ca, cb = float(a[j]), float(b[j])
        out += [
            (f"AC@{j}", 0, N(op, A(), N(val=cb)), j, ("a", None, None), ("a", "b")),
            (f"CA@{j}", 0, N(op, N(val=ca), Bn()), j, (None, None, "b"), ("a", "b")),
            (f"CF@{j}", 0, N(op, N(val=ca), x2()), j, (None, "b", None), ("a",)),
            (f"FC@{j}", 1, N(op, x1(), N(val=cb)), j, ("a", None, None), ("b",)),
            (f"CC@{j}", 1, N("*", N(op, N(val=ca), N(val=cb)), x1()), j, None, ("ax", "bx")),
        ]
    return out


def uniform_trees(sr, case, a, b):
    """The once-per-lane variants of the tile (an operator whose operands are constant subtrees), each with
    its own operand order: (form, tree, row j, const) with const as in binary_trees, every tree times x1.
    `A op c` (two constant leaves), `c op A` (c1, c2 + c3), `S[0] op A` (c1 + c2, c3 + c4) and `A op S[0]`
    (the right constant subtree needs a slot, so it goes first); the sums restore a[j] and b[j] exactly."""
    N = sr.Node
    op = binop_name(case)
    h = 0.5
    out = []
    for j in CONST_ROWS:
        ca, cb = float(a[j]), float(b[j])
        La = lambda: N("+", N(val=ca - h), N(val=h))  # noqa: E731
        Rb = lambda: N("+", N(val=cb - h), N(val=h))  # noqa: E731
        Rb2 = lambda: N("+", N("+", N(val=cb - h), N(val=0.25)), N("+", N(val=0.25), N(val=0.0)))  # noqa: E731
        for form, t, const in (("uAC", N(op, N(val=ca), N(val=cb)), ("ax", "bx")),
                               ("uCA", N(op, N(val=ca), Rb()), ("ax", "bx", "bx")),
                               ("uSA0", N(op, La(), Rb()), ("ax", "ax", "bx", "bx")),
                               ("uAS0", N(op, La(), Rb2()), ("ax", "ax", "bx", "bx", "bx", "bx"))):
            out.append((f"{form}@{j}", N("*", t, N(feature=1)), j, const))
    return out


def binary_datasets(a, b):
    h = a.dtype.type(0.5)
    return [np.stack([a - h, b, b - h]), np.stack([a, b, b - h])]


def binary_options(sr, case):
    return sr.Options(binary_operators=tuple(dict.fromkeys(("+", "*", binop_name(case)))), unary_operators=())


# ---- populations ------------------------------------------------------------------------------------
def all_operator_population(sr, dt):
    """Every tree of the two rule tests above that has a constant, gamma's included, over one operator
    set and one dataset (features in [0.5, 1.5]: some trees leave their domain there and fail, on every
    path alike)."""
    T = NP[dt]
    opts = sr.Options(binary_operators=tuple(dict.fromkeys(binop_name(c) for c in BIN_CASES)),
                      unary_operators=tuple(UN_OPS) + ("gamma",))
    trees = []
    for op in UN_OPS + ["gamma"]:
        x = unary_inputs(op, dt)[0][0] if op != "gamma" else np.array([1.5, 2.5], T)
        trees += unary_trees(sr, op, x)[1:]
    for case in BIN_CASES:
        a, b, _, _ = binary_inputs(case, dt)
        trees += [f[2] for f in binary_trees(sr, case, a, b) if f[5] and "@" not in f[0] or f[0].endswith("@100")]
        trees += [f[1] for f in uniform_trees(sr, case, a, b) if f[0].endswith("@100")]
    rng = np.random.default_rng(11)
    X = rng.uniform(0.5, 1.5, (3, 300)).astype(T)
    y = (X[0] * X[1] - X[2]).astype(T)
    nodes, offs = sr.flatten(trees, opts, T)
    return opts, nodes, offs, X, y


COMPOSITION_SEED = 141


def composition_problem(sr):
    """48 random Float64 trees over every operator but gamma, sizes uniform in 1 .. 14 (max_size 14), 300
    rows, features in [0.5, 1.5].  The reference's tree generator with one change: a new operator node is
    binary with probability 1/2 instead of 13/45 (the operator counts), since chains of unary operators
    have one leaf and so at most one constant -- too few to compare 60 gradient components."""
    from srhip import random_trees as rt
    from srhip.node import count_nodes

    opts = sr.Options(binary_operators=tuple(dict.fromkeys(binop_name(c) for c in BIN_CASES)),
                      unary_operators=tuple(UN_OPS))
    rng = np.random.default_rng(COMPOSITION_SEED)
    trees = []
    for size in rng.integers(1, 15, size=48):
        tree = rt.make_random_leaf(3, np.float64, rng)
        while count_nodes(tree) < size:
            binary = count_nodes(tree) < size - 1 and rng.random() < 0.5
            tree = rt.append_random_op(tree, opts, 3, np.float64, rng, make_new_bin_op=bool(binary))
        trees.append(tree)
    nodes, offs = sr.flatten(trees, opts, np.float64)
    X = rng.uniform(0.5, 1.5, (3, 300))
    y = X[0] * X[1] - np.cos(X[2])
    return opts, nodes, offs, X, y


def composition_reference(sr, oracle):
    """Per tree: None, or the oracle's exact gradient where the oracle evaluates the tree as ok and the tree
    has a constant (the gradient may hold Inf or NaN: the caller counts those trees)."""
    opts, nodes, offs, X, y = composition_problem(sr)
    ref = []
    for t in range(len(offs) - 1):
        tn = nodes[offs[t]:offs[t + 1]].copy()
        _, _, ok = oracle.eval_loss(tn, opts.binop_codes, opts.unaop_codes, X, y)
        g = oracle.loss_grad(tn, opts.binop_codes, opts.unaop_codes, X, y) if ok else np.zeros(0)
        ref.append(g if ok and g.size else None)
    return ref
