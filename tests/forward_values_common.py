"""Shared by tests/test_forward_values_table.py (no device) and tests/test_gpu_forward_values.py: the golden
table of exact forward values (tests/golden/make_forward_values.py) and the trees that put every operator, in
every operand form of the interpreter (csrc/srhip_eval_impl.h), in front of it.  Not a test module.

Operands reach the operator under test unchanged: straight from feature columns, or through identities that
are exact for every value, -0.0, subnormals, Inf and NaN included:

    I(x)  = x * ones                 a feature column of 1.0; makes the operand a subtree (stack need 0)
    R1(x) = cond(ones * ones, I(x))  the same value from a subtree that needs one stack slot
    NN(x) = neg(neg(x))              a subtree whose code begins with a feature load (fuses with a push)

Stack slots (csrc/srhip_compile.cpp emit): an operator of two subtrees evaluates the one with the larger need
first (the left one on a tie), pushes it to slot `base` and evaluates the other at base + 1; so a tree T sits
at base k inside k nested cond(G, .) whose left sides G are products of ones that need as many slots as what
they guard: cond(G(n), T) with need(T) = n evaluates G first, pushes it, runs T one slot up and returns T's
value (G = 1 > 0).  Constant subtrees are folded in evaluation programs, so depth is built from features.
"""
import importlib.util
import os

import numpy as np

from conftest import GOLDEN


def _gen_module():
    spec = importlib.util.spec_from_file_location("make_forward_values", os.path.join(GOLDEN, "make_forward_values.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _gen_module()
P = GEN.P
NP = {"f32": np.float32, "f64": np.float64}
UN_OPS = [o for o, _ in GEN.UN_OPS]
BIN_OPS = [o for o, _ in GEN.BIN_OPS]
WIDE = ("asin", "acos", "atanh_clip")          # csrc/srhip_isa.h un_wide_op: the K = 8 kernels only
HEAVY = ("^", "mod", "atan2")
SPEC = [o for o in BIN_OPS if o not in HEAVY]
CONST_ROWS = (0, 100, 190)  # general rows whose operand a constant form's constant restates (first, middle, last)
NUN = len(GEN.UN_SETS)
ONES = NUN + 2 * len(GEN.BIN_SETS) + 1          # the feature (1-based) that is 1.0 on every row
NFEAT = ONES
TILED_ROWS = {"f32": 4096 + 65, "f64": 3 * 256 + 7}
# the project's bars (tests/test_gpu_parity.py test_all_operators_single_values)
F64_RTOL, F64_RTOL_LOOSE, ATOL = 1e-14, 1e-13, 1e-30

_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = GEN.load_table()
        assert list(_TABLE["un_ops"]) == UN_OPS and list(_TABLE["bin_ops"]) == BIN_OPS
    return _TABLE


def un_feature(op):
    return 1 + int(table()["un_set"][UN_OPS.index(op)])


def bin_features(op):
    s = int(table()["bin_set"][BIN_OPS.index(op)])
    return NUN + 1 + 2 * s, NUN + 2 + 2 * s


def op_class(op, dt):
    """exact / rounded / ulp1 for Float32; exact / rel for Float64."""
    c = GEN.op_class(op)
    return c if (dt == "f32" or c == "exact") else "rel"


class Data:
    """One dataset: X [NFEAT, n], per operator the tabulated values and the mask of rows that count, and per
    row the general point it repeats (src, -1 for a special point)."""


_DATA = {}


def data(dt, which):
    """which: "general" (P rows), "tiled" (the P points cyclically: 4096 + 65 rows in Float32, which puts a
    K = 2 program on the R = 16 kernel with a ragged last tile; 3 * 256 + 7 in Float64), "special" (the
    special block, padded with general points)."""
    if (dt, which) in _DATA:
        return _DATA[dt, which]
    z = table()
    T = NP[dt]
    d = Data()
    if which == "special":
        ns, nb = len(z[f"un_sx_{dt}"]), len(z[f"bin_sa_{dt}"])
        n = max(ns, nb) + 9

        def cat(special, general, fill):
            m = n - special.shape[-1]
            return np.concatenate([special, general[..., :m]], axis=-1), np.concatenate(
                [fill, np.ones(general[..., :m].shape, bool)], axis=-1)

        ucols = [cat(z[f"un_sx_{dt}"], z[f"un_x_{dt}"][s], np.ones(ns, bool))[0] for s in range(NUN)]
        d.un_want, d.un_mask = cat(z[f"un_sy_{dt}"], z[f"un_y_{dt}"], z[f"un_sm_{dt}"])
        bcols = []
        for s in range(len(GEN.BIN_SETS)):
            bcols += [cat(z[f"bin_sa_{dt}"], z[f"bin_a_{dt}"][s], np.ones(nb, bool))[0],
                      cat(z[f"bin_sb_{dt}"], z[f"bin_b_{dt}"][s], np.ones(nb, bool))[0]]
        d.bin_want, d.bin_mask = cat(z[f"bin_sy_{dt}"], z[f"bin_y_{dt}"], z[f"bin_sm_{dt}"])
        d.un_src = np.concatenate([np.full(ns, -1), np.arange(n - ns)])
        d.bin_src = np.concatenate([np.full(nb, -1), np.arange(n - nb)])
    else:
        n = P if which == "general" else TILED_ROWS[dt]
        idx = np.arange(n) % P
        ucols = [z[f"un_x_{dt}"][s][idx] for s in range(NUN)]
        bcols = []
        for s in range(len(GEN.BIN_SETS)):
            bcols += [z[f"bin_a_{dt}"][s][idx], z[f"bin_b_{dt}"][s][idx]]
        d.un_want, d.bin_want = z[f"un_y_{dt}"][:, idx], z[f"bin_y_{dt}"][:, idx]
        d.un_mask, d.bin_mask = np.ones(d.un_want.shape, bool), np.ones(d.bin_want.shape, bool)
        d.un_src = d.bin_src = idx
    d.n = n
    d.X = np.ascontiguousarray(np.stack(ucols + bcols + [np.ones(n, T)]).astype(T))
    assert d.X.shape == (NFEAT, n)
    _DATA[dt, which] = d
    return d


def expected(d, tree):
    """(tabulated values [n], rows that count [n]) of one tree of build_trees on dataset d."""
    if tree["kind"] == "un":
        i = UN_OPS.index(tree["op"])
        want, mask, src = d.un_want[i], d.un_mask[i], d.un_src
    else:
        i = BIN_OPS.index(tree["op"])
        want, mask, src = d.bin_want[i], d.bin_mask[i], d.bin_src
    if tree["row"] is not None:
        mask = mask & (src == tree["row"])
    return want, mask


# ---- comparison -------------------------------------------------------------------------------------------
def _ordered(a):
    """Floats as integers in value order (np.longdouble: exact for 64-bit integers)."""
    i = a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]).astype(np.int64)
    lo = np.int64(np.iinfo({4: np.int32, 8: np.int64}[a.dtype.itemsize]).min)
    return np.where(i < 0, lo - i, i).astype(np.longdouble)


def ulp_distance(got, want):
    """Units in the last place between two arrays of one float type (NaN where either is NaN)."""
    d = np.abs(_ordered(got) - _ordered(want)).astype(np.float64)
    return np.where(np.isnan(got) | np.isnan(want), np.nan, d)


def bits_equal(got, want):
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return got.view(u) == want.view(u)


def failing_rows(op, dt, got, want, mask):
    """Rows (indices) of `got` that miss the operator's class bar against `want`; NaN exactly where the
    table has NaN in every class."""
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    cls = op_class(op, dt)
    nan_ok = np.isnan(got) == np.isnan(want)
    both = np.isnan(got) & np.isnan(want)
    if cls in ("exact", "rounded"):
        ok = bits_equal(got, want) | both
    elif cls == "ulp1":
        with np.errstate(invalid="ignore"):
            ok = (ulp_distance(got, want) <= 1) | both
    else:
        rtol = F64_RTOL_LOOSE if op in ("gamma", "^") else F64_RTOL
        with np.errstate(invalid="ignore", over="ignore"):
            ok = (got == want) | (np.abs(got - want) <= ATOL + rtol * np.abs(want)) | both
    return np.nonzero(mask & ~(ok & nan_ok))[0]


# ---- trees ------------------------------------------------------------------------------------------------
def build_trees(sr, dt, un_ops=None, bin_ops=None, consts=None):
    """Every operand form of every operator, as dicts {label, kind, op, tree, row, need}: row is None (every
    row sees tabulated operands) or the general row whose operand the tree's constant restates; need is the
    tree's stack need (checked against the compiled program by the table test).

    consts(kind, op, j) -> operand constants of general row j; by default from the table of dtype dt."""
    N = sr.Node
    un_ops = UN_OPS if un_ops is None else un_ops
    bin_ops = BIN_OPS if bin_ops is None else bin_ops
    z = table() if consts is None else None

    def cvals(kind, op, j):
        if consts is not None:
            return consts(kind, op, j)
        if kind == "un":
            return (float(z[f"un_x_{dt}"][z["un_set"][UN_OPS.index(op)]][j]),)
        s = z["bin_set"][BIN_OPS.index(op)]
        return float(z[f"bin_a_{dt}"][s][j]), float(z[f"bin_b_{dt}"][s][j])

    F = lambda f: N(feature=f)                       # noqa: E731
    one = lambda: F(ONES)                            # noqa: E731
    I = lambda t: N("*", t, one())                   # noqa: E731,E741
    NN = lambda t: N("neg", N("neg", t))             # noqa: E731

    def G(n):
        return N("*", one(), one()) if n == 0 else N("*", G(n - 1), G(n - 1))

    R1 = lambda t: N("cond", G(0), I(t))             # noqa: E731

    def at_base(t, need, k):
        for _ in range(k):
            t = N("cond", G(need), t)
            need += 1
        return t, need

    out = []

    def add(label, kind, op, tree, row=None, need=0):
        out.append(dict(label=f"{op}.{label}", kind=kind, op=op, tree=tree, row=row, need=need))

    for op in un_ops:
        f = un_feature(op)
        add("F", "un", op, N(op, F(f)))
        add("F2", "un", op, N(op, F(f)))             # a second use: U(x) becomes a derived column where it can
        add("A", "un", op, N(op, I(F(f))))           # of an operator output (cos / sin: the UN_NC_FLAG form)
        for j in CONST_ROWS:
            add(f"C@{j}", "un", op, N(op, N(val=cvals("un", op, j)[0])), row=j)  # the host constant folder
    for op in bin_ops:
        fa, fb = bin_features(op)
        a, b = (lambda: F(fa)), (lambda: F(fb))
        heavy = op in HEAVY
        h = 1 if heavy else 0  # a heavy operator's leaf operand goes through a stack slot
        add("FF", "bin", op, N(op, a(), b()), need=h)
        for j in CONST_ROWS:
            ca, cb = cvals("bin", op, j)
            add(f"AC@{j}", "bin", op, N(op, I(a()), N(val=cb)), row=j, need=h)
            add(f"CA@{j}", "bin", op, N(op, N(val=ca), I(b())), row=j, need=h)
            add(f"FC@{j}", "bin", op, N(op, a(), N(val=cb)), row=j, need=h)
            add(f"CF@{j}", "bin", op, N(op, N(val=ca), b()), row=j, need=h)
            add(f"CC@{j}", "bin", op, N(op, N(val=ca), N(val=cb)), row=j)            # the host constant folder
        for k in range(8):
            # A op X / X op A, or for a heavy operator SLOADF k with A op S[k] / S[k] op A
            for form, t in (("AF", N(op, I(a()), b())), ("FA", N(op, a(), I(b())))):
                if heavy or k == 0:
                    tree, need = at_base(t, h, k) if k else (t, h)
                    add(f"{form}{k}" if heavy else form, "bin", op, tree, need=need)
            if heavy:
                j = CONST_ROWS[k % len(CONST_ROWS)]
                ca, cb = cvals("bin", op, j)
                for form, t in ((f"SLC.CA{k}@{j}", N(op, N(val=ca), I(b()))), (f"SLC.AC{k}@{j}", N(op, I(a()), N(val=cb)))):
                    tree, need = at_base(t, 1, k)
                    add(form, "bin", op, tree, row=j, need=need)
            # S[k] op A after PUSH k; A op S[k] after PUSHLF k (the right side needs the deeper stack: it goes first)
            tree, need = at_base(N(op, I(a()), I(b())), 1, k)
            add(f"SA{k}", "bin", op, tree, need=need)
            tree, need = at_base(N(op, NN(a()), R1(b())), 1, k)
            add(f"AS{k}", "bin", op, tree, need=need)
    # PUSHLC k: a push followed by a constant load, which only a heavy operator with a constant left leaf and a
    # feature right leaf emits (it then needs slot k + 1: k = 7 cannot be compiled)
    hv = [o for o in bin_ops if o in HEAVY]
    for k in range(7 if hv else 0):
        op = hv[k % len(hv)]
        j = CONST_ROWS[k % len(CONST_ROWS)]
        fa, fb = bin_features(op)
        tree, need = at_base(N("cond", G(1), N(op, N(val=cvals("bin", op, j)[0]), F(fb))), 2, k)
        add(f"PUSHLC{k}@{j}", "bin", op, tree, row=j, need=need)
    return out


def options(sr, wide):
    una = [o for o in UN_OPS if wide or o not in WIDE]
    return sr.Options(binary_operators=tuple(BIN_OPS), unary_operators=tuple(una))


def select(trees, K):
    """The trees of the program that must run in the K-slot kernels: need <= 2 without the wide operators,
    need <= 4 without them, everything (the wide operators exist only in the K = 8 kernels)."""
    if K == 8:
        return list(trees)
    sel = [t for t in trees if t["need"] <= K and t["op"] not in WIDE]
    return sel[::-1] if K == 4 else sel  # (reversed: other operators' U(x) fill the 16 derived columns)


_PROGRAMS = {}


def program_nodes(sr, dt, K):
    """(options, selected trees, nodes, offsets) of the (dtype, K) program; flattened once."""
    if (dt, K) not in _PROGRAMS:
        if ("trees", dt) not in _PROGRAMS:
            _PROGRAMS["trees", dt] = build_trees(sr, dt)
        sel = select(_PROGRAMS["trees", dt], K)
        opts = options(sr, wide=K == 8)
        nodes, offs = sr.flatten([t["tree"] for t in sel], opts, NP[dt])
        _PROGRAMS[dt, K] = (opts, sel, nodes, offs)
    return _PROGRAMS[dt, K]


def handler_names(sr):
    return [sr.isa_handler_name(h) for h in range(sr.isa_handler_count())]


def slot_of(name):
    """The stack slot a handler name addresses, or None."""
    return int(name[-1]) if name[-1].isdigit() and not name.startswith("UN.") else None


# ---- Int32 ------------------------------------------------------------------------------------------------
INT_UN = ["neg", "square", "cube", "abs", "relu", "sign"]
INT_BIN = ["+", "-", "*", "greater", "cond", "logical_or", "logical_and", "max", "min"]
INT_ROWS = 67


def int_inputs():
    """(a, b) [INT_ROWS] Int32: the edge values in every pairing that fits, then random values."""
    lo, hi = -2 ** 31, 2 ** 31 - 1
    edge = [lo, lo + 1, -1, 0, 1, 46340, 46341, 1290, 1291, hi]
    rng = np.random.default_rng(32)
    a = edge + list(rng.integers(lo, hi, INT_ROWS - len(edge), endpoint=True))
    b = [edge[(i * 3 + 1) % len(edge)] for i in range(len(edge))] + list(
        rng.integers(lo, hi, INT_ROWS - len(edge), endpoint=True))
    perm = rng.permutation(INT_ROWS - 2 * len(edge))
    b[2 * len(edge):] = [edge[i % len(edge)] for i in perm]  # random a against edge b too
    return np.array(a, np.int32), np.array(b, np.int32)


def _wrap(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def int_reference(op, a, b=None):
    """Python integers wrapped to 32 bits (Julia Int32 arithmetic)."""
    a = int(a)
    if b is None:
        return _wrap({"neg": -a, "square": a * a, "cube": _wrap(a * a) * a, "abs": abs(a), "relu": max(a, 0),
                      "sign": (a > 0) - (a < 0)}[op])
    b = int(b)
    return _wrap({"+": a + b, "-": a - b, "*": a * b, "greater": int(a > b), "cond": b if a > 0 else 0,
                  "logical_or": int(a > 0 or b > 0), "logical_and": int(a > 0 and b > 0), "max": max(a, b),
                  "min": min(a, b)}[op])


def int_problem(sr):
    """(options, trees, X [NFEAT, INT_ROWS], expected(tree) -> (values, mask)) for Int32: the same operand
    forms over the ring operators; every unary operator reads column a."""
    a, b = int_inputs()
    X = np.ones((NFEAT, INT_ROWS), np.int32)
    X[:NUN] = a
    for s in range(len(GEN.BIN_SETS)):
        X[NUN + 2 * s], X[NUN + 2 * s + 1] = a, b

    def consts(kind, op, j):
        jj = j % INT_ROWS
        return (float(a[jj]),) if kind == "un" else (float(a[jj]), float(b[jj]))

    trees = build_trees(sr, "i32", INT_UN, INT_BIN, consts)
    opts = sr.Options(binary_operators=tuple(INT_BIN), unary_operators=tuple(INT_UN))

    def want(tree):
        if tree["kind"] == "un":
            v = np.array([int_reference(tree["op"], x) for x in a], np.int32)
        else:
            v = np.array([int_reference(tree["op"], x, y) for x, y in zip(a, b)], np.int32)
        mask = np.ones(INT_ROWS, bool) if tree["row"] is None else np.arange(INT_ROWS) == tree["row"] % INT_ROWS
        return v, mask

    return opts, trees, X, want
