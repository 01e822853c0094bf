"""The golden table of exact derivatives (tests/golden/derivative_rules.npz, mpmath at 40 digits) against
the oracle's dual-number gradient (oracle/sr_oracle_grad.h), against its own generator, and against a
working-precision restatement of the device's formulas (the conditioning of the table's domains).
No device: the device side of the same table is tests/test_gpu_derivative_rules.py.
"""
import os

import numpy as np
import pytest

import derivative_rules_common as C
from derivative_rules_common import BIN_CASES, EPS, EXACT_BIN, EXACT_UN, NP, RULES, UN_OPS, rel_err

LN2, LN10, TWO_SQRTPI = 0.69314718055994530942, 2.30258509299404568402, 1.12837916709551257390


@pytest.fixture(scope="module")
def table():
    return C.table()


def test_table_is_complete_and_small(table):
    """33 - 1 unary operators (gamma has no derivative), 13 binary operators (^ twice) and 20 losses,
    300 points each, finite, under 256 KB, and nothing in the file but inputs, expected values and names."""
    import srhip
    from srhip import operators

    assert os.path.getsize(RULES.TABLE) < 256 * 1024
    assert {operators.UNARY[o][0] for o in UN_OPS} | {"gamma"} == {v[0] for v in operators.UNARY.values()}
    assert {operators.BINARY[c.replace("^neg", "^")][0] for c in BIN_CASES} == {v[0] for v in operators.BINARY.values()}
    for k in RULES.DIST + RULES.MARG:
        assert hasattr(srhip, k + "Loss") or hasattr(srhip, k + "DistLoss"), k
    assert len(RULES.DIST) == 9 and len(RULES.MARG) == 11
    allowed = {"un_ops", "un_dom", "bin_cases", "bin_set", "loss_kinds"}
    for dt in ("f32", "f64"):
        allowed |= {f"{p}_{dt}" for p in ("un_x", "un_df", "bin_a", "bin_b", "bin_fa", "bin_fb", "loss_d", "loss_a",
                                          "loss_dl")}
    assert set(table) == allowed
    for k, v in table.items():
        if v.dtype.kind == "f":
            assert v.shape[-1] == 300 and np.all(np.isfinite(v)), k
            assert v.dtype == (NP[k[-3:]] if k.split("_")[1] in ("x", "a", "b", "d") else np.float64), k


def test_table_regenerates_bit_for_bit(table):
    """The committed arrays are what the generator computes now (inputs from its seed, values by mpmath)."""
    pytest.importorskip("mpmath")
    fresh = RULES.build_table()
    assert set(fresh) == set(table)
    for k, v in fresh.items():
        assert v.dtype == table[k].dtype and v.shape == table[k].shape, k
        if v.dtype.kind == "f":
            assert np.array_equal(v.view(np.uint8), np.ascontiguousarray(table[k]).view(np.uint8)), k
        else:
            assert np.array_equal(v, table[k]), k


# ---- the oracle's rules ------------------------------------------------------------------------------
def _one_row_grad(oracle, sr, opts, tree):
    """d tree / d constants at the single row x1 = 1: the L1 gradient with y far below (factor +1)."""
    nodes, _ = sr.flatten([tree], opts, np.float64)
    return oracle.loss_grad(nodes, opts.binop_codes, opts.unaop_codes, np.ones((1, 1)), np.array([-1e6]), kind=1)


@pytest.mark.parametrize("op", UN_OPS)
def test_oracle_unary_rule(oracle, table, op):
    """U(c1 * x1) at x1 = 1: d/dc1 = U'(c1), within 128 eps(Float64) of the table (exactly where it is 0 or
    +-1), at the Float64 inputs and at the Float32 inputs (evaluated in Float64)."""
    import srhip as sr

    opts = sr.Options(binary_operators=("*",), unary_operators=(op,))
    i = UN_OPS.index(op)
    for dt in ("f32", "f64"):
        x = table[f"un_x_{dt}"][table["un_dom"][i]].astype(np.float64)
        got = np.array([_one_row_grad(oracle, sr, opts, sr.Node(1, sr.Node(1, sr.Node(val=v), sr.Node(feature=1))))[0]
                        for v in x])
        err = rel_err(got, table[f"un_df_{dt}"][i])
        assert err.max() <= (0 if op in EXACT_UN else 128 * EPS["f64"]), (dt, err.max() / EPS["f64"])


@pytest.mark.parametrize("case", BIN_CASES)
def test_oracle_binary_rule(oracle, table, case):
    """B(c1, c2): (d/dc1, d/dc2) = (dB/da, dB/db), as test_oracle_unary_rule."""
    import srhip as sr

    opts = sr.Options(binary_operators=(case.replace("^neg", "^"),), unary_operators=())
    i = BIN_CASES.index(case)
    s = table["bin_set"][i]
    for dt in ("f32", "f64"):
        a, b = table[f"bin_a_{dt}"][s].astype(np.float64), table[f"bin_b_{dt}"][s].astype(np.float64)
        got = np.array([_one_row_grad(oracle, sr, opts, sr.Node(1, sr.Node(val=u), sr.Node(val=v)))
                        for u, v in zip(a, b)])
        bar = 0 if case in EXACT_BIN else 128 * EPS["f64"]
        ea, eb = rel_err(got[:, 0], table[f"bin_fa_{dt}"][i]), rel_err(got[:, 1], table[f"bin_fb_{dt}"][i])
        assert ea.max() <= bar and eb.max() <= bar, (dt, ea.max() / EPS["f64"], eb.max() / EPS["f64"])


def test_oracle_gamma_has_no_rule(oracle):
    import srhip as sr

    opts = sr.Options(binary_operators=("*",), unary_operators=("gamma",))
    g = _one_row_grad(oracle, sr, opts, sr.Node(1, sr.Node(1, sr.Node(val=1.5), sr.Node(feature=1))))
    assert np.isnan(g[0])


# ---- conditioning: the device's formulas in working precision ---------------------------------------
def restate_unary(op, x):
    """The device's derivative formula (csrc/srhip_grad_impl.h) in NumPy, in x's precision: Float32
    transcendentals widen to Float64 and round once, everything else is working-precision arithmetic."""
    T = x.dtype.type
    one = T(1)

    def w(fn, v=x):
        return fn(v.astype(np.float64)).astype(T)

    if op == "cos": return -w(np.sin)
    if op == "sin": return w(np.cos)
    if op == "tan": f = w(np.tan); return one + f * f
    if op == "exp": return w(np.exp)
    if op == "log": return one / x
    if op == "log2": return one / (x * T(LN2))
    if op == "log10": return one / (x * T(LN10))
    if op == "log1p": return one / (one + x)
    if op == "sqrt": return T(0.5) / np.sqrt(x)
    if op == "acosh": return one / np.sqrt(x * x - one)
    if op == "atanh_clip": u = np.mod(x + one, T(2)) - one; return one / (one - u * u)
    if op == "sinh": return w(np.cosh)
    if op == "cosh": return w(np.sinh)
    if op == "tanh": f = w(np.tanh); return one - f * f
    if op == "asin": return one / np.sqrt(one - x * x)
    if op == "acos": return -one / np.sqrt(one - x * x)
    if op == "atan": return one / (one + x * x)
    if op == "asinh": return one / np.sqrt(x * x + one)
    if op == "erf": return T(TWO_SQRTPI) * w(np.exp, -x * x)
    if op == "erfc": return -T(TWO_SQRTPI) * w(np.exp, -x * x)
    if op == "exp2": return w(np.exp2) * T(LN2)
    if op == "expm1": return w(np.expm1) + one
    if op == "cbrt": f = w(np.cbrt); return one / (T(3) * f * f)
    if op == "square": return T(2) * x
    if op == "cube": return T(3) * x * x
    raise KeyError(op)


def restate_binary(case, a, b):
    T = a.dtype.type
    one = T(1)

    def powT(u, v):
        return np.power(u.astype(np.float64), v.astype(np.float64)).astype(T)

    if case == "*": return b, a
    if case == "/": ib = one / b; return ib, -(a / b) * ib
    if case == "^": return b * powT(a, b - one), powT(a, b) * np.log(a.astype(np.float64)).astype(T)
    if case == "^neg": return b * powT(a, b - one), np.zeros_like(a)
    if case == "atan2": r = one / (a * a + b * b); return b * r, -a * r
    raise KeyError(case)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("op", [o for o in UN_OPS if o not in EXACT_UN])
def test_unary_domain_is_well_conditioned(table, op, dt):
    """On the table's domain the device's own formula, evaluated in working precision with a correctly
    rounded libm to within an ulp or so, stays within 16 eps(T) of the exact derivative: a condition on
    the inputs (measured: tanh 10.0, erf and erfc 2.0, cbrt 1.8, expm1 1.5, the others at most 1.4), which
    leaves the device tests' 128 eps a factor of 8 for the vendor libm's own ulps."""
    i = UN_OPS.index(op)
    x = table[f"un_x_{dt}"][table["un_dom"][i]]
    got = restate_unary(op, x)
    assert got.dtype == NP[dt]
    err = rel_err(got, table[f"un_df_{dt}"][i]).max() / EPS[dt]
    print(f"{op} {dt}: {err:.2f} eps")
    assert err <= 16, err


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("case", [c for c in BIN_CASES if c not in EXACT_BIN])
def test_binary_domain_is_well_conditioned(table, case, dt):
    i = BIN_CASES.index(case)
    s = table["bin_set"][i]
    fa, fb = restate_binary(case, table[f"bin_a_{dt}"][s], table[f"bin_b_{dt}"][s])
    ea = rel_err(fa, table[f"bin_fa_{dt}"][i]).max() / EPS[dt]
    eb = rel_err(fb, table[f"bin_fb_{dt}"][i]).max() / EPS[dt]
    print(f"{case} {dt}: {ea:.2f} {eb:.2f} eps")
    assert fa.dtype == NP[dt] and ea <= 16 and eb <= 16, (ea, eb)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_shifts_and_scalings_of_the_inputs_are_exact(table, dt):
    """What the device tests do to the inputs is exact in the working precision: x / 2 * 2, and
    (x - 0.5) + 0.5, ((x - 0.5) + 0.25) + 0.25 for the binary operands."""
    T = NP[dt]
    for k in ("un_x", "bin_a", "bin_b", "loss_d", "loss_a"):
        x = table[f"{k}_{dt}"]
        assert x.dtype == T
        assert np.array_equal((x / T(2)) * T(2), x)
        assert np.array_equal((x - T(0.5)) + T(0.5), x)
        assert np.array_equal(((x - T(0.5)) + T(0.25)) + T(0.25), x)
        assert np.array_equal((x - T(0.5)).astype(np.float64), x.astype(np.float64) - 0.5)


# ---- the oracle's Float32 rules ---------------------------------------------------------------------
def _one_row_grad_f32(oracle, sr, opts, tree):
    """As _one_row_grad through the Float32 restatement (grad_node_f32, behind loss_grad_devorder)."""
    nodes, _ = sr.flatten([tree], opts, np.float32)
    return oracle.loss_grad_devorder(nodes, opts.binop_codes, opts.unaop_codes, np.ones((1, 1), np.float32),
                                     np.array([-1e6], np.float32), kind=1)[1]


@pytest.mark.parametrize("op", UN_OPS)
def test_oracle_float32_unary_rule(oracle, table, op):
    """The Float32 dual numbers of the oracle: U(c1 * x1) at x1 = 1 within 128 eps(Float32) of the table's
    Float32 columns (exactly where the derivative is 0 or +-1)."""
    import srhip as sr

    opts = sr.Options(binary_operators=("*",), unary_operators=(op,))
    i = UN_OPS.index(op)
    x = table["un_x_f32"][table["un_dom"][i]]
    got = np.array([_one_row_grad_f32(oracle, sr, opts, sr.Node(1, sr.Node(1, sr.Node(val=float(v)), sr.Node(feature=1))))[0]
                    for v in x])
    err = rel_err(got, table["un_df_f32"][i])
    assert err.max() <= (0 if op in EXACT_UN else 128 * EPS["f32"]), err.max() / EPS["f32"]


@pytest.mark.parametrize("case", BIN_CASES)
def test_oracle_float32_binary_rule(oracle, table, case):
    import srhip as sr

    opts = sr.Options(binary_operators=(case.replace("^neg", "^"),), unary_operators=())
    i = BIN_CASES.index(case)
    s = table["bin_set"][i]
    got = np.array([_one_row_grad_f32(oracle, sr, opts, sr.Node(1, sr.Node(val=float(u)), sr.Node(val=float(v))))
                    for u, v in zip(table["bin_a_f32"][s], table["bin_b_f32"][s])])
    bar = 0 if case in EXACT_BIN else 128 * EPS["f32"]
    ea, eb = rel_err(got[:, 0], table["bin_fa_f32"][i]), rel_err(got[:, 1], table["bin_fb_f32"][i])
    assert ea.max() <= bar and eb.max() <= bar, (ea.max() / EPS["f32"], eb.max() / EPS["f32"])


# ---- the device tests' trees compile (no device) ----------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_device_rule_programs_compile_on_the_host(dt):
    """Every tree of tests/test_gpu_derivative_rules.py is accepted by the compiler, for every operator: the
    per-operator programs, the all-operator population and the composition population (host-only programs,
    as tests/test_host_compile.py makes them).  The operand forms a tree is meant to reach follow from the
    compiler's rules (derivative_rules_common's docstring) but cannot be asserted here: a program exposes
    its node and constant counts and the evaluator program's stack need (where constant subtrees are
    folded), not its gradient program, which is compiled on first use (SRHIP_DUMP_CODE writes the
    evaluator's program only), and this change adds no ABI for it.  What the node tables do show is
    asserted: the population holds, for every unary operator whose rule is not inline, that operator
    applied to feature x1 in a tree with a constant -- the nodes a constant-gradient launch turns into
    derived columns (csrc/srhip_compile.cpp grad_derived_spec), 24 distinct ones, within the view's 32."""
    import srhip as sr

    T = NP[dt]
    for op in UN_OPS:
        X, _ = C.unary_inputs(op, dt)
        opts = sr.Options(binary_operators=("*",), unary_operators=(op,))
        nodes, offs = sr.flatten(C.unary_trees(sr, op, X[0]), opts, T)
        assert list(sr.Program(None, nodes, offs, opts, T).num_constants()) == [0, 1, 1, 1, 1], op
    for case in BIN_CASES:
        a, b, _, _ = C.binary_inputs(case, dt)
        forms = C.binary_trees(sr, case, a, b)
        assert {f[0].split("@")[0] for f in forms} == {"AF", "FA", "AC", "CA", "SA0", "AS0", "SA1", "SA2", "SA3", "FF",
                                                       "FC", "CF", "CC"}
        opts = C.binary_options(sr, case)
        for form, tree, nconst in [(f[0], f[2], len(f[5])) for f in forms] + [
                (f[0], f[1], len(f[3])) for f in C.uniform_trees(sr, case, a, b)]:
            nodes, offs = sr.flatten([tree], opts, T)
            assert sr.Program(None, nodes, offs, opts, T).num_constants()[0] == nconst, (case, form)
    opts, nodes, offs, _, _ = C.all_operator_population(sr, dt)
    prog = sr.Program(None, nodes, offs, opts, T)
    assert prog.ntrees == 33 * 4 + 14 * 16 and (prog.num_constants() > 0).all()
    derived = set()
    for t in range(prog.ntrees):
        tn = nodes[offs[t]:offs[t + 1]]
        for n in tn:
            if n["degree"] == 1 and tn[n["l"]]["degree"] == 0 and not tn[n["l"]]["constant"]:
                derived.add((opts.unary_operators[n["op"] - 1], int(tn[n["l"]]["feature"])))
    names = {sr.operators.UNARY[o][0] for o in UN_OPS + ["gamma"] if o not in C.INLINE_UN}
    assert {d for d in derived if sr.operators.UNARY[d[0]][0] in names} == {(o, 1) for o in names} and len(names) == 24
    if dt == "f64":
        opts, nodes, offs, _, _ = C.composition_problem(sr)
        assert sr.Program(None, nodes, offs, opts, T).ntrees == 48


def test_composition_population_has_enough_to_compare(oracle):
    """The composition test's caps, decided here by the oracle alone: at least 30 of the 48 trees are ok
    with a constant, with at least 60 finite gradient components; no such tree has a non-finite one."""
    import srhip as sr

    ref = [r for r in C.composition_reference(sr, oracle) if r is not None]
    finite = sum(int(np.isfinite(r).sum()) for r in ref)
    assert len(ref) >= 30 and finite >= 60, (len(ref), finite)
    assert (len(ref), finite, sum(r.size for r in ref)) == (34, 63, 63)
