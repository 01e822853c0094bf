"""The did_succeed decision on the host (csrc/srhip_decide.cpp), without a device: host-only programs through
srhip_partials_finalize, srhip_precise_finalize and the diagnostic srhip_decide_rowset.

The rule, restated exactly below (Fraction arithmetic) from DESIGN.md section 4 and the comments of
csrc/srhip_decide.h -- not from the code.  For T = Float32 / Float64 let OVF = 2^128 - 2^103 / 2^1024 - 2^970 (the
smallest exact sum that rounds to +Inf in T) and m the row count.  A tree fails (status 1) when it fails
statically, when a fill constant c has |c| m >= OVF (a NaN constant never does), or when a feature column it
checks has a non-finite entry, a non-finite sum or |sum| >= OVF (Float64 sums arrive scaled by 2^-64).  A tree
with operators then fails on a non-finite check statistic, and is undecided (status 2) when twice the bound on
any operator output's column sum reaches OVF: the bound is m * chk for Float32 (chk = max |v|) and chk * 2^512
for Float64 (chk = sum of |v| 2^-512).  Otherwise it succeeds (status 0).  Int32 trees fail only statically.

Every input below makes the code's 64-bit-mantissa product exact (a power-of-two row count, or an operand of
at most 11 significant bits), so the exact rule and the long double code agree by construction.
"""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import srhip as sr
import srhip._lib as L

OVF = {np.float32: Fraction(2) ** 128 - Fraction(2) ** 103, np.float64: Fraction(2) ** 1024 - Fraction(2) ** 970}
OPTS = sr.Options(binary_operators=("+", "*"), unary_operators=("cos",))
OPTS_I32 = sr.Options(binary_operators=("+", "*"), unary_operators=("neg",))
X = lambda f: sr.Node(feature=f)  # noqa: E731
C = lambda v: sr.Node(val=v)  # noqa: E731


def _program(trees, dtype):
    opts = OPTS_I32 if dtype == np.int32 else OPTS
    nodes, offs = sr.flatten(trees, opts, dtype)
    return sr.Program(None, nodes, offs, opts, dtype)


def _sums(nt, nf, m, num=1.0, den=None, fsum=None, fbad=None):
    s = np.zeros(2 * nt + 2 * nf + 1)
    s[0:2 * nt:2] = num
    s[1:2 * nt:2] = m if den is None else den
    s[2 * nt:2 * nt + 2 * nf:2] = 0.0 if fsum is None else fsum
    s[2 * nt + 1:2 * nt + 2 * nf:2] = 0.0 if fbad is None else fbad
    s[2 * nt + 2 * nf] = m
    return s


def _finalize(prog, nf, sums, chk, slow=False):
    old = os.environ.pop("SRHIP_DECIDE_SLOW", None)
    try:
        if slow:
            os.environ["SRHIP_DECIDE_SLOW"] = "1"
        return prog.finalize(nf, sums, chk)
    finally:
        os.environ.pop("SRHIP_DECIDE_SLOW", None)
        if old is not None:
            os.environ["SRHIP_DECIDE_SLOW"] = old


def _both(prog, nf, sums, chk):
    """finalize with the compact records and with SRHIP_DECIDE_SLOW=1: equal, NaN positions included."""
    fast, slow = _finalize(prog, nf, sums, chk), _finalize(prog, nf, sums, chk, slow=True)
    for a, b in zip(fast, slow):
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    assert np.array_equal(np.isnan(fast[0]), np.isnan(slow[0]))
    return fast


def exact_status(dtype, m, static_fail=False, consts=(), cols=(), chk=None):
    """The rule of the module docstring: cols = (sum, non-finite count) of each checked column, chk = the check
    statistic of a tree with operators (None: a tree without)."""
    if static_fail:
        return 1
    if dtype == np.int32:
        return 0
    ovf = OVF[dtype]
    for c in consts:
        if math.isinf(c) or (not math.isnan(c) and abs(Fraction(c)) * m >= ovf):
            return 1
    for s, bad in cols:
        if bad > 0 or not math.isfinite(s):
            return 1
        if abs(Fraction(s)) * (Fraction(2) ** 64 if dtype == np.float64 else 1) >= ovf:
            return 1
    if chk is None:
        return 0
    if not math.isfinite(chk):
        return 1
    bound = Fraction(chk) * (Fraction(2) ** 512 if dtype == np.float64 else m)
    return 2 if 2 * bound >= ovf else 0


def _around(thr, ftype=np.float64):
    """The values of ftype around the exact threshold thr: the largest below it, the smallest at or above it
    (thr itself where ftype holds it, +Inf where no finite value reaches it) and the next one up -- one ulp of
    the input apart."""
    zero, inf = ftype(0), ftype(np.inf)
    if thr > Fraction(float(np.finfo(ftype).max)):
        at = inf
    else:
        at = ftype(float(thr))
        while Fraction(float(at)) < thr:
            at = np.nextafter(at, inf)
        while Fraction(float(np.nextafter(at, zero))) >= thr:
            at = np.nextafter(at, zero)
    return [float(np.nextafter(at, zero)), float(at), float(np.nextafter(at, inf))]


# ---- fast equals slow -------------------------------------------------------------------------------------------
NF = 72


def _population(dtype):
    big = 3.0e38 if dtype == np.float32 else 1.0e308
    trees = [C(2.5), C(-big), C(float("nan")), C(float("inf")), X(1), X(3), X(70), sr.Node("cos", X(2)),
             sr.Node("cos", X(71)), sr.Node("*", X(1), X(2)), sr.Node("+", sr.Node("*", X(1), C(3.0)), sr.Node("*", C(big), C(0.5))),
             sr.Node("+", X(1), C(float("nan"))), sr.Node("cos", sr.Node("*", X(1), X(2))), sr.Node("+", sr.Node("cos", X(5)), X(64))]
    if dtype == np.int32:
        trees = [C(3), X(1), X(70), sr.Node("*", X(1), X(2)), sr.Node("+", X(1), C(2))]
    return trees + sr.random_population(40, OPTS_I32 if dtype == np.int32 else OPTS, 5, dtype, seed=11, max_size=20)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_fast_records_decide_as_the_tree_info(dtype):
    trees = _population(dtype)
    prog, nt = _program(trees, dtype), len(trees)
    rng = np.random.default_rng(3)
    ovf = float(OVF[np.float64 if dtype == np.float64 else np.float32]) if dtype != np.float64 else 1.7e308
    seen = set()
    for it in range(300):
        m = float(2 ** int(rng.integers(0, 24))) if it % 3 else float(rng.integers(1, 5000))
        edge = [0.0, 1.0, -1.0, ovf, -ovf, ovf / m, ovf / (2 * m), np.nextafter(ovf / (2 * m), 0), ovf / 2, np.inf, -np.inf, np.nan]
        if dtype == np.float64:
            edge += [2.0 ** 511, np.nextafter(2.0 ** 511, 0), 2.0 ** 960, 2.0 ** 959]
        pick = lambda n: np.where(rng.random(n) < 0.5, rng.choice(edge, n), rng.standard_normal(n) * 10.0 ** rng.integers(-3, 39, n))  # noqa: E731
        sums = _sums(nt, NF, m, num=pick(nt), fsum=pick(NF), fbad=np.where(rng.random(NF) < 0.1, 1.0, 0.0))
        chk = np.abs(pick(nt))
        loss, ok, st = _both(prog, NF, sums, chk)
        assert np.array_equal(ok, st == 0) and np.all(np.isinf(loss[st != 0]))
        seen.update(st.tolist())
    assert seen == ({0} if dtype == np.int32 else {0, 1, 2})  # (no Int32 tree here fails statically)


# ---- the rule itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rule_against_the_exact_restatement(dtype):
    ovf = OVF[dtype]
    scale_chk = Fraction(2) ** 512 if dtype == np.float64 else None
    scale_col = Fraction(2) ** 64 if dtype == np.float64 else Fraction(1)
    checked = 0
    for m in (1, 4096, 2 ** 20, 1536, 5):  # powers of two: thresholds a double holds; 1536, 5: at most 11 bits
        mf = Fraction(m)
        # a fill constant: |c| m >= OVF fails; NaN never; +/-Inf always
        # (a constant is a value of T: the points are one ulp of T apart)
        near = _around(ovf / mf, dtype)
        for c in near + [-v for v in near] + [1.0, float("nan"), float("inf"), float("-inf")]:
            prog = _program([C(c)], dtype)
            loss, ok, st = _both(prog, 1, _sums(1, 1, m, num=3.0), np.zeros(1))
            want = exact_status(dtype, mf, consts=[c])
            assert st[0] == want and ok[0] == (want == 0), (m, c)
            assert loss[0] == (3.0 / m if want == 0 else np.inf)
            checked += 1
        # a checked feature column (a root feature leaf; feature 70: the TreeInfo record)
        for feat in (2, 70):
            prog = _program([X(feat)], dtype)
            thr = ovf / scale_col
            for s in _around(thr) + [-v for v in _around(thr)] + [0.0, float("inf"), float("nan")]:
                for bad in (0.0, 1.0):
                    fsum, fbad = np.zeros(NF), np.zeros(NF)
                    fsum[feat - 1], fbad[feat - 1] = s, bad
                    loss, ok, st = _both(prog, NF, _sums(1, NF, m, fsum=fsum, fbad=fbad), np.zeros(1))
                    assert st[0] == exact_status(dtype, mf, cols=[(s, bad)]), (m, feat, s, bad)
                    checked += 1
        # the operator statistic and the factor 2 of the undecided band
        prog = _program([sr.Node("*", X(1), X(2))], dtype)
        half = ovf / (2 * (scale_chk if scale_chk else mf))
        for chk in _around(half) + _around(2 * half) + [0.0, 1.0, float("inf"), float("nan")]:
            loss, ok, st = _both(prog, 2, _sums(1, 2, m, num=6.0, den=4.0), np.array([chk]))
            want = exact_status(dtype, mf, chk=chk)
            assert st[0] == want, (m, chk)
            assert loss[0] == (1.5 if want == 0 else np.inf) and ok[0] == (want == 0)
            checked += 1
        assert exact_status(dtype, mf, chk=_around(half)[0]) == 0 and exact_status(dtype, mf, chk=_around(half)[1]) == 2
    # a tree without operators ignores the statistic; a static failure stands whatever the partials say
    prog = _program([X(1), sr.Node("+", X(1), C(float("nan")))], dtype)
    _, ok, st = _both(prog, 1, _sums(2, 1, 64.0), np.array([np.inf, 0.0]))
    assert st.tolist() == [0, 1] and ok.tolist() == [True, False]
    assert checked == 5 * 56


def test_int32_fails_only_statically():
    prog = _program([X(1), sr.Node("*", X(1), X(2)), C(7)], np.int32)
    loss, ok, st = _both(prog, 2, _sums(3, 2, 8.0, num=16.0, fsum=1e300, fbad=1.0), np.full(3, np.inf))
    assert st.tolist() == [0, 0, 0] and loss.tolist() == [2.0, 2.0, 2.0]


# ---- precise finalize ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_precise_finalize(dtype):
    # tree 0: cos(x1 * x2) -- the product is evaluated inside cos's loop (operator 0 unchecked, operator 1
    # checked); tree 1: (x1 * x2) * x3 -- both checked; tree 2 fails statically; tree 3 has one operator
    trees = [sr.Node("cos", sr.Node("*", X(1), X(2))), sr.Node("*", sr.Node("*", X(1), X(2)), X(3)),
             sr.Node("+", sr.Node("*", X(1), X(2)), C(float("inf"))), sr.Node("*", X(1), X(2))]
    prog = _program(trees, dtype)
    stride = prog.max_ops()
    assert stride == 2
    thr = OVF[dtype] / (Fraction(2) ** 64 if dtype == np.float64 else 1)
    below, at, above = _around(thr)

    def ok_of(tree, k, v):
        ops = np.ones((2, stride))  # (a second listed tree: the stride is the program's, not the tree's)
        ops[1, k] = v
        return bool(prog.precise_finalize([3, tree], ops)[1])

    for v in (np.inf, -np.inf, np.nan):
        assert not ok_of(0, 0, v) and not ok_of(0, 1, v) and not ok_of(1, 0, v)  # whatever op_sumcheck says
    for sgn in (1.0, -1.0):
        assert ok_of(0, 0, sgn * above) and ok_of(0, 0, sgn * at)  # unchecked: only non-finite fails
        for tree, k in ((0, 1), (1, 0), (1, 1)):
            assert ok_of(tree, k, sgn * below)
            assert ok_of(tree, k, sgn * at) == (Fraction(at) < thr) and not ok_of(tree, k, sgn * above)
    assert not ok_of(2, 0, 1.0)  # a static failure stays a failure
    assert ok_of(3, 0, below) and ok_of(3, 1, np.nan)  # (entries past a tree's operators are not read)


# ---- the row-set form ---------------------------------------------------------------------------------------------
def _decide_rowset(prog, tree, nf, rows, stats, chk_raw, slow=False):
    lib = L.load()
    st, chk = ctypes.c_uint8(), ctypes.c_double()
    stats = np.ascontiguousarray(stats, dtype=np.float64)
    old = os.environ.pop("SRHIP_DECIDE_SLOW", None)
    try:
        if slow:
            os.environ["SRHIP_DECIDE_SLOW"] = "1"
        L.check(lib.srhip_decide_rowset(prog.handle, tree, nf, rows, L.ptr(stats), float(chk_raw), ctypes.byref(st),
                                        ctypes.byref(chk)))
    finally:
        os.environ.pop("SRHIP_DECIDE_SLOW", None)
        if old is not None:
            os.environ["SRHIP_DECIDE_SLOW"] = old
    return st.value, chk.value


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_rowset_decision_equals_finalize(dtype):
    trees = _population(dtype)
    prog, nt = _program(trees, dtype), len(trees)
    rng = np.random.default_rng(5)
    for it in range(40):
        m = int(rng.integers(1, 3000))
        stats = np.zeros((NF, 3))
        stats[:, 0] = rng.standard_normal(NF) * 10.0 ** rng.integers(-2, 39, NF)
        stats[:, 1] = rng.random(NF) < 0.05
        stats[:, 2] = np.abs(rng.standard_normal(NF)) * 10.0 ** rng.integers(-2, 30 if it % 2 else 3, NF)
        raw = np.abs(rng.standard_normal(nt)) * 10.0 ** rng.integers(-2, 39, nt)
        raw[rng.random(nt) < 0.1] = np.inf
        if dtype == np.float32:
            raw = raw.astype(np.float32).astype(np.float64)
        got = [_decide_rowset(prog, t, NF, m, stats, raw[t], slow=bool(it % 2)) for t in range(nt)]
        applied = np.array([g[1] for g in got])
        if dtype == np.float64:
            assert np.array_equal(applied, raw)
        sums = _sums(nt, NF, float(m), fsum=stats[:, 0], fbad=stats[:, 1])
        if dtype == np.int32:  # Int32 data carries no statistics
            sums = _sums(nt, NF, float(m))
            assert not applied.any()
        _, _, st = _both(prog, NF, sums, applied)
        assert [g[0] for g in got] == st.tolist()


def test_rowset_feature_bound_and_skip_bound():
    """Float32: the statistic is raised to the tree's +/- bound cM M + cF F + c0 with F = the set's largest
    |x| rounded up to Float32 (+Inf when any entry is non-finite): a finite bound only moves a decided tree to
    undecided, never to failed, and a non-finite raw statistic stands."""
    # x1 + x2: no statistic folded on the device, so its bound is all that decides; x1 * x2 has no bound
    prog = _program([sr.Node("+", X(1), X(2)), sr.Node("*", X(1), X(2))], np.float32)
    m = 1024

    def chk_at(maxabs, bad=0.0, raw=0.0, tree=0):
        return _decide_rowset(prog, tree, 2, m, [[0.0, 0.0, 1.0], [0.0, bad, maxabs]], raw)

    # F enters the bound as a Float32 rounded up.  The tree's bound is cM = 0, cF = 2 (a feature is within F, a
    # sum within its operands' bounds), c0 = 0, so the statistic decided on is max(raw, 2 F): a maxabs that is a
    # Float32 comes back as itself, one between two floats as the float above
    f = float(np.float32(3.0e30))
    up = float(np.nextafter(np.float32(f), np.float32(np.inf)))
    assert f < (f + up) / 2 < up
    assert chk_at(f) == (0, 2 * f) and chk_at(up) == (0, 2 * up)
    assert chk_at((f + up) / 2) == (0, 2 * up) and chk_at(float(np.nextafter(f, np.inf))) == (0, 2 * up)
    raw = float(np.float32(3 * f))  # (the interpreter's statistic is a Float32)
    assert chk_at(f, raw=raw) == (0, raw)  # the raw statistic where it is the larger
    # a finite bound moves 0 -> 2 and never to 1: 2 m (2 F) >= OVF is undecided, and so is a bound clamped at
    # FLT_MAX
    flt_max = float(np.finfo(np.float32).max)
    big = float(np.float32(1.0e38))
    assert chk_at(big) == (2, 2 * big) and chk_at(3.0e38) == (2, flt_max)
    # a non-finite count > 0, or an infinite maxabs: F = +Inf, the bound clamps to FLT_MAX: undecided, not failed
    for st_c in (chk_at(1.0, bad=1.0), chk_at(float("inf"))):
        assert st_c == (2, flt_max)
    # a non-finite raw statistic stands (and fails); a tree without a bound keeps its raw statistic
    for raw in (float("inf"), float("nan")):
        st, c = chk_at(1.0, raw=raw)
        assert st == 1 and (c == raw or (math.isnan(c) and math.isnan(raw)))
    assert chk_at(1.0e38, raw=5.0, tree=1) == (0, 5.0)
    # errors: a tree out of range, a checked feature past nfeatures
    lib, st8 = L.load(), ctypes.c_uint8()
    one = np.zeros(3)
    assert lib.srhip_decide_rowset(prog.handle, 2, 2, 4, L.ptr(np.zeros(6)), 0.0, ctypes.byref(st8), None) == L.ERR_INVALID
    pf = _program([X(2)], np.float32)
    assert lib.srhip_decide_rowset(pf.handle, 0, 1, 4, L.ptr(one), 0.0, ctypes.byref(st8), None) == L.ERR_INVALID
