"""Generator of tests/golden/forward_values.npz: exact values of every operator of the forward interpreter
(csrc/srhip_eval_impl.h), by mpmath at 50 digits and exact rational arithmetic.

    python tests/golden/make_forward_values.py          # rewrites forward_values.npz

Needs mpmath (1.3.0 when the committed table was made); the tests only read the table, and
tests/test_forward_values_table.py regenerates it in memory (build_table) where mpmath can be imported.

The semantics are csrc/srhip_ops.h restated: domain checks, zero signs and special values written out here,
the functions themselves evaluated by mpmath at the exact stored input.  Every operator has a class:

  exact    + - * / neg abs square cube relu sign round floor ceil max min greater cond logical_or logical_and
           sqrt mod: exact arithmetic with one rounding to T per machine operation (cube: two; mod: an exact
           remainder, then at most one rounded r + y).  A device must match bit for bit, zero signs included.
  rounded  the Float32 operators that widen to Float64 and round once.  Every Float32 point whose exact
           value lies within 2^-36 (relative) of a Float32 rounding boundary is rejected here (general points
           are redrawn, special points masked out -- or asserted, if hand-picked for the operator), so any
           Float64 implementation accurate to 2^17 ulp rounds to the tabulated Float32: bit for bit again.
  ulp1     Float32 exp sin cos tan (the shared include/srhip_math.h): within 1 ulp of the tabulated value.
  In Float64 every operator that is not exact is held to a relative bound against the tabulated value, which
  is the exact value rounded once to Float64.

Layout (D = "f32" / "f64": inputs are drawn once per type and stored in it; P = 191 general points, odd, so
that a cyclic tiling walks every point through every row position of a lane and both halves of a row pair):

  un_ops [33], un_class [33], un_set [33]     names, classes, index of the operator's input set
  un_sets [7]                                 names of the input sets
  un_x_D [7, P], un_y_D [33, P]               general inputs, values
  un_sx_D [S], un_sy_D [33, S], un_sm_D       special inputs (one list for every operator), values, and
                                              the mask of points that count for the operator
  bin_ops [13], bin_class [13], bin_set [13], bin_sets [3]
  bin_a_D, bin_b_D [3, P], bin_y_D [13, P]
  bin_sa_D, bin_sb_D [SB], bin_sy_D [13, SB], bin_sm_D [13, SB]
"""
import math
import os
import sys
from fractions import Fraction

import numpy as np

P = 191
NP = {"f32": np.float32, "f64": np.float64}
FMT = {"f32": (24, -126, 127), "f64": (53, -1022, 1023)}  # precision, emin, emax
MARGIN_BITS = 36
NAN, INF = math.nan, math.inf

EXACT_UN = ["neg", "abs", "square", "cube", "relu", "sign", "round", "floor", "ceil", "sqrt"]
EXACT_BIN = ["+", "-", "*", "/", "max", "min", "greater", "cond", "logical_or", "logical_and", "mod"]
ULP1 = ["exp", "sin", "cos", "tan"]

UN_SETS = ["pm", "pos", "log1p", "acosh", "unit", "gamma", "wrap"]
UN_OPS = [  # (name, input set) in the order of csrc/srhip_isa.h
    ("neg", "pm"), ("square", "pm"), ("cube", "pm"), ("abs", "pm"), ("relu", "pm"), ("cos", "pm"), ("sin", "pm"),
    ("tan", "pm"), ("exp", "pm"), ("log", "pos"), ("log2", "pos"), ("log10", "pos"), ("log1p", "log1p"),
    ("sqrt", "pos"), ("acosh", "acosh"), ("atanh_clip", "wrap"), ("sinh", "pm"), ("cosh", "pm"), ("tanh", "pm"),
    ("asin", "unit"), ("acos", "unit"), ("atan", "pm"), ("asinh", "pm"), ("erf", "pm"), ("erfc", "pm"),
    ("gamma", "gamma"), ("round", "pm"), ("floor", "pm"), ("ceil", "pm"), ("sign", "pm"), ("exp2", "pm"),
    ("expm1", "pm"), ("cbrt", "pm"),
]
BIN_SETS = ["gen", "pow", "mod"]
BIN_OPS = [
    ("+", "gen"), ("-", "gen"), ("*", "gen"), ("/", "gen"), ("^", "pow"), ("greater", "gen"), ("cond", "gen"),
    ("logical_or", "gen"), ("logical_and", "gen"), ("max", "gen"), ("min", "gen"), ("mod", "mod"), ("atan2", "gen"),
]


def op_class(name):
    if name in EXACT_UN or name in EXACT_BIN:
        return "exact"
    return "ulp1" if name in ULP1 else "rounded"


# ---- rounding an exact value to T ------------------------------------------------------------------------
def _scaled(fr, dt):
    """(|fr| in units of T's ulp at |fr|, that ulp's exponent)."""
    p, emin, _ = FMT[dt]
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = max(e, emin) - (p - 1)
    return a / Fraction(2) ** q, q


def round_to(fr, dt):
    """The T value nearest to the non-zero Fraction fr (ties to even), as a Python float: +-inf past the
    largest finite value, a signed zero below half the smallest subnormal."""
    p, _, emax = FMT[dt]
    n, q = _scaled(fr, dt)
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl & 1):
        fl += 1
    s = -1.0 if fr < 0 else 1.0
    if fl and fl.bit_length() + q > emax + 1:
        return s * INF
    return s * math.ldexp(fl, q)


def near_boundary(fr, dt):
    """Is fr within 2^-MARGIN_BITS (relative) of a rounding boundary of T (a midpoint of two neighbours,
    the overflow threshold among them)."""
    if abs(fr) >= Fraction(2) ** (FMT[dt][2] + 1):
        return False  # Inf whatever the last bits: the overflow threshold is 2^-(p + 1) below, relatively
    n, _ = _scaled(fr, dt)
    rem = n - n.numerator // n.denominator
    return abs(rem - Fraction(1, 2)) < n / Fraction(2) ** MARGIN_BITS


def _sb(x):
    return math.copysign(1.0, x) < 0


def _zero_like(x):
    return math.copysign(0.0, x)


# ---- the exact class: IEEE arithmetic from rational arithmetic ---------------------------------------------
def f_add(a, b, dt):
    if math.isnan(a) or math.isnan(b):
        return NAN
    if math.isinf(a) or math.isinf(b):
        if math.isinf(a) and math.isinf(b) and a != b:
            return NAN
        return a if math.isinf(a) else b
    s = Fraction(a) + Fraction(b)
    if s == 0:
        return -0.0 if (_sb(a) and _sb(b)) else 0.0
    return round_to(s, dt)


def f_mul(a, b, dt):
    if math.isnan(a) or math.isnan(b):
        return NAN
    neg = _sb(a) != _sb(b)
    if math.isinf(a) or math.isinf(b):
        return NAN if (a == 0 or b == 0) else (-INF if neg else INF)
    s = Fraction(a) * Fraction(b)
    if s == 0:
        return -0.0 if neg else 0.0
    return round_to(s, dt)


def f_div(a, b, dt):
    if math.isnan(a) or math.isnan(b):
        return NAN
    neg = _sb(a) != _sb(b)
    if math.isinf(a):
        return NAN if math.isinf(b) else (-INF if neg else INF)
    if math.isinf(b):
        return -0.0 if neg else 0.0
    if b == 0:
        return NAN if a == 0 else (-INF if neg else INF)
    if a == 0:
        return -0.0 if neg else 0.0
    return round_to(Fraction(a) / Fraction(b), dt)


def f_max(a, b):
    if math.isnan(a) or math.isnan(b):
        return NAN
    if a == b:
        return b if _sb(a) else a  # -0.0 < +0.0
    return a if a > b else b


def f_min(a, b):
    if math.isnan(a) or math.isnan(b):
        return NAN
    if a == b:
        return a if _sb(a) else b
    return a if a < b else b


def f_fmod(x, y):
    """C fmod: exact in every floating-point type."""
    if math.isnan(x) or math.isnan(y) or math.isinf(x) or y == 0:
        return NAN
    if math.isinf(y) or x == 0:
        return x
    fx, fy = Fraction(x), Fraction(y)
    q = abs(fx) // abs(fy)
    r = abs(fx) - q * abs(fy)
    v = float(r)
    assert Fraction(v) == r
    return -v if _sb(x) else v


def f_mod(x, y, dt):
    r = f_fmod(x, y)
    if r == 0:
        return math.copysign(r, y)
    if (r > 0) != (y > 0):
        return f_add(r, y, dt)
    return r


def _int_round(x, how):
    if math.isnan(x) or math.isinf(x) or x == 0:
        return x
    fx = Fraction(x)
    v = {"round": round, "floor": math.floor, "ceil": math.ceil}[how](fx)  # round(Fraction): ties to even
    return math.copysign(float(v), x) if v == 0 else float(v)


def f_sqrt(x, dt, mp):
    if math.isnan(x) or x < 0:
        return NAN
    if x == 0 or math.isinf(x):
        return x
    return round_to(_frac(mp.sqrt(mp.mpf(x))), dt)  # (never a tie: mpmath's 50 digits decide the rounding)


def exact_un(name, x, dt, mp):
    if name == "neg":
        return -x
    if name == "abs":
        return abs(x)
    if name == "square":
        return f_mul(x, x, dt)
    if name == "cube":
        return f_mul(f_mul(x, x, dt), x, dt)
    if name == "relu":
        return x if x > 0 else _zero_like(x)
    if name == "sign":
        return -1.0 if x < 0 else (1.0 if x > 0 else x)
    if name in ("round", "floor", "ceil"):
        return _int_round(x, name)
    if name == "sqrt":
        return f_sqrt(x, dt, mp)
    raise KeyError(name)


def exact_bin(name, a, b, dt):
    if name == "+":
        return f_add(a, b, dt)
    if name == "-":
        return f_add(a, -b, dt)
    if name == "*":
        return f_mul(a, b, dt)
    if name == "/":
        return f_div(a, b, dt)
    if name == "max":
        return f_max(a, b)
    if name == "min":
        return f_min(a, b)
    if name == "greater":
        return 1.0 if a > b else 0.0
    if name == "cond":
        return b if a > 0 else _zero_like(b)
    if name == "logical_or":
        return 1.0 if (a > 0) or (b > 0) else 0.0
    if name == "logical_and":
        return 1.0 if (a > 0) and (b > 0) else 0.0
    if name == "mod":
        return f_mod(a, b, dt)
    raise KeyError(name)


# ---- the transcendental operators: (special values, mpmath) ------------------------------------------------
def _frac(v):
    """An mpf as an exact Fraction; a magnitude outside 2^+-5000, far past every overflow and underflow
    threshold, is clamped to that (exp(1e38) must not become a 1e38-bit integer)."""
    sign, man, exp, bc = v._mpf_
    if int(exp) + int(bc) > 5000 or int(exp) + int(bc) < -5000:
        f = Fraction(2) ** (5000 if int(exp) > 0 else -5000)
        return -f if sign else f
    f = Fraction(int(man)) * Fraction(2) ** int(exp)
    return -f if sign else f


ODD_AT_ZERO = {"sin", "tan", "log1p", "sinh", "tanh", "asin", "atan", "asinh", "erf", "expm1", "cbrt", "atanh"}
# the value at +inf and at -inf ("pi/2": that multiple of pi, rounded like any other value)
AT_INF = {
    "cos": (NAN, NAN), "sin": (NAN, NAN), "tan": (NAN, NAN), "exp": (INF, 0.0), "log": (INF, NAN), "log2": (INF, NAN),
    "log10": (INF, NAN), "log1p": (INF, NAN), "acosh": (INF, NAN), "atanh": (NAN, NAN), "sinh": (INF, -INF),
    "cosh": (INF, INF), "tanh": (1.0, -1.0), "asin": (NAN, NAN), "acos": (NAN, NAN), "atan": ("pi/2", "-pi/2"),
    "asinh": (INF, -INF), "erf": (1.0, -1.0), "erfc": (0.0, 2.0), "gamma": (NAN, NAN), "exp2": (INF, 0.0),
    "expm1": (INF, -1.0), "cbrt": (INF, -INF),
}


def _mp_un(mp):
    return {
        "cos": mp.cos, "sin": mp.sin, "tan": mp.tan, "exp": mp.exp, "log": mp.log,
        "log2": lambda x: mp.log(x) / mp.log(2), "log10": lambda x: mp.log(x) / mp.log(10), "log1p": mp.log1p,
        "acosh": mp.acosh, "atanh": mp.atanh, "sinh": mp.sinh, "cosh": mp.cosh, "tanh": mp.tanh, "asin": mp.asin,
        "acos": mp.acos, "atan": mp.atan, "asinh": mp.asinh, "erf": mp.erf, "erfc": mp.erfc, "gamma": mp.gamma,
        "exp2": lambda x: mp.power(2, x), "expm1": mp.expm1,
        "cbrt": lambda x: mp.cbrt(x) if x >= 0 else -mp.cbrt(-x),
    }


def un_exact_value(name, x, dt, mp):
    """The operator's value at the T value x (a Python float): a Python float for the values that need no
    rounding (NaN, infinities, zeros, the input itself), otherwise the exact value as a Fraction.
    atanh_clip's argument mod(x + 1, 2) - 1 is formed in T first, as the device forms it."""
    if name == "atanh_clip":
        x = f_add(f_mod(f_add(x, 1.0, dt), 2.0, dt), -1.0, dt)
        name = "atanh"
    if math.isnan(x):
        return NAN
    if math.isinf(x):
        v = AT_INF[name][0 if x > 0 else 1]
        if isinstance(v, str):
            return _frac(mp.pi / 2) * (-1 if v.startswith("-") else 1)
        return v
    # domains (csrc/srhip_ops.h: the safe_* operators return NaN; asin / acos outside [-1, 1] are NaN too)
    if name in ("log", "log2", "log10") and x <= 0:
        return NAN
    if name == "log1p" and x <= -1:
        return NAN
    if name == "acosh" and x < 1:
        return NAN
    if name in ("asin", "acos") and abs(x) > 1:
        return NAN
    if name == "atanh" and abs(x) >= 1:
        return NAN if abs(x) > 1 else math.copysign(INF, x)
    if name == "gamma" and x <= 0 and x == math.floor(x):
        return NAN  # a pole: tgamma gives +-Inf at +-0 and NaN at the negative integers; Inf becomes NaN
    if x == 0 and name in ODD_AT_ZERO:
        return x
    if name in ("erf", "erfc") and abs(x) > 200:
        # erfc(200) < 2^-57000, below every underflow threshold (mpmath's erfc refuses arguments near 1e308)
        eps = Fraction(2) ** -5000
        if name == "erf":
            return (1 - eps) * (1 if x > 0 else -1)
        return eps if x > 0 else 2 - eps
    v = _mp_un(mp)[name](mp.mpf(x))
    if v == 0:
        return 0.0  # log(1), acosh(1), acos(1): +0
    return _frac(v)


def _finish(name, v, dt):
    """Round an exact value; gamma's overflow is NaN (csrc/srhip_ops.h: isinf(out) ? NaN : out)."""
    if isinstance(v, Fraction):
        v = round_to(v, dt)
    if name == "gamma" and math.isinf(v):
        return NAN
    return v


def pow_exact_value(x, y, mp):
    """safe_pow's checks, then C pow with its special cases; Fraction or float as un_exact_value."""
    yfin = not (math.isnan(y) or math.isinf(y))
    yint = yfin and y == math.trunc(y)
    if yint:
        if y < 0 and x == 0:
            return NAN
    else:
        if y > 0 and x < 0:
            return NAN
        if y < 0 and x <= 0:
            return NAN
    if y == 0 or x == 1:
        return 1.0
    if math.isnan(x) or math.isnan(y):
        return NAN
    yodd = yint and abs(y) < 2.0 ** 53 and int(abs(y)) % 2 == 1
    if x == 0:
        if y < 0:
            return math.copysign(INF, x) if yodd else INF
        return x if yodd else 0.0
    if math.isinf(y):
        if abs(x) == 1:
            return 1.0
        return INF if (abs(x) < 1) == (y < 0) else 0.0
    if math.isinf(x):
        if x > 0:
            return INF if y > 0 else 0.0
        if y > 0:
            return -INF if yodd else INF
        return -0.0 if yodd else 0.0
    if x < 0 and not yint:
        return NAN
    v = _frac(mp.power(mp.mpf(abs(x)), mp.mpf(y)))
    return -v if (x < 0 and yodd) else v


def atan2_exact_value(a, b, mp):
    if math.isnan(a) or math.isnan(b):
        return NAN
    pi = _frac(+mp.pi)
    s = -1 if _sb(a) else 1
    if a == 0:
        return a if not _sb(b) else s * pi
    if math.isinf(a) and math.isinf(b):
        return s * pi * (Fraction(1, 4) if b > 0 else Fraction(3, 4))
    if math.isinf(a) or b == 0:
        return s * pi / 2
    if math.isinf(b):
        return _zero_like(a) if b > 0 else s * pi
    return _frac(mp.atan2(mp.mpf(a), mp.mpf(b)))


def un_value(name, x, dt, mp):
    """(tabulated value, within the margin of a rounding boundary?)"""
    if op_class(name) == "exact":
        return exact_un(name, x, dt, mp), False
    v = un_exact_value(name, x, dt, mp)
    return _finish(name, v, dt), isinstance(v, Fraction) and near_boundary(v, dt)


def bin_value(name, a, b, dt, mp):
    if op_class(name) == "exact":
        return exact_bin(name, a, b, dt), False
    v = pow_exact_value(a, b, mp) if name == "^" else atan2_exact_value(a, b, mp)
    return _finish(name, v, dt), isinstance(v, Fraction) and near_boundary(v, dt)


def _margin_matters(name, dt):
    return dt == "f32" and op_class(name) == "rounded"


# ---- inputs ----------------------------------------------------------------------------------------------
# per input set: the interval of half of the draws, the binary exponents of the other half (log-uniform
# magnitudes), and whether those take both signs
_UN_DRAW = {
    "pm": ((-4.0, 4.0), (-30, 6), True), "pos": ((0.01, 8.0), (-30, 30), False),
    "log1p": ((-0.99, 4.0), (-30, 10), False), "acosh": ((1.0, 8.0), (0, 30), False),
    "unit": ((-1.0, 1.0), (-30, 0), True), "gamma": ((-6.0, 20.0), (-20, 5), True),
    "wrap": ((-6.0, 6.0), (-30, 2), True),
}


def _draw_one(rng, spec, dt):
    (lo, hi), (e0, e1), both = spec
    if rng.random() < 0.5:
        v = rng.uniform(lo, hi)
    else:
        v = 2.0 ** rng.uniform(e0, e1) * (1.0 if (not both or rng.random() < 0.5) else -1.0)
    return float(NP[dt](v))


def _specials(dt, mp):
    """The special unary inputs (one list for every operator) and, per operator, the hand-picked ones whose
    margin is asserted instead of masked."""
    T = NP[dt]
    fi = np.finfo(T)
    sub, tiny, big = float(fi.smallest_subnormal), float(fi.tiny), float(fi.max)
    nxt = lambda v, to: float(np.nextafter(T(v), T(to)))  # noqa: E731
    common = [0.0, -0.0, INF, -INF, NAN, sub, tiny, tiny / 4, big, -sub, -tiny, -big]
    picked = {o: list(common) for o, _ in UN_OPS}
    picked["log1p"] += [-1.0]
    picked["sqrt"] += [-tiny]
    picked["acosh"] += [1.0, nxt(1, 0)]
    picked["atanh_clip"] += [1.0, -1.0, 3.0, -3.0, 5.0, nxt(2, 0), nxt(2, 3), nxt(-2, 0), nxt(-2, -3), nxt(4, 0), nxt(4, 5)]
    for o in ("asin", "acos"):
        picked[o] += [1.0, -1.0, nxt(1, 2)]
    picked["tanh"] += [20.0, -20.0]
    picked["cbrt"] += [-8.0, 27.0]
    picked["round"] += [0.5, -0.5, 1.5, -1.5, 2.5, -2.5]
    emax, emin, p = FMT[dt][2], FMT[dt][1], FMT[dt][0]
    picked["exp2"] += [float(emax), float(emax + 1), float(emin), float(emin - p + 1), float(emin - p - 1)]
    # (2^(emin - p) itself is an exact tie between 0 and the smallest subnormal: not a fair point)

    def first(pred, lo, hi):
        """The smallest T value in [lo, hi] at which pred holds (pred false at lo, true at hi, monotonic)."""
        lo, hi = T(lo), T(hi)
        while np.nextafter(lo, hi) < hi:
            mid = T((float(lo) + float(hi)) / 2)
            if mid <= lo or mid >= hi:
                mid = np.nextafter(lo, hi)
            if pred(float(mid)):
                hi = mid
            else:
                lo = mid
        return float(hi)

    def val(name, x):
        return un_value(name, x, dt, mp)[0]

    def below(name, x):
        """The point under an overflow edge x: the nearest T value whose exact result is at least 2^-40
        (relative) under the largest finite value.  Float64 results are held to a relative bar of 1e-13
        (2^-43), so an implementation that meets it may still overflow nearer the edge than that."""
        for _ in range(64):
            x = nxt(x, 0)
            v = un_exact_value(name, x, dt, mp)
            if isinstance(v, Fraction) and abs(v) <= Fraction(big) * (1 - Fraction(1, 2 ** 40)):
                return x
        raise AssertionError(("no clear point under the edge", name, x))

    for name in ("exp", "expm1", "sinh", "cosh"):
        x = first(lambda v, n=name: math.isinf(val(n, v)), 1.0, 1000.0)
        picked[name] += [x, below(name, x)] + ([-x, -below(name, x)] if name in ("sinh", "cosh") else [])
    picked["expm1"] += [-40.0]
    x = first(lambda v: math.isnan(val("gamma", v)), 2.0, 200.0)  # tgamma overflows: Inf, which gamma makes NaN
    picked["gamma"] += [x, below("gamma", x), -1.0, -2.0, -3.0, -0.5]
    x = first(lambda v: val("erfc", v) < tiny, 1.0, 40.0)
    picked["erfc"] += [x, nxt(x, 0)]
    x = first(lambda v: val("erfc", v) == 0, 1.0, 40.0)
    picked["erfc"] += [x, nxt(x, 0)]
    x = first(lambda v: val("exp", -v) == 0, 1.0, 1000.0)
    picked["exp"] += [-x, -nxt(x, 0)]
    xs = []
    for o, _ in UN_OPS:
        for v in picked[o]:
            if not any(_same(v, w) for w in xs):
                xs.append(v)
    return xs, picked


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or (a == b and _sb(a) == _sb(b))


def _bin_specials(dt):
    T = NP[dt]
    fi = np.finfo(T)
    sub, tiny, big = float(fi.smallest_subnormal), float(fi.tiny), float(fi.max)
    third = float(T(1) / T(3))
    common = [0.0, -0.0, INF, -INF, NAN, sub, tiny, tiny / 4, big]
    every = [(c, d) for c in common for d in (1.5, -2.0)] + [(d, c) for c in common for d in (1.5, -2.0)]
    picked = {o: list(every) for o, _ in BIN_OPS}
    zeros = [(0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0)]
    nans = [(NAN, 1.0), (1.0, NAN), (NAN, NAN), (NAN, -1.0), (-1.0, NAN), (NAN, 0.0), (0.0, NAN)]
    for o in ("max", "min", "greater", "logical_or", "logical_and", "cond", "+", "-", "*", "/"):
        picked[o] += zeros + nans
    picked["cond"] += [(0.0, 5.0), (-0.0, 5.0), (0.0, -5.0), (1.0, -0.0), (-1.0, -0.0), (-1.0, 0.0), (sub, -3.0), (-sub, 3.0)]
    picked["mod"] += [(5.5, 3.0), (-5.5, 3.0), (5.5, -3.0), (-5.5, -3.0), (6.0, 3.0), (-6.0, 3.0), (6.0, -3.0), (-6.0, -3.0),
                      (1.0, 0.0), (1.0, -0.0), (1.0, INF), (-1.0, INF), (1.0, -INF), (-1.0, -INF), (0.0, INF), (-0.0, -INF),
                      (0.0, -INF), (-0.0, INF), (1.0, -3.0), (-1.0, 3.0), (-sub, big), (sub, -big), (-tiny, 1.0), (tiny, -1.0),
                      (INF, 2.0), (big, 3.0), (-big, 3.0), (NAN, 1.0), (1.0, NAN)]
    emax = FMT[dt][2]
    picked["^"] += [(0.0, -1.0), (-8.0, third), (-2.0, 3.0), (-2.0, 2.0), (0.0, 0.0), (INF, 0.0), (NAN, 0.0), (-2.0, INF),
                    (-0.5, INF), (-2.0, -INF), (2.0, 1024.0), (2.0, float(emax + 1)), (2.0, float(emax)), (1.0, NAN),
                    (-0.0, -3.0), (-0.0, 3.0), (-0.0, 2.0), (0.0, 3.0), (-INF, 3.0), (-INF, -3.0), (-INF, 2.0), (0.5, INF),
                    (0.5, -INF), (2.0, -INF), (-1.0, INF), (-0.0, -1.0), (-8.0, -third), (0.0, -0.5), (NAN, 1.0), (2.0, NAN),
                    (-2.0, -3.0), (-2.0, 0.5), (2.0, 0.5), (10.0, -2.0)]
    picked["atan2"] += [(a, b) for a in (0.0, -0.0) for b in (0.0, -0.0)] + [(a, b) for a in (INF, -INF) for b in (INF, -INF)]
    picked["atan2"] += [(a, b) for a in (0.0, -0.0) for b in (INF, -INF, 1.0, -1.0)]
    picked["atan2"] += [(a, b) for a in (INF, -INF, 1.0, -1.0) for b in (0.0, -0.0)]
    picked["atan2"] += [(NAN, 1.0), (1.0, NAN), (sub, big), (-sub, -big), (big, sub)]
    pairs = []
    for o, _ in BIN_OPS:
        for v in picked[o]:
            if not any(_same(v[0], w[0]) and _same(v[1], w[1]) for w in pairs):
                pairs.append(v)
    return pairs, picked


def build_table():
    """The whole table as {key: array} (needs mpmath)."""
    import mpmath as mp

    mp.mp.dps = 50
    z = {
        "un_ops": np.array([o for o, _ in UN_OPS]), "un_class": np.array([op_class(o) for o, _ in UN_OPS]),
        "un_set": np.array([UN_SETS.index(s) for _, s in UN_OPS], dtype=np.int32), "un_sets": np.array(UN_SETS),
        "bin_ops": np.array([o for o, _ in BIN_OPS]), "bin_class": np.array([op_class(o) for o, _ in BIN_OPS]),
        "bin_set": np.array([BIN_SETS.index(s) for _, s in BIN_OPS], dtype=np.int32), "bin_sets": np.array(BIN_SETS),
    }
    for dt in ("f32", "f64"):
        T = NP[dt]
        rng = np.random.default_rng([20250917, 32 if dt == "f32" else 64])
        # unary, general: a point is redrawn until no operator of its set lies near a rounding boundary
        ux = np.zeros((len(UN_SETS), P), T)
        uy = np.zeros((len(UN_OPS), P), T)
        for si, s in enumerate(UN_SETS):
            ops = [(i, o) for i, (o, ss) in enumerate(UN_OPS) if ss == s]
            for j in range(P):
                while True:
                    x = _draw_one(rng, _UN_DRAW[s], dt)
                    vals = [un_value(o, x, dt, mp) for _, o in ops]
                    if not any(near and _margin_matters(o, dt) for (_, o), (_, near) in zip(ops, vals)):
                        break
                ux[si, j] = x
                for (i, _), (v, _) in zip(ops, vals):
                    uy[i, j] = v
        z[f"un_x_{dt}"], z[f"un_y_{dt}"] = ux, uy
        # unary, special
        xs, picked = _specials(dt, mp)
        sy = np.zeros((len(UN_OPS), len(xs)), T)
        sm = np.ones((len(UN_OPS), len(xs)), bool)
        for i, (o, _) in enumerate(UN_OPS):
            for j, x in enumerate(xs):
                v, near = un_value(o, x, dt, mp)
                sy[i, j] = v
                if near and _margin_matters(o, dt):
                    assert not any(_same(x, w) for w in picked[o]), ("hand-picked point near a rounding boundary", o, x)
                    sm[i, j] = False
        z[f"un_sx_{dt}"], z[f"un_sy_{dt}"], z[f"un_sm_{dt}"] = np.array(xs, T), sy, sm
        # binary, general
        ba = np.zeros((len(BIN_SETS), P), T)
        bb = np.zeros((len(BIN_SETS), P), T)
        by = np.zeros((len(BIN_OPS), P), T)
        for si, s in enumerate(BIN_SETS):
            ops = [(i, o) for i, (o, ss) in enumerate(BIN_OPS) if ss == s]
            for j in range(P):
                while True:
                    if s == "pow":
                        if j % 8 == 7:  # a negative base with a small integer exponent
                            a = -abs(_draw_one(rng, ((0.1, 8.0), (-8, 8), False), dt))
                            b = float(rng.integers(-5, 6))
                        else:
                            a = _draw_one(rng, ((0.01, 8.0), (-8, 8), False), dt)
                            b = _draw_one(rng, ((-8.0, 8.0), (-10, 3), True), dt)
                    else:
                        a = _draw_one(rng, _UN_DRAW["pm"], dt)
                        b = _draw_one(rng, _UN_DRAW["pm"], dt)
                        if s == "mod" and j % 4 == 3 and abs(a) > abs(b):
                            a, b = b, a  # |x| < |y|
                    vals = [bin_value(o, a, b, dt, mp) for _, o in ops]
                    if b != 0 and not any(near and _margin_matters(o, dt) for (_, o), (_, near) in zip(ops, vals)):
                        break
                ba[si, j], bb[si, j] = a, b
                for (i, _), (v, _) in zip(ops, vals):
                    by[i, j] = v
        z[f"bin_a_{dt}"], z[f"bin_b_{dt}"], z[f"bin_y_{dt}"] = ba, bb, by
        # binary, special
        pairs, bpicked = _bin_specials(dt)
        sy = np.zeros((len(BIN_OPS), len(pairs)), T)
        sm = np.ones((len(BIN_OPS), len(pairs)), bool)
        for i, (o, _) in enumerate(BIN_OPS):
            for j, (a, b) in enumerate(pairs):
                v, near = bin_value(o, a, b, dt, mp)
                sy[i, j] = v
                if near and _margin_matters(o, dt):
                    assert not any(_same(a, w[0]) and _same(b, w[1]) for w in bpicked[o]), ("hand-picked pair", o, a, b)
                    sm[i, j] = False
        z[f"bin_sa_{dt}"] = np.array([p[0] for p in pairs], T)
        z[f"bin_sb_{dt}"] = np.array([p[1] for p in pairs], T)
        z[f"bin_sy_{dt}"], z[f"bin_sm_{dt}"] = sy, sm
    return z


TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "forward_values.npz")


def _planes(a):
    """A float array as its byte planes, uint8 [itemsize, *shape] (little-endian): the sign / exponent
    bytes of neighbouring values then lie together and deflate well."""
    a = np.ascontiguousarray(a, dtype=a.dtype.newbyteorder("<"))
    return np.ascontiguousarray(a.reshape(-1).view(np.uint8).reshape(-1, a.itemsize).T).reshape((a.itemsize,) + a.shape)


def _unplanes(p):
    dt = {4: "<f4", 8: "<f8"}[p.shape[0]]
    return np.ascontiguousarray(p.reshape(p.shape[0], -1).T).view(dt).reshape(p.shape[1:]).astype(dt[1:])


def load_table(path=TABLE):
    """The committed table as {key: array}: float arrays are stored as byte planes (_planes)."""
    z = np.load(path, allow_pickle=False)
    return {k: (_unplanes(z[k]) if z[k].dtype == np.uint8 else z[k]) for k in z.files}


def same_bits(a, b):
    """Equal arrays, bit for bit (zero signs; every NaN counts as one value)."""
    if a.dtype.kind != "f":
        return a.dtype == b.dtype and np.array_equal(a, b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and bool(
        np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def main():
    out = TABLE
    z = build_table()
    np.savez_compressed(out, **{k: (_planes(v) if v.dtype.kind == "f" else v) for k, v in z.items()})
    back = load_table(out)
    assert set(back) == set(z) and all(same_bits(back[k], z[k]) for k in z)
    size = os.path.getsize(out)
    print(f"{out}: {size} bytes")
    assert size < 256 * 1024, "the table must stay under 256 KB"
    return 0


if __name__ == "__main__":
    sys.exit(main())
