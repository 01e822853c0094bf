"""Generator of tests/golden/derivative_rules.npz: exact derivatives of every operator and loss that the
dual-number gradient kernel differentiates (csrc/srhip_grad_impl.h), by mpmath at 40 digits.

    python tests/golden/make_derivative_rules.py          # rewrites derivative_rules.npz

Needs mpmath (1.3.0 when the committed table was made); the tests only read the table, and
tests/test_oracle_grad_rules.py regenerates it in memory (build_table) where mpmath can be imported.

Layout (D = "f32" / "f64": the inputs are drawn once per dtype, stored in that dtype, and every
reference value is evaluated at the exact stored input and rounded once to Float64):

  un_ops [32]                 unary operator names (gamma has no derivative: not tabulated)
  un_dom [32]                 index of the operator's input set
  un_x_D [11, N]              the input sets (UN_DOMAINS below)
  un_df_D [32, N]             U'(x)
  bin_cases [14]              binary cases ("^neg": a negative base with an integer exponent)
  bin_set [14]                index of the case's input set
  bin_a_D, bin_b_D [5, N]     the input sets (BIN_SETS below)
  bin_fa_D, bin_fb_D [14, N]  dB/da, dB/db
  loss_kinds [20]             loss names, the nine distance losses first
  loss_d_D, loss_a_D [N]      residuals d = pred - y (distance losses), agreements a = y * pred (margin)
  loss_dl_D [20, N]           l'(d) or l'(a), the parameters being LOSS_P0 below

N = 300 points per case: a 256-row block and a 44-row tail.  Function values are not stored here: with
them the file would pass its 256 KB limit.  Operator values have a table of their own (forward_values.npz;
predictions are compared bit for bit with the evaluator), and so have the loss values l(d), l(a) at these
very residuals and agreements: loss_values.npz (make_loss_values.py, which imports the loss names, parameters
and kinks below and adds the points on and beside the kinks).  Float arrays are stored as byte planes (load_table
below reads them back): the same bits, about a sixth smaller once deflated.

Every input is a multiple of 2^-20 (Float32) / 2^-48 (Float64), so that the shifts and scalings the
tests apply (x - 0.5, x / 2, sums below 8) are exact in the working precision.  The distances from the
kinks are built into the draws and asserted here from the inputs alone: no test ever filters a row.
"""
import os
import sys

import numpy as np

N = 300
GRID = {"f32": 2.0 ** -20, "f64": 2.0 ** -48}
NP = {"f32": np.float32, "f64": np.float64}
MARGIN = 1.0 / 16

# (name, intervals of the domain, kinks to stay MARGIN away from)
_HALF = [k + 0.5 for k in range(-3, 3)]
UN_DOMAINS = [
    ("pm2", [(-2.0, 2.0)], []),
    ("tan", [(-1.2, 1.2)], []),
    ("log", [(0.25, 4.0)], []),
    ("cbrt", [(-4.0, -0.25), (0.25, 4.0)], []),
    ("log1p", [(-0.75, 3.0)], []),
    ("acosh", [(1.25, 4.0)], []),
    ("asin", [(-0.9, 0.9)], []),
    ("atanh", [(-0.9, 0.9), (1.1, 2.9)], []),
    ("sign", [(-2.0, 2.0)], [0.0]),
    ("floor", [(-2.0, 2.0)], [-2.0, -1.0, 0.0, 1.0, 2.0]),
    ("round", [(-2.0, 2.0)], _HALF),
]
_DOM = {d[0]: i for i, d in enumerate(UN_DOMAINS)}
UN_OPS = [  # (name, input set)
    ("cos", "pm2"), ("sin", "pm2"), ("exp", "pm2"), ("exp2", "pm2"), ("expm1", "pm2"), ("sinh", "pm2"),
    ("cosh", "pm2"), ("tanh", "pm2"), ("atan", "pm2"), ("asinh", "pm2"), ("erf", "pm2"), ("erfc", "pm2"),
    ("square", "pm2"), ("cube", "pm2"), ("neg", "pm2"), ("tan", "tan"), ("log", "log"), ("log2", "log"),
    ("log10", "log"), ("sqrt", "log"), ("cbrt", "cbrt"), ("log1p", "log1p"), ("acosh", "acosh"),
    ("asin", "asin"), ("acos", "asin"), ("atanh_clip", "atanh"), ("abs", "sign"), ("relu", "sign"),
    ("sign", "sign"), ("floor", "floor"), ("ceil", "floor"), ("round", "round"),
]
BIN_SETS = ["gen", "div", "pow", "powneg", "mod"]
BIN_CASES = [
    ("+", "gen"), ("-", "gen"), ("*", "gen"), ("/", "div"), ("^", "pow"), ("^neg", "powneg"), ("mod", "mod"),
    ("atan2", "gen"), ("max", "gen"), ("min", "gen"), ("greater", "gen"), ("cond", "gen"), ("logical_or", "gen"),
    ("logical_and", "gen"),
]
DIST = ["L2", "L1", "LP", "Huber", "L1EpsilonIns", "L2EpsilonIns", "LogitDist", "Periodic", "Quantile"]
MARG = ["ZeroOne", "Perceptron", "LogitMargin", "L1Hinge", "L2Hinge", "SmoothedL1Hinge", "ModifiedHuber", "L2Margin",
        "Exp", "Sigmoid", "DWDMargin"]
LOSS_P0 = {"LP": 1.5, "Huber": 0.5, "L1EpsilonIns": 0.25, "L2EpsilonIns": 0.25, "Periodic": 1.5, "Quantile": 0.3,
           "SmoothedL1Hinge": 0.6, "DWDMargin": 1.5}
DIST_KINKS = sorted({0.0} | {s * p for s in (-1, 1) for k, p in LOSS_P0.items() if k in DIST})
MARG_KINKS = sorted([0.0, 1.0, -1.0, 1.0 - LOSS_P0["SmoothedL1Hinge"],
                     LOSS_P0["DWDMargin"] / (LOSS_P0["DWDMargin"] + 1.0)])


def _allowed(intervals, kinks, grid):
    """The domain minus the open MARGIN-neighbourhoods of the kinks, each piece shrunk by one grid step."""
    out = []
    for lo, hi in intervals:
        cuts = [lo] + [v for k in kinks for v in (k - MARGIN, k + MARGIN)] + [hi]
        pts = sorted(set(cuts))
        for a, b in zip(pts[:-1], pts[1:]):
            mid = 0.5 * (a + b)
            if a >= lo and b <= hi and all(abs(mid - k) >= MARGIN for k in kinks) and b - a > 4 * grid:
                out.append((a + grid, b - grid))
    return out


def _draw(rng, intervals, kinks, dt, n=N):
    grid = GRID[dt]
    pieces = _allowed(intervals, kinks, grid)
    w = np.array([b - a for a, b in pieces])
    which = rng.choice(len(pieces), size=n, p=w / w.sum())
    u = rng.random(n)
    x = np.array([pieces[k][0] + t * (pieces[k][1] - pieces[k][0]) for k, t in zip(which, u)])
    x = np.round(x / grid) * grid
    x = x.astype(NP[dt])
    x64 = x.astype(np.float64)
    assert np.array_equal(np.round(x64 / grid) * grid, x64), "inputs are grid points"
    assert all(any(lo <= v <= hi for lo, hi in intervals) for v in x64), "inputs lie in the domain"
    for k in kinks:
        assert np.all(np.abs(x64 - k) >= MARGIN), ("kink margin", k)
    return x


def _draw_pairs(rng, ia, ib, dt, accept):
    """Pairs (a, b) from the two 1-D draws, redrawn here (never at test time) until accept(a, b) holds."""
    a = _draw(rng, *ia, dt)
    b = _draw(rng, *ib, dt)
    for _ in range(200):
        bad = ~accept(a.astype(np.float64), b.astype(np.float64))
        if not bad.any():
            return a, b
        a[bad] = _draw(rng, *ia, dt, n=int(bad.sum()))
        b[bad] = _draw(rng, *ib, dt, n=int(bad.sum()))
    raise AssertionError("pair draw did not converge")


def make_inputs():
    """Every input set, from the fixed seed: {key: array}."""
    z = {}
    for dt in ("f32", "f64"):
        rng = np.random.default_rng([20240611, 32 if dt == "f32" else 64])
        z[f"un_x_{dt}"] = np.stack([_draw(rng, iv, kinks, dt) for _, iv, kinks in UN_DOMAINS])
        pm2 = ([(-2.0, 2.0)], [])
        pm2nz = ([(-2.0, 2.0)], [0.0])
        sets = {}
        sets["gen"] = _draw_pairs(rng, pm2nz, pm2nz, dt,
                                  lambda a, b: (np.abs(a - b) >= MARGIN) & (a * a + b * b >= 0.25))
        sets["div"] = _draw_pairs(rng, pm2, ([(-4.0, -0.25), (0.25, 4.0)], []), dt, lambda a, b: a == a)
        sets["pow"] = _draw_pairs(rng, ([(0.25, 4.0)], []), pm2, dt, lambda a, b: a == a)
        a = _draw(rng, [(-4.0, -0.25)], [], dt)
        sets["powneg"] = (a, rng.choice(np.array([-3.0, -2.0, 2.0, 3.0]), size=N).astype(NP[dt]))
        # mod: a = q b rounded to the grid, the fractional part of q in [1/16, 15/16] with room for the rounding
        grid = GRID[dt]
        b = _draw(rng, [(-2.0, -0.75), (0.75, 2.0)], [], dt)
        q = rng.integers(-3, 3, size=N) + (MARGIN + 2.0 ** -10 + rng.random(N) * (1 - 2 * MARGIN - 2.0 ** -9))
        a = (np.round(q * b.astype(np.float64) / grid) * grid).astype(NP[dt])
        sets["mod"] = (a, b)
        z[f"bin_a_{dt}"] = np.stack([sets[s][0] for s in BIN_SETS])
        z[f"bin_b_{dt}"] = np.stack([sets[s][1] for s in BIN_SETS])
        z[f"loss_d_{dt}"] = _draw(rng, [(-2.0, 2.0)], DIST_KINKS, dt)
        z[f"loss_a_{dt}"] = _draw(rng, [(-2.5, 2.5)], MARG_KINKS, dt)
        # the margins of the pair sets, from the inputs alone
        ga, gb = (v.astype(np.float64) for v in sets["gen"])
        assert np.all(np.abs(ga) >= MARGIN) and np.all(np.abs(gb) >= MARGIN) and np.all(np.abs(ga - gb) >= MARGIN)
        assert np.all(ga * ga + gb * gb >= 0.25)
        db = sets["div"][1].astype(np.float64)
        assert np.all((np.abs(db) >= 0.25) & (np.abs(db) <= 4))
        pa, pb = (v.astype(np.float64) for v in sets["pow"])
        assert np.all((pa >= 0.25) & (pa <= 4) & (np.abs(pb) <= 2))
        na, nb = (v.astype(np.float64) for v in sets["powneg"])
        assert np.all((na <= -0.25) & (na >= -4) & np.isin(nb, [-3, -2, 2, 3]))
    return z


# ---- the exact rules (mpmath) --------------------------------------------------------------------
def _rules(mp):
    one = mp.mpf(1)
    ln2, ln10 = mp.log(2), mp.log(10)

    def wrap(x):  # atanh_clip's argument: mod(x + 1, 2) - 1
        return x + 1 - 2 * mp.floor((x + 1) / 2) - 1

    un = {
        "cos": lambda x: -mp.sin(x), "sin": mp.cos, "exp": mp.exp, "exp2": lambda x: ln2 * mp.power(2, x),
        "expm1": mp.exp, "sinh": mp.cosh, "cosh": mp.sinh, "tanh": lambda x: one / mp.cosh(x) ** 2,
        "atan": lambda x: one / (1 + x * x), "asinh": lambda x: one / mp.sqrt(x * x + 1),
        "erf": lambda x: 2 / mp.sqrt(mp.pi) * mp.exp(-x * x), "erfc": lambda x: -2 / mp.sqrt(mp.pi) * mp.exp(-x * x),
        "square": lambda x: 2 * x, "cube": lambda x: 3 * x * x, "neg": lambda x: -one,
        "tan": lambda x: one / mp.cos(x) ** 2, "log": lambda x: one / x, "log2": lambda x: one / (x * ln2),
        "log10": lambda x: one / (x * ln10), "sqrt": lambda x: one / (2 * mp.sqrt(x)),
        "cbrt": lambda x: one / (3 * mp.cbrt(abs(x)) ** 2), "log1p": lambda x: one / (1 + x),
        "acosh": lambda x: one / mp.sqrt(x * x - 1), "asin": lambda x: one / mp.sqrt(1 - x * x),
        "acos": lambda x: -one / mp.sqrt(1 - x * x), "atanh_clip": lambda x: one / (1 - wrap(x) ** 2),
        "abs": lambda x: mp.sign(x), "relu": lambda x: one if x > 0 else 0 * one, "sign": lambda x: 0 * one,
        "floor": lambda x: 0 * one, "ceil": lambda x: 0 * one, "round": lambda x: 0 * one,
    }
    bn = {
        "+": lambda a, b: (one, one), "-": lambda a, b: (one, -one), "*": lambda a, b: (b, a),
        "/": lambda a, b: (one / b, -a / (b * b)),
        "^": lambda a, b: (b * mp.power(a, b - 1), mp.power(a, b) * mp.log(a)),
        # a < 0, integer b: d/da = b a^(b-1); d/db is the device's convention (0), not a derivative
        "^neg": lambda a, b: (b * mp.power(a, b - 1), 0 * one),
        "mod": lambda a, b: (one, -mp.floor(a / b)),
        "atan2": lambda a, b: (b / (a * a + b * b), -a / (a * a + b * b)),
        "max": lambda a, b: (one, 0 * one) if a > b else (0 * one, one),
        "min": lambda a, b: (one, 0 * one) if a < b else (0 * one, one),
        "greater": lambda a, b: (0 * one, 0 * one),
        "cond": lambda a, b: (0 * one, one if a > 0 else 0 * one),
        "logical_or": lambda a, b: (0 * one, 0 * one), "logical_and": lambda a, b: (0 * one, 0 * one),
    }
    P = {k: mp.mpf(v) for k, v in LOSS_P0.items()}
    q = P["DWDMargin"]
    g = P["SmoothedL1Hinge"]
    kper = 2 * mp.pi / P["Periodic"]
    ls = {
        "L2": lambda d: 2 * d, "L1": mp.sign, "LP": lambda d: P["LP"] * mp.power(abs(d), P["LP"] - 1) * mp.sign(d),
        "Huber": lambda d: d if abs(d) <= P["Huber"] else P["Huber"] * mp.sign(d),
        "L1EpsilonIns": lambda d: mp.sign(d) if abs(d) > P["L1EpsilonIns"] else 0 * one,
        "L2EpsilonIns": lambda d: 2 * (abs(d) - P["L2EpsilonIns"]) * mp.sign(d) if abs(d) > P["L2EpsilonIns"] else 0 * one,
        "LogitDist": lambda d: mp.tanh(d / 2), "Periodic": lambda d: kper * mp.sin(kper * d),
        "Quantile": lambda d: P["Quantile"] - (1 if d < 0 else 0),
        "ZeroOne": lambda a: 0 * one, "Perceptron": lambda a: -one if a < 0 else 0 * one,
        "LogitMargin": lambda a: -one / (1 + mp.exp(a)), "L1Hinge": lambda a: -one if a < 1 else 0 * one,
        "L2Hinge": lambda a: 2 * (a - 1) if a < 1 else 0 * one,
        "SmoothedL1Hinge": lambda a: 0 * one if a >= 1 else ((a - 1) / g if a >= 1 - g else -one),
        "ModifiedHuber": lambda a: -4 * one if a < -1 else (2 * (a - 1) if a < 1 else 0 * one),
        "L2Margin": lambda a: 2 * (a - 1), "Exp": lambda a: -mp.exp(-a), "Sigmoid": lambda a: -one / mp.cosh(a) ** 2,
        "DWDMargin": lambda a: -one if a <= q / (q + 1) else -mp.power(q / (q + 1), q + 1) / mp.power(a, q + 1),
    }
    return un, bn, ls


def build_table():
    """The whole table as {key: array} (needs mpmath)."""
    import mpmath as mp

    mp.mp.dps = 40
    un, bn, ls = _rules(mp)
    z = make_inputs()
    z["un_ops"] = np.array([o for o, _ in UN_OPS])
    z["un_dom"] = np.array([_DOM[d] for _, d in UN_OPS], dtype=np.int32)
    z["bin_cases"] = np.array([c for c, _ in BIN_CASES])
    z["bin_set"] = np.array([BIN_SETS.index(s) for _, s in BIN_CASES], dtype=np.int32)
    z["loss_kinds"] = np.array(DIST + MARG)

    def f64(v):
        return float(mp.mpf(v))  # one rounding, to nearest

    for dt in ("f32", "f64"):
        ux = z[f"un_x_{dt}"]
        z[f"un_df_{dt}"] = np.array([[f64(un[o](mp.mpf(float(x)))) for x in ux[_DOM[d]]] for o, d in UN_OPS])
        fa, fb = [], []
        for c, s in BIN_CASES:
            k = BIN_SETS.index(s)
            pr = [bn[c](mp.mpf(float(a)), mp.mpf(float(b))) for a, b in zip(z[f"bin_a_{dt}"][k], z[f"bin_b_{dt}"][k])]
            fa.append([f64(p[0]) for p in pr])
            fb.append([f64(p[1]) for p in pr])
        z[f"bin_fa_{dt}"] = np.array(fa)
        z[f"bin_fb_{dt}"] = np.array(fb)
        # mod's margin: the fractional part of a / b, exactly
        k = BIN_SETS.index("mod")
        for a, b in zip(z[f"bin_a_{dt}"][k], z[f"bin_b_{dt}"][k]):
            qq = mp.mpf(float(a)) / mp.mpf(float(b))
            fr = qq - mp.floor(qq)
            assert MARGIN <= fr <= 1 - MARGIN, ("mod margin", a, b)
        z[f"loss_dl_{dt}"] = np.array(
            [[f64(ls[kd](mp.mpf(float(v)))) for v in z[f"loss_d_{dt}" if kd in DIST else f"loss_a_{dt}"]]
             for kd in DIST + MARG])
    return z


TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "derivative_rules.npz")


def _planes(a):
    """A float array as its byte planes, uint8 [itemsize, *shape] (little-endian): the sign / exponent
    bytes of neighbouring values then lie together and deflate well, which keeps the file under its limit."""
    a = np.ascontiguousarray(a, dtype=a.dtype.newbyteorder("<"))
    return np.ascontiguousarray(a.reshape(-1).view(np.uint8).reshape(-1, a.itemsize).T).reshape((a.itemsize,) + a.shape)


def _unplanes(p):
    dt = {4: "<f4", 8: "<f8"}[p.shape[0]]
    return np.ascontiguousarray(p.reshape(p.shape[0], -1).T).view(dt).reshape(p.shape[1:]).astype(dt[1:])


def load_table(path=TABLE):
    """The committed table as {key: array}: float arrays are stored as byte planes (_planes)."""
    z = np.load(path, allow_pickle=False)
    return {k: (_unplanes(z[k]) if z[k].dtype == np.uint8 else z[k]) for k in z.files}


def main():
    out = TABLE
    z = build_table()
    np.savez_compressed(out, **{k: (_planes(v) if v.dtype.kind == "f" else v) for k, v in z.items()})
    back = load_table(out)
    assert set(back) == set(z) and all(back[k].dtype == z[k].dtype and np.array_equal(back[k], z[k]) for k in z)
    size = os.path.getsize(out)
    print(f"{out}: {size} bytes")
    assert size < 256 * 1024, "the table must stay under 256 KB"
    return 0


if __name__ == "__main__":
    sys.exit(main())
