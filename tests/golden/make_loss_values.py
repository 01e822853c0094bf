"""Generator of tests/golden/loss_values.npz: exact values of the 20 built-in elementwise losses (the bodies
loss_elem and margin_loss of csrc/srhip_ops.h), by mpmath at 40 digits.

    python tests/golden/make_loss_values.py          # rewrites loss_values.npz

Needs mpmath (1.3.0 when the committed table was made); the tests only read the table, and
tests/test_loss_values_table.py regenerates it in memory (build_table) where mpmath can be imported.

The conventions are those of make_derivative_rules.py, whose loss names, parameters and kink lists are
imported, not restated: inputs stored in the dtype they are used in (D = "f32" / "f64"), every value
evaluated at the exact stored input and rounded once to Float64, float arrays stored as byte planes, the
file under 256 KB.  Definitions: the published LossFunctions.jl ones, distance losses of d = pred - y,
margin losses of a = y * pred, ZeroOne 1 for a < 0 and 0 at both zeros.  The parameter of a loss is the
one the kernel sees, T(p0) (`const T p0 = (T)p.loss_p0`): the Float32 rows of Quantile are evaluated at
Float32's 0.3, not at the decimal.

  loss_kinds [20]                  loss names, the nine distance losses first
  loss_l_D [20, 300]               general: l at the residuals loss_d_D (distance losses) or agreements
                                   loss_a_D (margin losses) of derivative_rules.npz, which are read from
                                   that file and not stored again
  kink_d_D [30], kink_a_D [18]     kinks: prev_T(k), k, next_T(k) for every nonzero kink of DIST_KINKS /
                                   MARG_KINKS, k being the value the kernel computes in T from the rounded
                                   parameters (kernel_kink); at 0: -0.0, +0.0, +-2^-30, +-2^-10 (no
                                   subnormals: whether they flush is not decided here)
  kink_ld_D [9, 30], kink_la_D [11, 18]     every kind at every point of its family (a kink of one loss
                                   is an ordinary point for the others)
  ext_d_D, ext_a_D                 extreme: points where the formula in T leaves exact math (overflow,
                                   underflow, Inf / Inf); the exact value is stored all the same, and the
                                   tests compare the class (NaN, +Inf, -Inf, finite) with the CPU
                                   restatement of the formula in T, and finite results with the table
  ext_ld_D [9, .], ext_la_D [11, .]
  par_d_D [6], par_l_D [6]         parameter: PAR_KIND (a kind that rounds at most once, so the tests demand
                                   equality) at PAR_P0 = 0.3, which Float32 does not hold, at d = +-(prev_T,
                                   T(0.3), next_T): exact math at T(0.3) is 0 at |d| = T(0.3), and a kernel
                                   that used the decimal 0.3 would return T(0.3) - 0.3 = 1.2e-8 there
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _rules_module():
    spec = importlib.util.spec_from_file_location("make_derivative_rules", os.path.join(HERE, "make_derivative_rules.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RULES = _rules_module()
DIST, MARG, LOSS_P0 = RULES.DIST, RULES.MARG, RULES.LOSS_P0
DIST_KINKS, MARG_KINKS = RULES.DIST_KINKS, RULES.MARG_KINKS
NP = RULES.NP
TABLE = os.path.join(HERE, "loss_values.npz")

EXT_D = {"f32": [40.0, -40.0, 50.0, -50.0, 100.0, -100.0, 1e13, 1e20, 1e30],
         "f64": [400.0, -400.0, 800.0, -800.0, 1e103, 1e160]}
EXT_A = {"f32": [50.0, -50.0, 100.0, -100.0], "f64": [400.0, -400.0, 800.0, -800.0]}
PAR_KIND, PAR_P0 = "L1EpsilonIns", 0.3


def kernel_kink(k, dt):
    """The kink k of DIST_KINKS / MARG_KINKS as the kernel computes it in T from the rounded parameters:
    T(1) - T(gamma) for SmoothedL1Hinge (Float32: 0.39999998, one below T(0.4)), T(q) / (T(q) + 1) for
    DWDMargin, T(k) for the others (the parameter itself, or a constant)."""
    T = NP[dt]
    g, q = T(LOSS_P0["SmoothedL1Hinge"]), T(LOSS_P0["DWDMargin"])
    if k == 1.0 - LOSS_P0["SmoothedL1Hinge"]:
        return T(1) - g
    if k == LOSS_P0["DWDMargin"] / (LOSS_P0["DWDMargin"] + 1.0):
        return q / (q + T(1))
    return T(k)


def kink_points(kinks, dt, margin=False):
    """prev_T(k), k, next_T(k) per nonzero kink k (as the kernel sees it); around 0 the six points above."""
    T = NP[dt]
    out = []
    for k in kinks:
        if k == 0.0:
            out += [T(-0.0), T(0.0), T(2.0 ** -30), T(-2.0 ** -30), T(2.0 ** -10), T(-2.0 ** -10)]
        else:
            k = kernel_kink(k, dt) if margin else T(k)
            out += [np.nextafter(k, T(-np.inf)), k, np.nextafter(k, T(np.inf))]
    return np.array(out, dtype=T)


def make_inputs():
    """The kink and extreme inputs per dtype: {key: array} (the general inputs are derivative_rules.npz's)."""
    z = {}
    for dt in ("f32", "f64"):
        z[f"kink_d_{dt}"] = kink_points(DIST_KINKS, dt)
        z[f"kink_a_{dt}"] = kink_points(MARG_KINKS, dt, margin=True)
        p = NP[dt](PAR_P0)
        z[f"par_d_{dt}"] = np.array([s * v for s in (1, -1) for v in (np.nextafter(p, NP[dt](0)), p, np.nextafter(p, NP[dt](1)))],
                                    dtype=NP[dt])
        z[f"ext_d_{dt}"] = np.array(EXT_D[dt], dtype=NP[dt])
        z[f"ext_a_{dt}"] = np.array(EXT_A[dt], dtype=NP[dt])
        assert np.isfinite(z[f"ext_d_{dt}"]).all() and np.isfinite(z[f"ext_a_{dt}"]).all()
    return z


# ---- the exact values (mpmath) ----------------------------------------------------------------------
def _values(mp, dt, p0=LOSS_P0):
    """{kind: l(x)} with the parameters p0 rounded to T, as the kernel sees them."""
    T = NP[dt]
    P = {k: mp.mpf(float(T(v))) for k, v in p0.items()}
    zero, one = mp.mpf(0), mp.mpf(1)
    q, g = P["DWDMargin"], P["SmoothedL1Hinge"]

    def pos(x):
        return x if x > 0 else zero

    return {
        "L2": lambda d: d * d, "L1": lambda d: abs(d),
        "LP": lambda d: mp.power(abs(d), P["LP"]) if d != 0 else zero,
        "Huber": lambda d: d * d / 2 if abs(d) <= P["Huber"] else P["Huber"] * (abs(d) - P["Huber"] / 2),
        "L1EpsilonIns": lambda d: pos(abs(d) - P["L1EpsilonIns"]),
        "L2EpsilonIns": lambda d: pos(abs(d) - P["L2EpsilonIns"]) ** 2,
        # -log(4 e^d / (1 + e^d)^2), in the form that stays finite: 2 log(1 + e^-|d|) + |d| - log 4
        "LogitDist": lambda d: 2 * mp.log1p(mp.exp(-abs(d))) + abs(d) - mp.log(4),
        "Periodic": lambda d: 1 - mp.cos(2 * mp.pi * d / P["Periodic"]),
        "Quantile": lambda d: d * (P["Quantile"] - (1 if d < 0 else 0)),
        "ZeroOne": lambda a: one if a < 0 else zero, "Perceptron": lambda a: pos(-a),
        "LogitMargin": lambda a: mp.log1p(mp.exp(-a)), "L1Hinge": lambda a: pos(1 - a),
        "L2Hinge": lambda a: zero if a >= 1 else (1 - a) ** 2,
        "SmoothedL1Hinge": lambda a: pos(1 - a) ** 2 / (2 * g) if a >= 1 - g else 1 - g / 2 - a,
        "ModifiedHuber": lambda a: pos(1 - a) ** 2 if a >= -1 else -4 * a,
        "L2Margin": lambda a: (1 - a) ** 2, "Exp": lambda a: mp.exp(-a), "Sigmoid": lambda a: 1 - mp.tanh(a),
        "DWDMargin": lambda a: 1 - a if a <= q / (q + 1) else mp.power(q, q) / mp.power(q + 1, q + 1) / mp.power(a, q),
    }


def build_table():
    """The whole table as {key: array} (needs mpmath)."""
    import mpmath as mp

    mp.mp.dps = 40
    gen = RULES.load_table()
    z = make_inputs()
    z["loss_kinds"] = np.array(DIST + MARG)
    assert list(gen["loss_kinds"]) == DIST + MARG

    def f64(v):
        v = mp.mpf(v)
        return float(v) if abs(v) < mp.mpf(2) ** 1024 else float(mp.sign(v)) * np.inf  # one rounding, to nearest

    def tab(kinds, f, x):
        return np.array([[f64(f[k](mp.mpf(float(v)))) for v in x] for k in kinds], dtype=np.float64)

    for dt in ("f32", "f64"):
        f = _values(mp, dt)
        z[f"loss_l_{dt}"] = np.concatenate([tab(DIST, f, gen[f"loss_d_{dt}"]), tab(MARG, f, gen[f"loss_a_{dt}"])])
        for blk in ("kink", "ext"):
            z[f"{blk}_ld_{dt}"] = tab(DIST, f, z[f"{blk}_d_{dt}"])
            z[f"{blk}_la_{dt}"] = tab(MARG, f, z[f"{blk}_a_{dt}"])
        fp = _values(mp, dt, {**LOSS_P0, PAR_KIND: PAR_P0})
        z[f"par_l_{dt}"] = tab([PAR_KIND], fp, z[f"par_d_{dt}"])[0]
        assert not np.isnan(z[f"ext_ld_{dt}"]).any() and not np.isnan(z[f"ext_la_{dt}"]).any()
        assert np.isfinite(z[f"kink_ld_{dt}"]).all() and np.isfinite(z[f"kink_la_{dt}"]).all()
    return z


def load_table(path=TABLE):
    """The committed table as {key: array}: float arrays are stored as byte planes."""
    return RULES.load_table(path)


def main():
    out = TABLE
    z = build_table()
    np.savez_compressed(out, **{k: (RULES._planes(v) if v.dtype.kind == "f" else v) for k, v in z.items()})
    back = load_table(out)
    assert set(back) == set(z)
    assert all(back[k].dtype == z[k].dtype and back[k].tobytes() == z[k].tobytes() for k in z)
    size = os.path.getsize(out)
    print(f"{out}: {size} bytes")
    assert size < 256 * 1024, "the table must stay under 256 KB"
    return 0


if __name__ == "__main__":
    sys.exit(main())
