"""The golden table of exact loss values (tests/golden/loss_values.npz) and the bars of
tests/loss_values_common.py, without a device: the committed file reproduces from its generator, the CPU
restatement of every loss formula in T (oracle/sr_oracle.c) meets the bars on the general and kink blocks, and
every loss class of the package carries the kind code and parameter the table assumes.  The worst multiples
printed here are the "oracle" column of DESIGN.md's table of loss values."""
import os

import numpy as np
import pytest

import loss_values_common as C

DTS = ["f32", "f64"]


def _sr():
    import srhip

    return srhip


def test_committed_table_reproduces():
    pytest.importorskip("mpmath")
    z = C.GEN.build_table()
    back = C.GEN.load_table()
    assert set(back) == set(z)
    for k in z:
        assert back[k].dtype == z[k].dtype and back[k].shape == z[k].shape, k
        assert back[k].tobytes() == z[k].tobytes(), k
    assert os.path.getsize(C.GEN.TABLE) < 256 * 1024


def test_table_layout_and_inputs():
    """Shapes; the kink points are the neighbours in T of the kinks the kernel sees; no subnormal input."""
    z = C.table()
    for dt in DTS:
        T = C.NP[dt]
        assert z[f"loss_l_{dt}"].shape == (20, 300) and z[f"loss_l_{dt}"].dtype == np.float64
        for c, kinks, nk in (("d", C.GEN.DIST_KINKS, len(C.DIST)), ("a", C.GEN.MARG_KINKS, len(C.MARG))):
            x = z[f"kink_{c}_{dt}"]
            assert x.dtype == T and len(x) == 3 * (len(kinks) - 1) + 6
            assert z[f"kink_l{c}_{dt}"].shape == (nk, len(x)) and z[f"ext_l{c}_{dt}"].shape == (nk, len(z[f"ext_{c}_{dt}"]))
            assert z[f"ext_{c}_{dt}"].dtype == T
            for k in kinks:
                if k:
                    kk = C.GEN.kernel_kink(k, dt) if c == "a" else T(k)
                    i = int(np.nonzero(x == kk)[0][0])
                    assert x[i - 1] == np.nextafter(kk, T(-np.inf)) and x[i + 1] == np.nextafter(kk, T(np.inf))
            nz = x[x != 0]
            assert np.all(np.abs(nz) >= 2.0 ** -30)
        for kind, p in C.LOSS_P0.items():  # the kink the kernel compares with is tabulated with both neighbours
            x = z[f"kink_{'d' if kind in C.DIST else 'a'}_{dt}"]
            seen = {"SmoothedL1Hinge": T(1) - T(p), "DWDMargin": T(p) / (T(p) + T(1))}.get(kind, T(p))
            for v in (np.nextafter(seen, T(-np.inf)), seen, np.nextafter(seen, T(np.inf))):
                assert v in x, (kind, dt, v)
        p = T(C.GEN.PAR_P0)
        assert z[f"par_d_{dt}"].dtype == T and z[f"par_l_{dt}"].shape == (6,)
        assert np.array_equal(np.abs(z[f"par_d_{dt}"][:3]), [np.nextafter(p, T(0)), p, np.nextafter(p, T(1))])
    assert float(np.float32(C.GEN.PAR_P0)) != C.GEN.PAR_P0 and C.GEN.PAR_KIND in C.EXACT_KINDS


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", C.KINDS)
def test_oracle_meets_the_bars(oracle, kind, dt):
    """The formula in T against exact math on the general and kink rows (per row), and on their mean."""
    sr = _sr()
    blk = C.rows(C.family(kind), dt)
    got = C.oracle_rows(oracle, sr, kind, blk)
    assert got.dtype == C.NP[dt] and np.isfinite(got).all()
    worst = C.check_rows(kind, dt, got, blk.exact_of(kind), blk.v, "oracle rows")
    C.report("oracle_rows", kind, dt, worst)
    w = C.weights(dt, blk.n, False)
    wl = (w * got).astype(np.float64)
    mean = float(np.sum(wl) / np.sum(w.astype(np.float64)))
    C.report("oracle_mean", kind, dt, C.check_mean(kind, dt, mean, blk.exact_of(kind), blk.v, w, "oracle mean"))


@pytest.mark.parametrize("dt", DTS)
def test_oracle_on_the_parameter_block(oracle, dt):
    """L1EpsilonIns at 0.3, a parameter Float32 does not hold: the formula in T with T(0.3) equals exact math."""
    blk = C.rows("dist", dt, which=("param",))
    got = C.oracle_rows(oracle, _sr(), C.GEN.PAR_KIND, blk, loss=C.param_loss(_sr()))
    C.check_rows(C.GEN.PAR_KIND, dt, got, blk.exact_of(C.GEN.PAR_KIND), blk.v, "oracle parameter rows")
    assert got[1] == 0 and got[2] > 0


def test_an_unrounded_parameter_fails_the_parameter_block():
    """The mutation `p.loss_p0 used unrounded in Float32`, restated: the formula in Float64 with the decimal
    parameter, rounded once to Float32.  On the 20 kinds' own parameters it stays inside the bars (Quantile
    and SmoothedL1Hinge, the two whose parameter Float32 does not hold, shown here); the parameter block
    rejects it, at |d| = T(0.3)."""
    blk = C.rows("dist", "f32", which=("param",))
    d = blk.v.astype(np.float64)
    got = np.maximum(0.0, np.abs(d) - C.GEN.PAR_P0).astype(np.float32)
    with pytest.raises(AssertionError):
        C.check_rows(C.GEN.PAR_KIND, "f32", got, blk.exact_of(C.GEN.PAR_KIND), blk.v, "decimal parameter")
    assert got[1] > 0 and blk.exact_of(C.GEN.PAR_KIND)[1] == 0
    for kind, f in (("Quantile", lambda v, p: v * (p - (v < 0))),
                    ("SmoothedL1Hinge", lambda v, p: np.where(v >= 1 - p, 0.5 / p * np.maximum(0.0, 1 - v) ** 2, 1 - p / 2 - v))):
        b = C.rows(C.family(kind), "f32")
        got = f(b.v.astype(np.float64), C.LOSS_P0[kind]).astype(np.float32)
        print("LOSS_ERR decimal_parameter", kind, "f32", C.check_rows(kind, "f32", got, b.exact_of(kind), b.v))


def test_hubers_branches_agree_at_the_kink():
    """Why no value test can tell `<=` from `<` in Huber's branch: at |d| = p0 the two branches, 0.5 (d d) and
    p0 (|d| - 0.5 p0), both round to fl(p0^2) / 2, for every p0 (halving is exact)."""
    rng = np.random.default_rng(3)
    for T in (np.float32, np.float64):
        p = np.concatenate([rng.uniform(0.01, 100.0, 2000), [0.5, 0.3, 1.5]]).astype(T)
        a = T(0.5) * (p * p)
        b = p * (p - T(0.5) * p)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("dt", DTS)
def test_oracle_classes_on_the_extreme_block(oracle, dt):
    """Prints the class of the formula in T per extreme point; finite results meet the per-row bar, and the
    points that the Inf-on-the-last-row tests rely on are +Inf."""
    sr = _sr()
    inf_at = {}
    for kind in C.KINDS:
        blk = C.rows(C.family(kind), dt, which=("extreme",))
        got = C.oracle_rows(oracle, sr, kind, blk)
        cls = C.classes(got)
        print(f"LOSS_CLASS oracle {kind} {dt} " + " ".join(f"{float(x):g}:{C.CLASS_NAMES[c]}" for x, c in zip(blk.v, cls)))
        fin = cls == 0
        C.check_rows(kind, dt, got[fin], blk.exact_of(kind)[fin], blk.v[fin], "oracle extreme rows")
        inf_at[kind] = {float(x) for x, c in zip(blk.v, cls) if c == 1}
    for kind, x in C.INF_POINTS[dt]:
        assert float(C.NP[dt](x)) in inf_at[kind], (kind, dt, x)


@pytest.mark.parametrize("kind", C.KINDS)
def test_loss_class_carries_the_tables_kind_and_parameter(kind):
    import srhip._lib as L

    sr = _sr()
    obj = C.loss_object(sr, kind)
    ls = obj.c_struct()
    code = {"L2": "L2", "L1": "L1", "LP": "LP", "Huber": "HUBER", "L1EpsilonIns": "L1_EPS_INS",
            "L2EpsilonIns": "L2_EPS_INS", "LogitDist": "LOGIT_DIST", "Periodic": "PERIODIC", "Quantile": "QUANTILE",
            "ZeroOne": "ZERO_ONE", "Perceptron": "PERCEPTRON", "LogitMargin": "LOGIT_MARGIN", "L1Hinge": "L1_HINGE",
            "L2Hinge": "L2_HINGE", "SmoothedL1Hinge": "SMOOTHED_L1_HINGE", "ModifiedHuber": "MODIFIED_HUBER",
            "L2Margin": "L2_MARGIN", "Exp": "EXP", "Sigmoid": "SIGMOID", "DWDMargin": "DWD_MARGIN"}[kind]
    assert ls.kind == L.LOSS[code]
    assert ls.p0 == C.LOSS_P0.get(kind, 0.0) and ls.p1 == 0.0
    assert len({C.loss_object(sr, k).c_struct().kind for k in C.KINDS}) == 20
