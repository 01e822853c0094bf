"""Every forward operator in every operand form of the interpreter (csrc/srhip_eval_impl.h) against exact
math: the golden table tests/golden/forward_values.npz through the trees of tests/forward_values_common.py
(tests/test_forward_values_table.py shows, without a device, that they compile to every handler).

Bars, per class of the table (no tolerance is taken from what the device returns): exact and rounded-once
operators bit for bit, zero signs included; Float32 exp sin cos tan within 1 ulp; Float64 non-exact operators
within the project's relative bar (1e-14; 1e-13 for gamma and ^); NaN exactly where the table has NaN.

Seven kernel variants: Float32 K = 2 below 4096 rows (R = 8), K = 2 on the tiled data (R = 16, ragged last
tile), K = 4, K = 8; Float64 K = 2, 4, 8.  The K = 4 and K = 8 programs hold the shallower trees too; the wide
operators (asin acos atanh_clip) exist only in the K = 8 kernels, so their trees are in the K = 8 program alone."""
import numpy as np
import pytest

import forward_values_common as fv
from test_gpu_parity import F32_REL, F64_REL

pytestmark = pytest.mark.gpu

CASES = [(dt, K) for dt in ("f32", "f64") for K in (2, 4, 8)]
_CACHE = {}


def _sr():
    import srhip

    return srhip


def _program(ctx, dt, K):
    sr = _sr()
    if ("prog", dt, K) not in _CACHE:
        opts, sel, nodes, offs = fv.program_nodes(sr, dt, K)
        _CACHE["prog", dt, K] = sr.Program(ctx, nodes, offs, opts, fv.NP[dt])
    return _CACHE["prog", dt, K]


def _oracle_ok(oracle, dt, K, which):
    """The oracle's did_succeed of the (dt, K) trees on a dataset, computed once."""
    key = ("ok", dt, K, which)
    if key not in _CACHE:
        opts, sel, nodes, offs = fv.program_nodes(_sr(), dt, K)
        d = fv.data(dt, which)
        _CACHE[key] = oracle.eval_loss_batch(nodes, offs, opts.binop_codes, opts.unaop_codes, d.X,
                                             np.zeros(d.n, fv.NP[dt]))[2]
    return _CACHE[key]


def _check_predictions(dt, sel, d, pred, trees=None):
    bad = []
    for t, tree in enumerate(sel):
        if trees is not None and t not in trees:
            continue
        want, mask = fv.expected(d, tree)
        rows = fv.failing_rows(tree["op"], dt, pred[t], want, mask)
        bad += [(tree["label"], int(r), [float(v) for v in d.X[:, r][[fv.un_feature(tree["op"]) - 1] if tree["kind"] == "un"
                                                                     else [f - 1 for f in fv.bin_features(tree["op"])]]],
                 float(pred[t][r]), float(want[r])) for r in rows[:3]]
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("which", ["general", "tiled", "special"])
@pytest.mark.parametrize("dt,K", CASES)
def test_every_form_meets_its_class_bar(ctx, oracle, dt, K, which):
    """Predictions of every tree on every row that counts; did_succeed equal to the oracle's, and true for
    every tree whose tabulated results are all finite (general data)."""
    sr = _sr()
    opts, sel, nodes, offs = fv.program_nodes(sr, dt, K)
    d = fv.data(dt, which)
    prog = _program(ctx, dt, K)
    assert prog.stats()["max_stack"] == K  # with the options' wide operators, the kernel variant run
    pred, ok = prog.eval_predict(sr.DeviceDataset(ctx, d.X))
    _check_predictions(dt, sel, d, pred)
    # the tiled data repeats the general points: the same decisions
    ook = _oracle_ok(oracle, dt, K, "general" if which == "tiled" else which)
    assert np.array_equal(ok, ook), [(sel[t]["label"], bool(ok[t])) for t in np.nonzero(ok != ook)[0][:10]]
    if which != "special":
        for t, tree in enumerate(sel):
            want, mask = fv.expected(d, tree)
            if tree["row"] is None and np.isfinite(want[mask]).all():
                assert ok[t], tree["label"]


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_derived_columns_match_the_plain_program_and_the_table(ctx, monkeypatch, dt):
    """U(x) used twice is a derived column (forced on the device with SRHIP_DERIVE_ALWAYS=1): the same bits
    as the program compiled with SRHIP_NO_DERIVE=1, and the table's values."""
    sr = _sr()
    T = fv.NP[dt]
    for K in (2, 4):  # between them every derivable operator has its column (16 per program)
        opts, sel, nodes, offs = fv.program_nodes(sr, dt, K)
        d = fv.data(dt, "tiled")
        ds = sr.DeviceDataset(ctx, d.X)
        monkeypatch.setenv("SRHIP_DERIVE_ALWAYS", "1")
        dprog = sr.Program(ctx, nodes, offs, opts, T)
        cols = dprog.derived_columns()
        assert len(cols) == 16
        a, aok = dprog.eval_predict(ds)
        monkeypatch.setenv("SRHIP_NO_DERIVE", "1")
        plain = sr.Program(ctx, nodes, offs, opts, T)
        assert plain.derived_columns() == []
        b, bok = plain.eval_predict(ds)
        monkeypatch.delenv("SRHIP_NO_DERIVE")
        monkeypatch.delenv("SRHIP_DERIVE_ALWAYS")
        un = [t for t, tree in enumerate(sel) if tree["kind"] == "un"]
        assert np.array_equal(aok, bok)
        for t in un:
            assert (fv.bits_equal(a[t], b[t]) | (np.isnan(a[t]) & np.isnan(b[t]))).all(), sel[t]["label"]
        _check_predictions(dt, sel, d, a, trees=set(un))
        _check_predictions(dt, sel, d, b, trees=set(un))


@pytest.mark.parametrize("dt,K", CASES)
def test_loss_mode_hot_form_included(ctx, monkeypatch, dt, K):
    """L1 loss against y = 0 on the tiled data: each ok tree's loss is the mean of |tabulated value| (summed
    in Float64) within the parity bar.  The Float32 K = 2 program runs as a hot-form launch; the general
    persistent form and the grid launch return the same bits."""
    sr = _sr()
    opts, sel, nodes, offs = fv.program_nodes(sr, dt, K)
    d = fv.data(dt, "tiled")
    ds = sr.DeviceDataset(ctx, d.X, np.zeros(d.n, fv.NP[dt]))
    prog = _program(ctx, dt, K)
    h0 = ctx.hot_form_launches()
    loss, ok = prog.eval_loss(ds, sr.L1DistLoss())
    if (dt, K) == ("f32", 2):
        assert ctx.hot_form_launches() == h0 + 1, "not a hot-form launch"
        for flag in ("SRHIP_NO_HOT_FORM", "SRHIP_NO_PERSISTENT"):
            monkeypatch.setenv(flag, "1")
            l2, ok2 = prog.eval_loss(ds, sr.L1DistLoss())
            monkeypatch.delenv(flag)
            assert np.array_equal(ok, ok2), flag
            assert np.array_equal(loss.view(np.uint64), l2.view(np.uint64)), flag
        assert ctx.hot_form_launches() == h0 + 1
    tol = F32_REL if dt == "f32" else F64_REL
    bad, checked = [], 0
    for t, tree in enumerate(sel):
        want, mask = fv.expected(d, tree)
        if tree["row"] is not None or not ok[t]:
            continue
        ref = np.abs(want.astype(np.float64)).sum() / d.n
        checked += 1
        if not abs(loss[t] - ref) <= tol * abs(ref):
            bad.append((tree["label"], loss[t], ref))
    assert not bad, bad[:10]
    assert checked > len(sel) // 3


def test_int32_forms_bit_for_bit(ctx):
    """The ring operators and comparisons in every operand form on Int32 edge values, against Python
    integers wrapped to 32 bits, in the K = 2, 4 and 8 kernels."""
    sr = _sr()
    opts, trees, X, want = fv.int_problem(sr)
    ds = sr.DeviceDataset(ctx, X)
    for K in (2, 4, 8):
        sel = [t for t in trees if t["need"] <= K]
        nodes, offs = sr.flatten([t["tree"] for t in sel], opts, np.int32)
        prog = sr.Program(ctx, nodes, offs, opts, np.int32)
        assert prog.stats()["max_stack"] == K
        pred, ok = prog.eval_predict(ds)
        assert ok.all()
        bad = []
        for t, tree in enumerate(sel):
            v, mask = want(tree)
            rows = np.nonzero(mask & (pred[t] != v))[0]
            bad += [(K, tree["label"], int(X[0, r]), int(X[fv.NUN + 1, r]), int(pred[t][r]), int(v[r])) for r in rows[:3]]
        assert not bad, (len(bad), bad[:10])


def device_worst_ulps(ctx, dt):
    """{operator: worst error in ulp over the finite tabulated points, every form and dataset}."""
    sr = _sr()
    opts, sel, nodes, offs = fv.program_nodes(sr, dt, 8)
    prog = _program(ctx, dt, 8)
    out = {}
    for which in ("general", "special"):
        d = fv.data(dt, which)
        pred, _ = prog.eval_predict(sr.DeviceDataset(ctx, d.X))
        for t, tree in enumerate(sel):
            want, mask = fv.expected(d, tree)
            m = mask & np.isfinite(want) & np.isfinite(pred[t])
            if m.any():
                out[tree["op"]] = max(out.get(tree["op"], 0.0), float(fv.ulp_distance(pred[t], want)[m].max()))
    return out
