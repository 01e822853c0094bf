"""The hot form of the interpreter kernel (the persistent main launch of the wide
Float32 loss kernel, with one 16-byte record per order slot read by a scalar load) returns what the
grid launch returns, bit for bit, and what the oracle returns, at the smallest shapes where its
slot mapping, its records and its failure paths can go wrong.

Every case evaluates the same program three ways -- hot form, the general persistent form
(SRHIP_NO_HOT_FORM=1) and the grid launch (SRHIP_NO_PERSISTENT=1) -- and checks through
srhip_hot_form_launches that the first really was a hot-form launch and the others were not."""
import numpy as np
import pytest

import srhip
from srhip import workloads
from test_gpu_parity import F32_REL

pytestmark = pytest.mark.gpu

LATE = 7  # rows from the end where x2 = 100: exp(x2) overflows there and nowhere else


def _special_trees():
    """Hand-built trees on top of the random ones (all within two stack slots)."""
    N = srhip.Node
    x1, x2, x3, x4 = N("x1"), N("x2"), N("x3"), N("x4")
    return [
        srhip.exp(x1 * N(val=1000.0)),                       # fails in the first tile (x1 > 0.09 there)
        x3 / N(val=0.0),                                     # Inf on every row
        srhip.exp(x2),                                       # fails only at row n - LATE
        srhip.exp(x2) * x1 + srhip.cos(x2),                  # ... through a derived column, in a longer tree
        x1 + srhip.exp(srhip.exp(N(val=100.0))),             # statically failing (constant subtree)
        N(val=3e38) * N(val=10.0),                           # statically failing (constant overflow)
        x3,                                                  # one-leaf trees
        N(val=1.25),
        srhip.cos(x4) * N(val=2.0) + x1 * x1 - N(val=2.0),   # reads a derived column; the data's own law
        srhip.cos(x1) + srhip.exp(srhip.cos(x4)),            # two derived columns
    ]


def _case(ntrees, rows, nfeat=5, seed=0, weighted=False, leaf=None):
    """(opts, X, y, w, nodes, offs, index of the first special tree): a C2-style random population plus the special trees; x2 = 100 at
    one late row; nfeat > 5: extra N(0, 1) feature columns; leaf: a one-leaf tree of that feature
    (sets the program's staged feature count)."""
    opts, X, y, trees, _, _ = workloads.c2(seed, ntrees - len(_special_trees()) - (leaf is not None), rows)
    rng = np.random.default_rng(100 + seed)
    if nfeat > 5:
        X = np.concatenate([X, rng.standard_normal((nfeat - 5, rows)).astype(np.float32)])
    X = np.ascontiguousarray(X)
    X[1, rows - LATE] = 100.0
    sp0 = len(trees)
    trees = list(trees) + _special_trees()
    if leaf is not None:
        trees.append(srhip.Node(f"x{leaf}"))
    nodes, offs = srhip.flatten(trees, opts, np.float32)
    w = np.abs(rng.standard_normal(rows)).astype(np.float32) if weighted else None
    return opts, X, y, w, nodes, offs, sp0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _three_ways(ctx, monkeypatch, prog, ds, loss, env=()):
    """eval_loss by the hot form, the general persistent form and the grid launch; asserts which form
    ran and that all three agree bit for bit; returns the hot form's (losses, ok)."""
    for k, v in env:
        monkeypatch.setenv(k, v)
    h0 = ctx.hot_form_launches()
    l, ok = prog.eval_loss(ds, loss)
    assert ctx.hot_form_launches() == h0 + 1, "not a hot-form launch"
    others = []
    for flag in ("SRHIP_NO_HOT_FORM", "SRHIP_NO_PERSISTENT"):
        monkeypatch.setenv(flag, "1")
        others.append((flag, *prog.eval_loss(ds, loss)))
        monkeypatch.delenv(flag)
    assert ctx.hot_form_launches() == h0 + 1
    for k, _ in env:
        monkeypatch.delenv(k)
    for flag, l2, ok2 in others:
        assert np.array_equal(ok, ok2), (flag, np.nonzero(ok != ok2)[0][:8])
        diff = np.nonzero(_bits(l) != _bits(l2))[0]
        assert not len(diff), (flag, [(int(t), l[t], l2[t]) for t in diff[:8]])
    return l.copy(), ok.copy()


def _oracle(oracle, opts, nodes, offs, X, y, w, loss, l, ok):
    ol, _, ook, _ = oracle.eval_loss_batch(nodes, offs, opts.binop_codes, opts.unaop_codes, X, y, w, loss.kind, loss.p0)
    assert np.array_equal(ok, ook), np.nonzero(ok != ook)[0][:8]
    live = np.nonzero(ook)[0]
    rel = np.abs(l[live] - ol[live]) / np.maximum(np.abs(ol[live]), 1e-300)
    bad = live[(l[live] != ol[live]) & (rel > F32_REL)]
    assert not len(bad), [(int(t), l[t], ol[t]) for t in bad[:8]]
    assert np.all(np.isinf(l[~ok]))


def _run(ctx, oracle, monkeypatch, case, loss=None, env=(), derived=True):
    opts, X, y, w, nodes, offs, sp0 = case
    loss = loss or srhip.L2DistLoss()
    prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
    assert prog.stats()["max_stack"] <= 2  # the wide variant
    assert bool(prog.derived_columns()) == derived
    ds = srhip.DeviceDataset(ctx, X, y, w)
    l, ok = _three_ways(ctx, monkeypatch, prog, ds, loss, env)
    sp = ok[sp0:sp0 + len(_special_trees())]
    # the special trees: the first six fail, the one-leaf and derived-column trees succeed
    assert not sp[:6].any() and sp[6:10].all(), sp
    _oracle(oracle, opts, nodes, offs, X, y, w, loss, l, ok)
    prog.close()


def test_every_item_a_tail_share(ctx, oracle, monkeypatch):
    """300 trees x 150,016 rows: 74 row blocks of 2048, a 4-block probe, then 70 main blocks on more
    CUs than blocks -- every item is a share of the last round (the gw > 1 slot mapping)."""
    _run(ctx, oracle, monkeypatch, _case(300, 150_016, seed=1))


def test_whole_rounds_then_two_part_shares(ctx, oracle, monkeypatch):
    """64 trees x 131,072 rows on 8 workgroups: 60 main blocks are seven whole rounds and four
    leftover blocks dealt to eight shares, some of them in two parts."""
    _run(ctx, oracle, monkeypatch, _case(64, 131_072, seed=2), env=(("SRHIP_PERSISTENT_WGS", "8"),))


def test_slots_past_the_failure_snapshot(ctx, oracle, monkeypatch):
    """2,100 trees x 133,120 rows: order slots past the 2,048-entry failure snapshot."""
    _run(ctx, oracle, monkeypatch, _case(2100, 133_120, seed=3))


def test_weighted_generic_loss(ctx, oracle, monkeypatch):
    """A weighted dataset and a loss evaluated out of line inside the tile loop."""
    _run(ctx, oracle, monkeypatch, _case(200, 133_120, seed=4, weighted=True), loss=srhip.HuberLoss(0.7))


def test_twelve_features_no_derived_columns(ctx, oracle, monkeypatch):
    """12 staged feature columns and a program without derived columns (records with an empty mask)."""
    monkeypatch.setenv("SRHIP_NO_DERIVE", "1")
    _run(ctx, oracle, monkeypatch, _case(200, 133_120, nfeat=12, seed=5, leaf=12), derived=False)


def test_records_belong_to_program_and_plan(ctx, oracle, monkeypatch):
    """Two programs in flight through eval_loss_submit, waited in reverse order; then the first program
    on a weighted dataset whose extra column pushes the derived-column program out of LDS (19 columns
    of 2048 Float32 rows fit beside the kernel's own arrays): the plan changes to the plain program
    and its records with it."""
    loss = srhip.L2DistLoss()
    opts, X, y, _, nodes_a, offs_a, _ = _case(160, 133_120, nfeat=12, seed=6, leaf=5)
    nd = len(srhip.Program(ctx, nodes_a, offs_a, opts, np.float32).derived_columns())
    assert 6 <= nd <= 13  # (the leaf below must lie between the population's x5 and the dataset's x12)
    leaf = 19 - 1 - nd  # features + y + derived columns = 19: fits; one more column (w) does not
    case_a = _case(160, 133_120, nfeat=12, seed=6, leaf=leaf)
    nodes_a, offs_a = case_a[4], case_a[5]
    nodes_b, offs_b = _case(96, 133_120, nfeat=12, seed=7)[4:6]
    pa = srhip.Program(ctx, nodes_a, offs_a, opts, np.float32)
    pb = srhip.Program(ctx, nodes_b, offs_b, opts, np.float32)
    assert len(pa.derived_columns()) == nd
    ds = srhip.DeviceDataset(ctx, X, y)
    h0 = ctx.hot_form_launches()
    ta, tb = pa.eval_loss_submit(ds, loss), pb.eval_loss_submit(ds, loss)
    lb, okb = tb.wait()
    la, oka = ta.wait()
    assert ctx.hot_form_launches() == h0 + 2
    for prog, nodes, offs, l, ok in ((pa, nodes_a, offs_a, la, oka), (pb, nodes_b, offs_b, lb, okb)):
        l2, ok2 = _three_ways(ctx, monkeypatch, prog, ds, loss)
        assert np.array_equal(ok, ok2) and np.array_equal(_bits(l), _bits(l2))
        _oracle(oracle, opts, nodes, offs, X, y, None, loss, l, ok)
    w = np.abs(np.random.default_rng(8).standard_normal(X.shape[1])).astype(np.float32)
    dsw = srhip.DeviceDataset(ctx, X, y, w)
    lw, okw = _three_ways(ctx, monkeypatch, pa, dsw, loss)
    _oracle(oracle, opts, nodes_a, offs_a, X, y, w, loss, lw, okw)
    # ... and back on the unweighted dataset: the derived-column plan and its records again
    l3, ok3 = _three_ways(ctx, monkeypatch, pa, ds, loss)
    assert np.array_equal(ok3, oka) and np.array_equal(_bits(l3), _bits(la))
    pa.close()
    pb.close()


def test_reported_plan_is_the_launch_taken(ctx, monkeypatch):
    """32 trees x 3 features x 8,192 rows (four row blocks: no probe, whole blocks): srhip_plan_eval says
    persistent and hot, and the hot-form counter rises by exactly one over one eval_loss; with
    SRHIP_NO_HOT_FORM=1 it says not hot, the counter stays, and losses and ok flags are the same bits."""
    import ctypes

    import srhip._lib as L

    opts = workloads.c2(0, 1, 64)[0]
    N = srhip.Node
    trees = srhip.random_population(29, opts, 3, np.float32, seed=12, max_size=30)
    trees = list(trees) + [N("x3"), srhip.cos(N("x1")) * N("x2"), srhip.exp(N("x2") * N(val=1000.0))]
    nodes, offs = srhip.flatten(trees, opts, np.float32)
    rng = np.random.default_rng(12)
    X = rng.standard_normal((3, 8192)).astype(np.float32)
    y = (2 * np.cos(X[2]) + X[0] ** 2 - 2).astype(np.float32)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
    assert prog.stats()["max_stack"] <= 2
    ds = srhip.DeviceDataset(ctx, X, y)
    loss = srhip.L2DistLoss()

    def plan():  # (an MI355X: 256 CUs, 160 KB of LDS per workgroup)
        q = L.PlanQuery(dtype=L.F32, mode=0, nlive=32, m=8192, maxfeat=3, nd=len(prog.derived_columns()), kmax=2,
                        dkmax=2, have_recs=1, num_cu=256, lds_max=160 * 1024)
        out = L.PlanInfo()
        assert L.load().srhip_plan_eval(ctypes.byref(q), ctypes.byref(out)) == 0
        return out

    p = plan()
    assert (p.kind, p.hot, p.nrb, p.wgs, p.expect_items) == (1, 1, 4, 4, 4)
    h0 = ctx.hot_form_launches()
    l, ok = prog.eval_loss(ds, loss)
    assert ctx.hot_form_launches() == h0 + 1
    l, ok = l.copy(), ok.copy()
    monkeypatch.setenv("SRHIP_NO_HOT_FORM", "1")
    p = plan()
    assert (p.kind, p.hot) == (1, 0)
    l2, ok2 = prog.eval_loss(ds, loss)
    assert ctx.hot_form_launches() == h0 + 1
    assert np.array_equal(ok, ok2) and np.array_equal(_bits(l), _bits(l2))
    assert ok[:31].any() and not ok[31]
    prog.close()
