"""srhip_eval_loss_rowsets: every tree on a row subset of its own in one launch (the batching mode's
fresh minibatch per score).  The contract is bit equality with srhip_eval_loss on the single tree with
idx = its set, which the coalescer's promise rests on; the oracle on the gathered rows is the second
reference (did_succeed equal, losses 1e-6 relative for Float32 / 1e-12 for Float64).

Set lengths cycle through the tile and loss-chunk edges of both element sizes (Float32: 512-row tiles,
1024-row chunks; Float64: 256 / 256) and past the per-wave staging cap (5 features and y, 40 KB per
wave: Float32 1536 rows, 1024 with weights; Float64 768 / 512), where the call evaluates the tree
through the single-subset path."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32_REL = 1e-6
F64_REL = 1e-12
LENGTHS = [1, 2, 50, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049]
N, NFEAT, NTREES = 5000, 5, 96


def _sr():
    import srhip

    return srhip


def _opts(sr):
    return sr.Options(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _b(x):
    return int(np.float64(x).view(np.uint64))


def _one_tree(sr, ctx, nodes, offs, t, opts, dtype):
    nd = nodes[offs[t]:offs[t + 1]]
    return sr.Program(ctx, nd, np.array([0, len(nd)], dtype=np.int64), opts, dtype)


def _singles(sr, ctx, ds, nodes, offs, opts, dtype, loss, idxs, which=None):
    """prog_t.eval_loss(ds, loss, idx=idx_t), one one-tree program per call."""
    which = range(len(idxs)) if which is None else which
    out = {}
    for t in which:
        p = _one_tree(sr, ctx, nodes, offs, t, opts, dtype)
        l, ok = p.eval_loss(ds, loss, idx=idxs[t])
        p.close()
        out[t] = (float(l[0]), bool(ok[0]))
    return out


def _oracle_each(oracle, nodes, offs, opts, X, y, w, idxs, kind=0, p0=0.0):
    """The oracle on each tree's gathered rows: (exact loss[T], ok[T])."""
    ol, ook = np.empty(len(idxs)), np.empty(len(idxs), dtype=bool)
    for t, i in enumerate(idxs):
        i = np.asarray(i)
        l, _, ok = oracle.eval_loss(nodes[offs[t]:offs[t + 1]], opts.binop_codes, opts.unaop_codes, X[:, i].copy(),
                                    y[i].copy(), None if w is None else w[i].copy(), kind, p0)
        ol[t], ook[t] = l, ok
    return ol, ook


def _check(loss, ok, single, ol, ook, tol, which=None):
    which = range(len(ok)) if which is None else which
    assert np.array_equal(ok, ook), np.nonzero(ok != ook)[0]
    for t in which:
        assert (bool(ok[t]), _b(loss[t])) == (single[t][1], _b(single[t][0])), (t, loss[t], single[t])
    for t in np.nonzero(ook)[0]:
        assert loss[t] == ol[t] or abs(loss[t] - ol[t]) <= tol * abs(ol[t]), (t, loss[t], ol[t])


_shared = {}


def _fixture(ctx, oracle, dtype, weighted):
    """The 96-tree case of one (dtype, weighting): data, sets, the rowsets call, the per-tree calls and
    the oracle -- computed once, shared by the tests below, never modified."""
    key = (np.dtype(dtype).name, weighted)
    if key in _shared:
        return _shared[key]
    sr = _sr()
    opts = _opts(sr)
    rng = np.random.default_rng(102)
    X = rng.standard_normal((NFEAT, N)).astype(dtype)
    y = rng.standard_normal(N).astype(dtype)
    w = np.abs(rng.standard_normal(N)).astype(dtype) if weighted else None
    idxs = [rng.integers(0, N, size=LENGTHS[t % len(LENGTHS)]) for t in range(NTREES)]
    trees = sr.random_population(NTREES, opts, NFEAT, dtype, 101, 25)
    nodes, offs = sr.flatten(trees, opts, dtype)
    ds = sr.DeviceDataset(ctx, X, y, w)
    prog = sr.Program(ctx, nodes, offs, opts, dtype)
    loss, ok = prog.eval_loss_rowsets(ds, sr.L2DistLoss(), idxs)
    kernel_ms = ctx.last_kernel_ms()
    work = ctx.last_work()
    single = _singles(sr, ctx, ds, nodes, offs, opts, dtype, sr.L2DistLoss(), idxs)
    ol, ook = _oracle_each(oracle, nodes, offs, opts, X, y, w, idxs)
    f = dict(sr=sr, opts=opts, X=X, y=y, w=w, idxs=idxs, nodes=nodes, offs=offs, ds=ds, prog=prog, loss=loss, ok=ok,
             single=single, ol=ol, ook=ook, kernel_ms=kernel_ms, work=work, dtype=dtype)
    _shared[key] = f
    return f


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parity_with_single_calls_and_oracle(ctx, oracle, dtype, weighted):
    f = _fixture(ctx, oracle, dtype, weighted)
    print(f"rowsets {np.dtype(dtype).name} weighted={weighted}: oracle ok {int(f['ook'].sum())}/{NTREES}, "
          f"kernel {f['kernel_ms']:.4f} ms, work {f['work']}")
    assert f["ook"].sum() >= 0.9 * NTREES, int(f["ook"].sum())
    _check(f["loss"], f["ok"], f["single"], f["ol"], f["ook"], F32_REL if dtype == np.float32 else F64_REL)
    assert f["kernel_ms"] > 0.0


def test_int32_bit_identical(ctx, oracle):
    sr = _sr()
    opts = sr.Options(binary_operators=("+", "-", "*"), unary_operators=("square", "neg"))
    rng = np.random.default_rng(3)
    trees = sr.random_population(24, opts, 3, np.float64, seed=4)
    for tr in trees:
        for nd in tr:
            if nd.degree == 0 and nd.constant:
                nd.val = int(rng.integers(-7, 8))
    nodes, offs = sr.flatten(trees, opts, np.int32)
    X = rng.integers(-1000, 1000, size=(3, 2053)).astype(np.int32)
    y = rng.integers(-50, 50, size=2053).astype(np.int32)
    idxs = [rng.integers(0, 2053, size=[1, 50, 511, 512, 513, 1025, 2049, 4000][t % 8]) for t in range(24)]
    ds = sr.DeviceDataset(ctx, X, y)
    prog = sr.Program(ctx, nodes, offs, opts, np.int32)
    for loss in (sr.L2DistLoss(), sr.L1DistLoss()):
        l, ok = prog.eval_loss_rowsets(ds, loss, idxs)
        single = _singles(sr, ctx, ds, nodes, offs, opts, np.int32, loss, idxs)
        ol, ook = _oracle_each(oracle, nodes, offs, opts, X, y, None, idxs, loss.kind, loss.p0)
        assert ok.all() and np.array_equal(ok, ook)
        assert [(float(l[t]), True) for t in range(24)] == [single[t] for t in range(24)]
        assert np.array_equal(l, ol)
    prog.close()


def test_did_succeed_is_per_set(ctx, oracle):
    """One Inf in x3 at row 777: only the trees that read x3 on a set holding that row fail; a bare
    constant's fill check depends on its own set's length."""
    sr = _sr()
    opts = _opts(sr)
    rng = np.random.default_rng(102)
    X = rng.standard_normal((NFEAT, N)).astype(np.float32)
    y = rng.standard_normal(N).astype(np.float32)
    X[2, 777] = np.inf
    a = sr.cos(sr.Node("x3")) * sr.Node("x1")
    b = sr.Node("x1") + sr.Node(val=1.0)
    x3 = sr.Node("x3")
    big = sr.Node(val=np.float32(3e38))
    lo, hi = np.arange(700, 750), np.arange(750, 800)
    trees = [a, b, a, b, x3, x3, big, big]
    idxs = [lo, lo, hi, hi, lo, hi, np.array([5, 9]), np.array([5])]
    nodes, offs = sr.flatten(trees, opts, np.float32)
    ds = sr.DeviceDataset(ctx, X, y)
    prog = sr.Program(ctx, nodes, offs, opts, np.float32)
    l, ok = prog.eval_loss_rowsets(ds, sr.L2DistLoss(), idxs)
    prog.close()
    single = _singles(sr, ctx, ds, nodes, offs, opts, np.float32, sr.L2DistLoss(), idxs)
    ol, ook = _oracle_each(oracle, nodes, offs, opts, X, y, None, idxs)
    assert list(ook[:4]) == [True, True, False, True] and ol[2] == np.inf, (ook, ol)
    assert list(ook[4:]) == [True, False, False, True], ook  # 2 x 3e38 overflows Float32, 1 x does not
    _check(l, ok, single, ol, ook, F32_REL)
    assert l[2] == np.inf and l[5] == np.inf and l[6] == np.inf


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_near_overflow_trees_are_settled(ctx, oracle, dtype):
    """test_gpu_precise.py's construction per set: c * x1 over positive x1 with the set's exact sum
    just below (ok) or just above (fail) the type's threshold -- every row finite, the fast bound
    undecided -- mixed among ordinary trees on 50-row sets."""
    sr = _sr()
    opts = sr.Options(binary_operators=("*", "+"), unary_operators=("cos",))
    n = 1000
    rng = np.random.default_rng(17)
    x = rng.uniform(0.25, 1.0, n).astype(dtype)
    X = np.stack([x, rng.standard_normal(n).astype(dtype)])
    y = np.zeros(n, dtype=dtype)
    thr = 2.0 ** 128 - 2.0 ** 103 if dtype == np.float32 else float(np.finfo(np.float64).max)
    trees, idxs, expect = [], [], []
    for i in range(16):
        idx = rng.integers(0, n, size=50)
        idxs.append(idx)
        if i % 2 == 0:
            k = i // 2
            s = float(np.sum(x[idx].astype(np.longdouble)))
            rel = (1 - 2e-5 * (k + 1)) if k % 2 == 0 else (1 + 2e-5 * (k + 1))
            trees.append(sr.Node(1, sr.Node(val=dtype(thr / s * rel)), sr.Node(feature=1)))  # c * x1
            expect.append(k % 2 == 0)
        else:
            trees.append(sr.Node(2, sr.Node(feature=2), sr.Node(val=1.5)))
            expect.append(True)
    nodes, offs = sr.flatten(trees, opts, dtype)
    ds = sr.DeviceDataset(ctx, X, y)
    prog = sr.Program(ctx, nodes, offs, opts, dtype)
    ol, ook = _oracle_each(oracle, nodes, offs, opts, X, y, None, idxs)
    assert list(ook) == expect, "the fixture's near-threshold sums"
    single = _singles(sr, ctx, ds, nodes, offs, opts, dtype, sr.L2DistLoss(), idxs)
    for _ in range(2):
        l, ok = prog.eval_loss_rowsets(ds, sr.L2DistLoss(), idxs)
        assert np.array_equal(ok, ook), np.nonzero(ok != ook)[0]
        assert [(float(l[t]), bool(ok[t])) for t in range(16)] == [single[t] for t in range(16)]
    prog.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_results_do_not_depend_on_the_batch(ctx, oracle, dtype):
    f = _fixture(ctx, oracle, dtype, False)
    sr, opts, nodes, offs, ds, idxs = f["sr"], f["opts"], f["nodes"], f["offs"], f["ds"], f["idxs"]
    # the trees reversed
    rev = list(range(NTREES))[::-1]
    rn = np.concatenate([nodes[offs[t]:offs[t + 1]] for t in rev])
    ro = np.concatenate([[0], np.cumsum([offs[t + 1] - offs[t] for t in rev])]).astype(np.int64)
    p = sr.Program(ctx, rn, ro, opts, dtype)
    l, ok = p.eval_loss_rowsets(ds, sr.L2DistLoss(), [idxs[t] for t in rev])
    p.close()
    assert np.array_equal(_bits(l[::-1]), _bits(f["loss"])) and np.array_equal(ok[::-1], f["ok"])
    # a tree alone with its set
    for t in (0, 2, 12, 13, 15, 40, 95):
        p = _one_tree(sr, ctx, nodes, offs, t, opts, dtype)
        l, ok = p.eval_loss_rowsets(ds, sr.L2DistLoss(), [idxs[t]])
        p.close()
        assert (_b(l[0]), bool(ok[0])) == (_b(f["loss"][t]), bool(f["ok"][t])), t


@pytest.mark.parametrize("ntrees", [300, 4096])
def test_more_trees_than_one_round_of_waves(ctx, oracle, ntrees):
    """300 trees: more than one wave per CU; 4096: more single-wave workgroups than the chip holds at
    once (256 CUs x 11 regions of 14 KB LDS), so late trees start when earlier ones retire."""
    sr = _sr()
    opts = _opts(sr)
    rng = np.random.default_rng(202)
    X = rng.standard_normal((NFEAT, N)).astype(np.float32)
    y = rng.standard_normal(N).astype(np.float32)
    trees = sr.random_population(ntrees, opts, NFEAT, np.float32, 201, 25)
    idxs = [rng.integers(0, N, size=50) for _ in trees]
    nodes, offs = sr.flatten(trees, opts, np.float32)
    ds = sr.DeviceDataset(ctx, X, y)
    prog = sr.Program(ctx, nodes, offs, opts, np.float32)
    l, ok = prog.eval_loss_rowsets(ds, sr.L2DistLoss(), idxs)
    work = ctx.last_work()
    prog.close()
    sample = [int(t) for t in rng.choice(ntrees, size=32, replace=False)]
    single = _singles(sr, ctx, ds, nodes, offs, opts, np.float32, sr.L2DistLoss(), idxs, sample)
    ol, ook = _oracle_each(oracle, nodes, offs, opts, X, y, None, idxs)
    _check(l, ok, single, ol, ook, F32_REL, sample)
    # node-rows over the sets: every launched tree on its 50 rows
    # srhip_last_work: node-rows over the sets (no early exit: evaluated = nominal), 50 rows per launched tree
    total = sum(sr.count_nodes(t) for t in trees)
    assert work["node_rows"] == work["nominal_node_rows"], work
    assert 0.9 * 50 * total <= work["nominal_node_rows"] <= 50 * total, (work, total)
    assert work["tree_rows"] % 50 == 0 and 0.9 * 50 * ntrees <= work["tree_rows"] <= 50 * ntrees, work


@pytest.mark.parametrize("kind_name,args", [("HuberLoss", (0.7,)), ("L1DistLoss", ()), ("LogitMarginLoss", ())])
def test_loss_kinds(ctx, oracle, kind_name, args):
    """Weighted Float64 on 50-row sets against the oracle, at the bound test_gpu_parity.test_loss_kinds
    holds the same loss kinds to (1e-10: the losses' own transcendentals are a few ulp from the oracle's)."""
    sr = _sr()
    loss = getattr(sr, kind_name)(*args)
    opts = _opts(sr)
    rng = np.random.default_rng(302)
    X = rng.standard_normal((4, 1500))
    y = rng.standard_normal(1500)
    w = np.abs(rng.standard_normal(1500))
    trees = sr.random_population(48, opts, 4, np.float64, 301, 12)
    idxs = [rng.integers(0, 1500, size=50) for _ in trees]
    nodes, offs = sr.flatten(trees, opts, np.float64)
    ds = sr.DeviceDataset(ctx, X, y, w)
    prog = sr.Program(ctx, nodes, offs, opts, np.float64)
    l, ok = prog.eval_loss_rowsets(ds, loss, idxs)
    prog.close()
    ol, ook = _oracle_each(oracle, nodes, offs, opts, X, y, w, idxs, loss.kind, loss.p0)
    assert np.array_equal(ok, ook)
    for t in np.nonzero(ook)[0]:
        assert l[t] == ol[t] or abs(l[t] - ol[t]) <= 1e-10 * abs(ol[t]), (t, l[t], ol[t])


def test_validation(ctx, oracle):
    f = _fixture(ctx, oracle, np.float32, False)
    sr, prog, ds = f["sr"], f["prog"], f["ds"]
    lib = sr._lib.load()
    ls = sr.L2DistLoss().c_struct()

    def call(offsets, rows):
        offsets, rows = np.asarray(offsets, dtype=np.int64), np.asarray(rows, dtype=np.int64)
        out, ok = np.empty(NTREES), np.empty(NTREES, dtype=np.uint8)
        sr._lib.check(lib.srhip_eval_loss_rowsets(ctx.handle, ds.handle, prog.handle, ctypes.byref(ls), sr._lib.ptr(offsets),
                                                  sr._lib.ptr(rows), sr._lib.ptr(out), sr._lib.ptr(ok)))
        return out, ok.astype(bool)

    good = np.arange(NTREES + 1) * 2
    rows = np.arange(2 * NTREES) % N
    for offsets, rr, what in ((np.where(np.arange(NTREES + 1) == 7, 11, good), rows, r"row_offsets\[7\] = 11 < row_offsets\[6\] = 12"),
                              (np.where(np.arange(NTREES + 1) == 7, 12, good), rows, r"tree 6 has an empty row set"),
                              (good, np.where(np.arange(2 * NTREES) == 21, N, rows), r"tree 10: .*position 1 of its set.* = 5000"),
                              (good, np.where(np.arange(2 * NTREES) == 0, -1, rows), r"tree 0: .*= -1"),
                              (good + 1, np.arange(2 * NTREES + 1) % N, r"row_offsets\[0\]")):
        with pytest.raises(sr.SrhipError, match=what) as e:
            call(offsets, rr)
        assert e.value.code == sr._lib.ERR_INVALID
    with pytest.raises(sr.SrhipError, match="null"):
        sr._lib.check(lib.srhip_eval_loss_rowsets(ctx.handle, ds.handle, prog.handle, ctypes.byref(ls), None, None, None, None))
    out, ok = call(good, rows)  # a valid call afterwards
    l2, ok2 = prog.eval_loss_rowsets(ds, sr.L2DistLoss(), [rows[2 * t:2 * t + 2] for t in range(NTREES)])
    assert np.array_equal(_bits(out), _bits(l2)) and np.array_equal(ok, ok2) and ok.sum() > NTREES // 2


def test_coalescer_puts_all_subsets_into_one_launch(ctx, oracle):
    f = _fixture(ctx, oracle, np.float32, False)
    sr, opts, nodes, offs, ds = f["sr"], f["opts"], f["nodes"], f["offs"], f["ds"]
    rng = np.random.default_rng(402)
    loss = sr.L2DistLoss()
    idxs = [rng.integers(0, N, size=50) for _ in range(64)]
    single = _singles(sr, ctx, ds, nodes, offs, opts, np.float32, loss, idxs)
    co = sr.Coalescer(ctx, ds, opts, loss, max_batch=64, max_wait_us=2_000_000)
    try:
        tickets = [co.submit(nodes[offs[t]:offs[t + 1]], idxs[t]) for t in range(64)]
        got = [co.wait(k) for k in tickets]
        assert [(_b(g[0]), g[1]) for g in got] == [(_b(single[t][0]), single[t][1]) for t in range(64)]
        assert co.stats()["launches"] == 1, co.stats()
        # 32 requests over the whole dataset and 32 with subsets: two more launches
        tickets = [co.submit(nodes[offs[t]:offs[t + 1]], idxs[t] if t % 2 else None) for t in range(64)]
        got = [co.wait(k) for k in tickets]
        assert co.stats()["launches"] == 3, co.stats()
    finally:
        co.close()
    whole, wok = f["prog"].eval_loss(ds, loss)
    for t in range(64):
        want = single[t] if t % 2 else (float(whole[t]), bool(wok[t]))
        assert (_b(got[t][0]), got[t][1]) == (_b(want[0]), want[1]), t


def test_score_func_batched_batch_equals_the_loop(ctx):
    sr = _sr()
    opts = sr.Options(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"), batching=True, batch_size=50)
    rng = np.random.default_rng(502)
    X = rng.standard_normal((NFEAT, N)).astype(np.float32)
    ds = sr.Dataset(X, (2 * np.cos(X[3]) + X[0] ** 2 - 2).astype(np.float32))
    trees = sr.random_population(40, opts, NFEAT, np.float32, 501, 25)
    ra, rb = np.random.default_rng(7), np.random.default_rng(7)
    scores, losses = sr.score_func_batched_batch(ds, trees, opts, rng=ra)
    loop = [sr.score_func_batched(ds, t, opts, rng=rb) for t in trees]
    assert [float(s) for s in scores] == [float(s) for s, _ in loop]
    assert [float(l) for l in losses] == [float(l) for _, l in loop]
    assert ra.integers(0, 1 << 30) == rb.integers(0, 1 << 30)
    assert np.isfinite(losses).sum() > 30
