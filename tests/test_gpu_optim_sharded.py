"""Row-sharded constant gradients and constant optimisation (srhip_eval_loss_grad_sharded,
srhip_optimize_constants_sharded and the manual steps srhip_eval_loss_grad_partials /
srhip_grad_partials_finalize) on one MI355X: at world size 1 through the library's RCCL communicator, bit for
bit against the one-device calls; with more than one shard through the manual steps, whose combination is
done here (RCCL cannot place two ranks on one device)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPS = dict(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))


def _sr():
    import srhip

    return srhip


@pytest.fixture(scope="module")
def comm(ctx):
    from srhip import parallel

    c = parallel.NativeComm(ctx, 1, 0, parallel.NativeComm.unique_id())
    yield c
    c.close()


def _population(dtype):
    """The population of test_native_sharded_eval_world1_equals_eval_loss (200 random trees over + - * /, cos,
    exp, 3 features) and five more: 11 constants (several chunks at 8 and at 4 tangents), one constant, none,
    one that fails on its statistic (exp(exp(x1)) * huge) and one that is undecided on it and goes through the
    precise pass (x1 * huge; its sum overflows there)."""
    sr = _sr()
    opts = sr.Options(**OPS)
    trees = sr.random_population(200, opts, 3, dtype, seed=5, max_size=30)
    x1, x2, x3 = sr.Node("x1"), sr.Node("x2"), sr.Node("x3")
    f32 = dtype == np.float32
    terms = [lambda: sr.Node("x2"), lambda: sr.Node("x3"), lambda: sr.cos(sr.Node("x2"))]
    many = sr.Node(val=0.25)
    for k in range(10):
        many = many + sr.Node(val=0.5 + 0.125 * k) * terms[k % 3]()
    extra = [many, x2 * sr.Node(val=1.5), x2 * x3 - x2,
             sr.exp(sr.exp(x1)) * sr.Node(val=1e30 if f32 else 1e300), x1 * sr.Node(val=3e37 if f32 else 1e306)]
    trees = trees + extra
    nodes, offs = sr.flatten(trees, opts, dtype)
    return opts, trees, nodes, offs


def _data(dtype, n, seed=6):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((3, n)).astype(dtype)
    X[0, :] = np.abs(X[0, :]) + 1.0
    y = (np.cos(X[1]) * 2 + X[2] ** 2).astype(dtype)
    w = rng.uniform(0.5, 2.0, n).astype(dtype)
    return X, y, w


def _same(a, b):
    """loss / gradient / ok triples equal bit for bit (NaN equals NaN)."""
    la, ga, oa = a
    lb, gb, ob = b
    return (np.array_equal(oa, ob) and np.array_equal(la.view(np.uint64), lb.view(np.uint64)) and
            all(np.array_equal(x.view(np.uint64), z.view(np.uint64)) for x, z in zip(ga, gb)))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_world1_gradient_equals_eval_loss_grad(ctx, comm, monkeypatch, dtype, weighted):
    sr = _sr()
    opts, trees, nodes, offs = _population(dtype)
    X, y, w = _data(dtype, 300_000)
    prog = sr.Program(ctx, nodes, offs, opts, dtype)
    nconst = prog.num_constants()
    assert list(nconst[-5:]) == [11, 1, 0, 1, 1]
    ds = sr.DeviceDataset(ctx, X, y, w if weighted else None)
    loss = sr.L2DistLoss()
    idx = np.random.default_rng(7).integers(0, X.shape[1], size=5000)
    # both tangent widths forced (left alone, the cost heuristic gives this population 4): at 8 the 11-constant
    # tree is the chunks 8 + 3, at 4 it is 4 + 4 + 3
    for kt in ("8", "4"):
        monkeypatch.setenv("SRHIP_GRAD_KT", kt)
        for rows in (None, idx):
            want = prog.eval_loss_grad(ds, loss, idx=rows)
            calls0 = comm.stats()[2]
            got = comm.eval_loss_grad_sharded(prog, ds, loss, idx=rows)
            # the call-start exchange, the round's, and the precise pass's SUM for the undecided tree
            assert comm.stats()[2] >= calls0 + 2, (kt, comm.stats()[2] - calls0)
            assert np.array_equal(got[2], want[2])
            assert np.array_equal(got[0], want[0], equal_nan=True)
            for t in range(len(nconst)):
                assert np.array_equal(got[1][t], want[1][t], equal_nan=True), (kt, t)
            assert _same(got, want)
            if rows is None:
                assert not want[2][-2] and want[0][-2] == np.inf  # exp(exp(x1)) * huge fails
                assert want[2][-3] and want[2][-4] and want[2][-5]
                # (x1 * huge is undecided on its statistic; the precise pass fails it: the sum overflows)
                assert not want[2][-1] and want[0][-1] == np.inf
    prog.close()


@pytest.mark.parametrize("kt", [None, "8", "4"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_world1_optimiser_equals_unsplit_optimize_constants(ctx, comm, monkeypatch, dtype, kt):
    """kt: the gradient passes' tangent width left to the cost heuristic (4 for the first launches of this
    population, then whatever the active trees give), or forced to 8 / 4 for every round of both optimisers."""
    sr = _sr()
    if kt:
        monkeypatch.setenv("SRHIP_GRAD_KT", kt)
    opts = sr.Options(**OPS)
    cand = sr.random_population(200, opts, 3, dtype, seed=31, max_size=20)
    cn, co = sr.flatten(cand, opts, dtype)
    nc = sr.Program(None, cn, co, opts, dtype).num_constants()
    trees = [t for t, k in zip(cand, nc) if k > 0][:64]
    assert len(trees) == 64
    nodes, offs = sr.flatten(trees, opts, dtype)
    X, y, _ = _data(dtype, 20_000, seed=32)
    ds = sr.DeviceDataset(ctx, X, y)
    loss = sr.L2DistLoss()
    a = sr.Program(ctx, nodes, offs, opts, dtype)
    b = sr.Program(ctx, nodes, offs, opts, dtype)
    calls0 = comm.stats()[2]
    la, ia, fa, sa = comm.optimize_constants_sharded(a, ds, loss, iterations=8, nrestarts=2, seed=9, return_starts=True)
    # the call-start exchange, the baseline's and the re-score's groups, and one exchange per optimiser round
    # (each start of a tree takes at least one evaluation)
    assert comm.stats()[2] >= calls0 + 3 + 3
    monkeypatch.setenv("SRHIP_OPTIM_SPLIT", "1")
    lb, ib, fb, sb = b.optimize_constants(ds, loss, iterations=8, nrestarts=2, seed=9, return_starts=True)
    assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64))
    assert np.array_equal(ia, ib) and np.array_equal(fa, fb)
    assert np.array_equal(la.view(np.uint64), lb.view(np.uint64))
    ca, cb = np.concatenate(a.get_constants()), np.concatenate(b.get_constants())
    assert np.array_equal(ca.view(np.uint64), cb.view(np.uint64))
    assert ia.sum() >= 16  # the optimiser did move constants
    # caller-supplied starts travel the same way
    a2 = sr.Program(ctx, nodes, offs, opts, dtype)
    b2 = sr.Program(ctx, nodes, offs, opts, dtype)
    la2, ia2, fa2 = comm.optimize_constants_sharded(a2, ds, loss, iterations=4, nrestarts=2, seed=1, starts=sa)
    lb2, ib2, fb2 = b2.optimize_constants(ds, loss, iterations=4, nrestarts=2, seed=1, starts=sa)
    assert np.array_equal(la2.view(np.uint64), lb2.view(np.uint64)) and np.array_equal(ia2, ib2) and np.array_equal(fa2, fb2)
    for p in (a, b, a2, b2):
        p.close()


def test_sharded_calls_refuse_int32_and_a_migration_in_flight(ctx, comm):
    sr = _sr()
    from srhip import _lib

    opts = sr.Options(binary_operators=("+", "*"), unary_operators=())
    tree = sr.Node("x1") * sr.Node(val=2) + sr.Node(val=1)
    Xi = np.arange(12, dtype=np.int32).reshape(2, 6)
    nodes, offs = sr.flatten([tree], opts, np.int32)
    prog = sr.Program(ctx, nodes, offs, opts, np.int32)
    ds = sr.DeviceDataset(ctx, Xi, Xi[0].copy())
    for call in (lambda: comm.eval_loss_grad_sharded(prog, ds, sr.L2DistLoss()),
                 lambda: comm.optimize_constants_sharded(prog, ds, sr.L2DistLoss())):
        with pytest.raises(_lib.SrhipError) as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED
    nodes, offs = sr.flatten([tree], opts, np.float32)
    fprog = sr.Program(ctx, nodes, offs, opts, np.float32)
    Xf = Xi.astype(np.float32)
    fds = sr.DeviceDataset(ctx, Xf, Xf[0].copy())
    pend = comm.migrate_start(nodes, offs, np.zeros(1), 1, 8)
    for call in (lambda: comm.eval_loss_grad_sharded(fprog, fds, sr.L2DistLoss()),
                 lambda: comm.optimize_constants_sharded(fprog, fds, sr.L2DistLoss())):
        with pytest.raises(_lib.SrhipError) as e:
            call()
        assert e.value.code == _lib.ERR_INVALID and "migration" in str(e.value)
    pend.wait()
    l, g, ok = comm.eval_loss_grad_sharded(fprog, fds, sr.L2DistLoss())  # and it works once the migration is collected
    want = fprog.eval_loss_grad(fds, sr.L2DistLoss())
    assert _same((l, g, ok), want)


# ---- more than one shard on one GPU: the manual steps ------------------------------------------------------
def _combine(prog, parts):
    """Partials of several shards combined as an all-reduce would: sums and gsums by +, chk by the dtype's op."""
    sums = sum(p[0] for p in parts)
    gsums = sum(p[1] for p in parts)
    chks = [p[2] for p in parts]
    chk = np.maximum.reduce(chks) if prog.chk_reduce_op() == "max" else sum(chks)
    return sums, gsums, chk


def _manual(ctx, prog, loss, X, y, w, bounds):
    """eval_loss_grad_partials per shard (its own dataset), combination, finalize_grad."""
    sr = _sr()
    shards = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        shards.append(sr.DeviceDataset(ctx, np.ascontiguousarray(X[:, lo:hi]), y[lo:hi], None if w is None else w[lo:hi]))
    parts = [prog.eval_loss_grad_partials(ds, loss) for ds in shards]
    sums, gsums, chk = _combine(prog, parts)
    return shards, sums, prog.finalize_grad(X.shape[0], sums, gsums, chk)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_shards_exact_arithmetic(ctx, comm, monkeypatch, dtype):
    """Inputs on which every summation order gives the same bits (small integers throughout), so loss and gradient
    must EQUAL the exact integer sums over the weight sum -- unsharded, and on 2 and on 3 shards through the manual
    steps.  Shard sizes 1 (shorter than a 256-row block), 16 639 (65 blocks, the last partial: the reduction's
    lanes wrap) and 133 360 (521 blocks: the reduction's second batch of 512).  The manual steps reduce each
    shard with grad_reduce_kernel (the records go to host memory); so that the same three shapes reach
    grad_reduce_shard_kernel too, each shard is also a dataset of its own under the world-1 sharded call, at
    both tangent widths, against the exact sums over its own rows."""
    sr = _sr()
    n = 150_000
    rng = np.random.default_rng(40)
    Xi = rng.integers(-2, 3, size=(3, n)).astype(np.int64)
    wi = rng.integers(1, 4, size=n).astype(np.int64)
    yi = rng.integers(-5, 6, size=n).astype(np.int64)
    x1, x2, x3 = Xi
    opts = sr.Options(binary_operators=("+", "-", "*"), unary_operators=())
    N, C = sr.Node, lambda v: sr.Node(val=float(v))  # noqa: E731
    trees = [
        C(2) * N("x1") + C(-1),
        C(1) * N("x1") * N("x2") + C(-2) * N("x3") - C(2),
        (N("x1") + C(1)) * (N("x2") - C(-2)),
        N("x1") * N("x2") - N("x3"),          # no constants
        N("x2") * sr.Node(val=np.inf),        # fails on every row: 0 * Inf is NaN, the others +-Inf
    ]
    # exact predictions and d pred / d constant (get_constants order), in int64
    pred = [2 * x1 - 1, x1 * x2 - 2 * x3 - 2, (x1 + 1) * (x2 + 2), x1 * x2 - x3]
    dpred = [[x1, np.ones_like(x1)], [x1 * x2, x3, -np.ones_like(x1)], [x2 + 2, -(x1 + 1)], []]
    per_row = []
    for p, ds_ in zip(pred, dpred):
        r = p - yi
        assert np.abs(r).max() <= 30
        rows = [wi * r * r] + [2 * wi * r * d for d in ds_]
        for v in rows:
            # every per-row value, and so every 256-row partial, below 2^24; every total below 2^53: a condition on
            # the inputs (Float32 products and per-lane sums are then exact), not a tolerance
            assert 256 * int(np.abs(v).max()) < 2 ** 24 and int(np.abs(v).sum()) < 2 ** 53
        per_row.append(rows)

    def exact(lo, hi):
        W = np.float64(int(wi[lo:hi].sum()))
        return ([np.float64(int(rows[0][lo:hi].sum())) / W for rows in per_row],
                [np.array([np.float64(int(v[lo:hi].sum())) / W for v in rows[1:]]) for rows in per_row])

    nodes, offs = sr.flatten(trees, opts, dtype)
    prog = sr.Program(ctx, nodes, offs, opts, dtype)
    assert list(prog.num_constants()) == [2, 3, 2, 0, 1]
    X, y, w = Xi.astype(dtype), yi.astype(dtype), wi.astype(dtype)
    loss = sr.L2DistLoss()

    def check(l, g, ok, want, zero_slice):
        assert list(ok) == [True, True, True, True, False]
        for t in range(4):
            assert l[t] == want[0][t], (t, l[t], want[0][t])
            assert np.array_equal(g[t], want[1][t]), (t, g[t], want[1][t])
        assert l[4] == np.inf
        if zero_slice:
            assert np.array_equal(g[4], [0.0])

    full = sr.DeviceDataset(ctx, X, y, w)
    check(*prog.eval_loss_grad(full, loss), exact(0, n), zero_slice=False)
    for bounds in ([0, 16_640, n], [0, 1, 16_640, n]):
        shards, sums, (l, g, ok, status) = _manual(ctx, prog, loss, X, y, w, bounds)
        assert not np.any(status == 2)
        assert sums[1] == wi.sum() and sums[-1] == n
        check(l, g, ok, exact(0, n), zero_slice=True)
    # the same three shapes through grad_reduce_shard_kernel: each shard alone under the world-1 sharded call
    for kt in ("8", "4"):
        monkeypatch.setenv("SRHIP_GRAD_KT", kt)
        for ds, lo, hi in zip(shards, bounds[:-1], bounds[1:]):
            got = comm.eval_loss_grad_sharded(prog, ds, loss)
            check(*got, exact(lo, hi), zero_slice=False)
            assert _same(got, prog.eval_loss_grad(ds, loss))
    prog.close()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_shards_general_arithmetic(ctx, oracle, dtype, weighted):
    """The world-1 population on two uneven shards of 40 000 rows (51 and 106 row blocks: the shard boundary is a
    block boundary, so both paths sum the same 157 block partials and differ in the order alone).  ok equals the
    unsharded call's; losses agree to nrb * 2^-53 relative (the reassociation of a sum of nrb non-negative f64
    partials); gradients agree with the oracle's exact gradient in the device's row order to the tolerance
    tests/test_gpu_optim.py holds the device to against the oracle (1e-6 Float32, 1e-12 Float64, relative);
    trees left undecided are settled through eval_precise_partials / precise_finalize."""
    sr = _sr()
    opts, trees, nodes, offs = _population(dtype)
    n, cut = 40_000, 51 * 256
    X, y, w = _data(dtype, n)
    w = w if weighted else None
    prog = sr.Program(ctx, nodes, offs, opts, dtype)
    nconst = prog.num_constants()
    loss = sr.L2DistLoss()
    full = sr.DeviceDataset(ctx, X, y, w)
    ul, ug, uok = prog.eval_loss_grad(full, loss)
    shards, sums, (l, g, ok, status) = _manual(ctx, prog, loss, X, y, w, [0, cut, n])
    und = np.nonzero(status == 2)[0].astype(np.int32)
    assert len(nconst) - 1 in und  # x1 * huge
    opsums = sum(prog.eval_precise_partials(ds, und) for ds in shards)
    for t, good in zip(und, prog.precise_finalize(und, opsums)):
        if not good:
            ok[t], l[t] = False, np.inf
            g[t][:] = 0.0
    assert np.array_equal(ok, uok)
    nrb = -(-n // 256)
    tol = 1e-6 if dtype == np.float32 else 1e-12
    worst_l = worst_g = 0.0
    checked = 0
    for t in range(len(nconst)):
        if not ok[t]:
            assert l[t] == np.inf and not np.any(g[t])
            continue
        if l[t] != ul[t]:
            assert np.isfinite(l[t]) and np.isfinite(ul[t]), (t, l[t], ul[t])
            rel = abs(l[t] - ul[t]) / max(abs(l[t]), abs(ul[t]))
            worst_l = max(worst_l, rel)
            assert rel <= nrb * 2.0 ** -53, (t, l[t], ul[t], rel)
        if nconst[t] == 0 or not np.isfinite(l[t]):
            continue
        _, og = oracle.loss_grad_devorder(nodes[offs[t]:offs[t + 1]], opts.binop_codes, opts.unaop_codes, X, y, w)
        for k in range(nconst[t]):
            a, b = g[t][k], og[k]
            if a == b or not np.isfinite(b):
                continue
            rel = abs(a - b) / max(abs(a), abs(b)) if np.isfinite(a) else np.inf
            worst_g = max(worst_g, rel)
            assert abs(a - b) <= tol * max(abs(a), abs(b)) + 1e-300, (t, k, a, b, ug[t][k], rel)
        checked += 1
    print(f"sharded vs unsharded: worst loss difference {worst_l:.3e} (bound {nrb * 2.0 ** -53:.3e}); "
          f"worst gradient difference to the oracle {worst_g:.3e} (bound {tol:.0e}); {checked} trees")
    assert checked >= 100
    prog.close()
