"""The row-sharded constant gradient of srhip.parallel on CPU (gloo, world_size 2).

Each rank forms its shard's loss, gradient and check partials with the oracle (standing in for the device:
oracle.partials for the sums and the statistic, oracle.loss_grad_devorder for the gradient sums), the ranks
exchange them once (parallel.eval_loss_grad_sharded: one buffer, one exchange), and libsrhip's host-side
srhip_grad_partials_finalize (a host-only program: no device touched) must reproduce the oracle's unsharded loss
and gradient on both ranks identically."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = dict(binary_operators=("+", "-", "*", "/"), unary_operators=("cos",))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _problem(dtype, n=1500, ntrees=48, seed=5):
    import srhip

    opts = srhip.Options(**OPS)
    trees = srhip.random_population(ntrees, opts, 3, dtype, seed=seed, max_size=25)
    nodes, offs = srhip.flatten(trees, opts, dtype)
    rng = np.random.default_rng(seed + 1)
    X = rng.standard_normal((3, n)).astype(dtype)
    y = (np.cos(X[0]) * 2 + X[1] ** 2).astype(dtype)
    w = rng.uniform(0.5, 2.0, n).astype(dtype)
    return opts, nodes, offs, X, y, w


def _shard_partials(oracle, opts, nodes, offs, nconst, X, y, w):
    """(sums, gsums, chk) of one shard: the oracle's mean loss gradient times the shard's weight sum."""
    sums, chk = oracle.partials(nodes, offs, opts.binop_codes, opts.unaop_codes, X, y, w)
    wsum = float(np.sum(w.astype(np.float64)))
    gs = []
    for t in range(len(offs) - 1):
        if nconst[t] == 0:
            continue
        _, g = oracle.loss_grad_devorder(nodes[offs[t]:offs[t + 1]], opts.binop_codes, opts.unaop_codes, X, y, w)
        assert len(g) == nconst[t]
        gs.append(g * wsum)
    return sums, (np.concatenate(gs) if gs else np.zeros(0)), chk


def _rank_main(rank, world, port, dtype_name, q):
    try:
        sys.path[:0] = [os.path.join(ROOT, "symbolicregression.jl_amd"), os.path.join(ROOT, "oracle")]
        import torch.distributed as dist

        import oracle
        import srhip
        from srhip.parallel import eval_loss_grad_sharded

        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        dtype = np.dtype(dtype_name).type
        opts, nodes, offs, X, y, w = _problem(dtype)
        lo, hi = (0, 517) if rank == 0 else (517, X.shape[1])  # uneven shards
        prog = srhip.Program(None, nodes, offs, opts, dtype)
        nconst = prog.num_constants()
        part = lambda: _shard_partials(oracle, opts, nodes, offs, nconst, X[:, lo:hi], y[lo:hi], w[lo:hi])  # noqa: E731
        loss, grads, ok = eval_loss_grad_sharded(prog, X.shape[0], part)
        mine = np.abs(part()[1])
        q.put((rank, loss, ok, np.concatenate([np.zeros(0)] + list(grads)), mine))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # surface the failure to the parent
        q.put((rank, repr(e), None, None, None))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_row_sharded_gradient_gloo_world2(oracle, dtype):
    import multiprocessing as mp

    import srhip

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, np.dtype(dtype).name, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    res.sort(key=lambda r: r[0])
    for r in res:
        assert r[2] is not None, r[1]
    opts, nodes, offs, X, y, w = _problem(dtype)
    nconst = srhip.Program(None, nodes, offs, opts, dtype).num_constants()
    coff = np.concatenate([[0], np.cumsum(nconst)])
    ol, _, ook, _ = oracle.eval_loss_batch(nodes, offs, opts.binop_codes, opts.unaop_codes, X, y, w, 0, 0.0)
    wsum = float(np.sum(w.astype(np.float64)))
    # the tolerance's scale: what the shards contributed to each component, in the gradient's units
    contrib = (res[0][4] + res[1][4]) / wsum
    checked = 0
    for _, loss, ok, grad, _ in res:
        assert np.array_equal(ok, ook)
        np.testing.assert_allclose(loss[ook], ol[ook], rtol=1e-12)
        assert np.all(np.isinf(loss[~ook]))
        for t in range(len(nconst)):
            g = grad[coff[t]:coff[t + 1]]
            if not ook[t]:
                assert not np.any(g), t  # a failing tree: a zero slice
                continue
            if nconst[t] == 0:
                continue
            _, og = oracle.loss_grad_devorder(nodes[offs[t]:offs[t + 1]], opts.binop_codes, opts.unaop_codes, X, y, w)
            for k in range(nconst[t]):
                if not np.isfinite(og[k]):
                    continue
                tol = 1e-12 * max(1.0, contrib[coff[t] + k])
                assert abs(g[k] - og[k]) <= tol, (t, k, g[k], og[k], tol)
                checked += 1
    assert checked >= 2 * 40
    # identical on every rank, bit for bit
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    assert np.array_equal(res[0][3].view(np.uint64), res[1][3].view(np.uint64))
