"""The device-free steps of the row-sharded constant gradient (no GPU): srhip_grad_partials_finalize on
hand-made partials of a host-only program, and srhip_shard_signature_check on hand-made signatures."""
import ctypes

import numpy as np
import pytest


def _prog(dtype):
    """x1 * 2 + 0.5 (two constants), cos(x2) (none), x1 * 3 (one), over 2 features; host-only."""
    import srhip as sr

    opts = sr.Options(binary_operators=("+", "*"), unary_operators=("cos",))
    x1, x2 = sr.Node("x1"), sr.Node("x2")
    trees = [x1 * sr.Node(val=2.0) + sr.Node(val=0.5), sr.cos(x2), x1 * sr.Node(val=3.0)]
    nodes, offs = sr.flatten(trees, opts, dtype)
    return sr.Program(None, nodes, offs, opts, dtype)


def _partials(nt, nfeat, rows, wsum, loss_sums):
    sums = np.zeros(2 * nt + 2 * nfeat + 1)
    sums[0:2 * nt:2] = loss_sums
    sums[1:2 * nt:2] = wsum
    sums[2 * nt:2 * nt + 2 * nfeat:2] = 1.0  # finite column sums, no non-finite entries
    sums[-1] = rows
    return sums


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_finalize_divides_by_the_weight_sum_and_fails_on_a_bad_statistic(dtype):
    prog = _prog(dtype)
    assert list(prog.num_constants()) == [2, 0, 1]
    sums = _partials(3, 2, rows=1000, wsum=250.0, loss_sums=[500.0, 125.0, 750.0])
    gsums = np.array([50.0, -25.0, 1000.0])
    chk = np.array([1.0, 1.0, np.inf])  # tree 2: a non-finite operator output on some shard
    loss, grads, ok, status = prog.finalize_grad(2, sums, gsums, chk)
    assert list(ok) == [True, True, False] and list(status) == [0, 0, 1]
    assert loss[0] == 2.0 and loss[1] == 0.5 and loss[2] == np.inf
    assert np.array_equal(grads[0], [0.2, -0.1]) and grads[1].size == 0
    assert np.array_equal(grads[2], [0.0])  # a failing tree: +Inf and a zero slice
    # NaN fails like +Inf
    loss, grads, ok, status = prog.finalize_grad(2, sums, gsums, np.array([np.nan, 1.0, 1.0]))
    assert list(ok) == [False, True, True] and loss[0] == np.inf and np.array_equal(grads[0], [0.0, 0.0])
    assert loss[2] == 3.0 and np.array_equal(grads[2], [4.0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_finalize_takes_the_decisions_of_partials_finalize_around_the_threshold(dtype):
    """Statistics from far below to far above the undecided threshold (Float32: rows * max |v| against 2^128;
    Float64: sum |v| 2^-512 against 2^1024), and the thresholds' neighbours: status and ok are those of
    srhip_partials_finalize on the same sums and chk; an undecided tree reports its quotients with ok = 1."""
    prog = _prog(dtype)
    rows = 4096.0
    sums = _partials(3, 2, rows=rows, wsum=rows, loss_sums=[4096.0, 8192.0, 2048.0])
    gsums = np.array([4096.0, 2048.0, -4096.0])
    if dtype == np.float32:
        edge = 2.0 ** 128 / (2.0 * rows)
    else:
        edge = 2.0 ** 511  # chk * 2^512 * 2 reaches 2^1024
    seen = set()
    for c in (1.0, edge * 2.0 ** -20, np.nextafter(edge, 0.0) * 0.5, edge * (1 - 2.0 ** -20), edge, edge * 1.5, edge * 2.0 ** 20,
              np.inf):
        chk = np.array([c, c, c])
        l0, ok0, st0 = prog.finalize(2, sums, chk)
        loss, grads, ok, status = prog.finalize_grad(2, sums, gsums, chk)
        assert np.array_equal(status, st0), (c, status, st0)
        assert np.array_equal(ok, st0 != 1)
        for t in range(3):
            if st0[t] == 1:
                assert loss[t] == np.inf and not np.any(grads[t])
            else:
                assert loss[t] == sums[2 * t] / rows
        if st0[0] != 1:
            assert np.array_equal(grads[0], [1.0, 0.5]) and np.array_equal(grads[2], [-1.0])
        seen.update(int(s) for s in st0)
    assert seen == {0, 1, 2}


def test_finalize_argument_errors():
    import srhip as sr
    from srhip import _lib

    lib = _lib.load()
    prog = _prog(np.float32)
    sums = _partials(3, 2, rows=10, wsum=10.0, loss_sums=[1.0, 1.0, 1.0])
    gsums, chk = np.zeros(3), np.zeros(3)
    loss, grad, ok, st = np.zeros(3), np.zeros(3), np.zeros(3, np.uint8), np.zeros(3, np.uint8)
    p = _lib.ptr
    good = (prog.handle, 2, p(sums), p(gsums), p(chk), p(loss), p(grad), p(ok), p(st))
    assert lib.srhip_grad_partials_finalize(*good) == 0
    assert lib.srhip_grad_partials_finalize(*good[:8], None) == 0  # the status is optional
    for i in (0, 2, 3, 4, 5, 6, 7):
        bad = list(good)
        bad[i] = None
        assert lib.srhip_grad_partials_finalize(*bad) == _lib.ERR_INVALID, i
    assert lib.srhip_grad_partials_finalize(prog.handle, -1, *good[2:]) == _lib.ERR_INVALID
    # tree 1 reads feature 2: a dataset of one feature cannot hold its column check
    assert lib.srhip_grad_partials_finalize(prog.handle, 1, *good[2:]) == _lib.ERR_INVALID
    assert b"feature" in lib.srhip_last_error()
    with pytest.raises(ValueError):
        prog.finalize_grad(2, sums[:-1], gsums, chk)
    # Int32 programs have no constant gradients
    opts = sr.Options(binary_operators=("+", "*"), unary_operators=())
    nodes, offs = sr.flatten([sr.Node("x1") * sr.Node(val=2)], opts, np.int32)
    iprog = sr.Program(None, nodes, offs, opts, np.int32)
    s1 = _partials(1, 1, rows=10, wsum=10.0, loss_sums=[1.0])
    one = np.zeros(1)
    assert lib.srhip_grad_partials_finalize(iprog.handle, 1, p(s1), p(one), p(one), p(loss), p(grad), p(ok),
                                            p(st)) == _lib.ERR_UNSUPPORTED


def _signature(lib, **fields):
    """One rank's signature: [k_i, -k_i] per field, every field 0 but the named ones."""
    n = lib.srhip_shard_signature_fields()
    names = [lib.srhip_shard_signature_field_name(i).decode() for i in range(n)]
    k = np.zeros(n)
    for name, v in fields.items():
        k[names.index(name)] = v
    out = np.empty(2 * n)
    out[0::2], out[1::2] = k, -k
    return out, names


def test_signature_check_names_the_first_disagreeing_field():
    from srhip import _lib

    lib = _lib.load()
    n = lib.srhip_shard_signature_fields()
    base = dict(trees=64, dtype=1, iterations=8, restarts=2)
    a, names = _signature(lib, **base)
    assert n >= 16 and len(set(names)) == n
    for want in ("trees", "total constants", "dtype", "loss kind", "iterations", "restarts", "SRHIP_GRAD_KT"):
        assert want in names
    assert lib.srhip_shard_signature_field_name(n) is None and lib.srhip_shard_signature_field_name(-1) is None
    b, _ = _signature(lib, **base)
    assert lib.srhip_shard_signature_check(_lib.ptr(np.maximum(a, b)), n) == -1
    # each single field disagreeing is named, whichever rank holds the larger value
    for i, name in enumerate(names):
        for delta in (1.0, -1.0, 2.0 ** 31):
            other = dict(base)
            other[name] = other.get(name, 0.0) + delta
            c, _ = _signature(lib, **other)
            red = np.maximum(a, c)
            assert lib.srhip_shard_signature_check(_lib.ptr(red), n) == i, (name, delta)
            assert lib.srhip_shard_signature_check(_lib.ptr(np.maximum(c, a)), n) == i
    # two fields: the first one; three ranks; a NaN disagrees; argument errors
    c, _ = _signature(lib, **dict(base, trees=65, restarts=3))
    assert names[lib.srhip_shard_signature_check(_lib.ptr(np.maximum(a, c)), n)] == "trees"
    assert lib.srhip_shard_signature_check(_lib.ptr(np.maximum(np.maximum(a, b), c)), n) == names.index("trees")
    d = a.copy()
    d[2 * 3] = np.nan
    assert lib.srhip_shard_signature_check(_lib.ptr(d), n) == 3
    assert lib.srhip_shard_signature_check(_lib.ptr(a), 0) == -1
    assert lib.srhip_shard_signature_check(None, n) == -2
    assert lib.srhip_shard_signature_check(_lib.ptr(a), -1) == -2
    assert isinstance(lib.srhip_shard_signature_check(_lib.ptr(a), ctypes.c_int32(n)), int)
