"""The persistent launch's last round in equal shares (csrc/srhip_tail_shares.h): the
row blocks past the last whole round of workgroups -- every block of a launch with fewer blocks than
workgroups -- are dealt to the workgroups as shares of their population units.  Whatever the plan, the
results are the grid launch's bit for bit, and every (row block, order slot) entry of the slabs is
written exactly once.

Work counts (srhip_last_work) are compared exactly where they are a function of the inputs: with the
early exit off.  With it on, a failed tree's count depends on which row block reached it first, in
the grid launch as in the persistent one, so only its bounds are checked there."""
import re

import numpy as np
import pytest

import srhip
from srhip import workloads

pytestmark = pytest.mark.gpu

ROWS = (44_100,   # 22 blocks of 2048 rows; the last block's second tile has 68 valid rows
        43_500)   # the last block's second tile is all padding
WGS = ("5", "6", "11", "32")  # 5, 6: leftover blocks; 11: divides 22 blocks (no shares); 32: every block shared
UNITS = ("32", "64", "128")


@pytest.fixture(scope="module")
def pops():
    out = {}
    for rows in ROWS:
        opts, X, y, trees, nodes, offs = workloads.c2(0, 200, rows)
        w = np.random.default_rng(5).uniform(0.5, 2.0, rows).astype(np.float32)
        out[rows] = (opts, X, y, w, nodes, offs)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _eval(prog, ds, loss, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        l, ok = prog.eval_loss(ds, loss)
        return l.copy(), ok.copy(), prog.ctx.last_work()
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _expected_items(prog, ds, loss, env, seed, monkeypatch):
    """The launch plan's item count, read from the lost-item report of a seeded claim counter."""
    with pytest.raises(RuntimeError, match="row-block counter") as e:
        _eval(prog, ds, loss, dict(env, SRHIP_DEBUG_BLOCK_CTR=str(seed)), monkeypatch)
    done, items = map(int, re.search(r"evaluated (\d+) of (\d+) row-block items", str(e.value)).groups())
    assert done == items - seed
    return items


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("kind", ["weighted_l2", "l1"])
def test_every_plan_equals_the_grid_launch_bitwise(pops, monkeypatch, rows, kind):
    opts, X, y, w, nodes, offs = pops[rows]
    ctx = srhip.Context(0)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
    assert prog.stats()["max_stack"] <= 2  # the wide variant: the persistent path
    ds = srhip.DeviceDataset(ctx, X, y, weights=w if kind == "weighted_l2" else None)
    loss = srhip.L2DistLoss() if kind == "weighted_l2" else srhip.L1DistLoss()
    for ee in ({}, {"SRHIP_NO_EARLY_EXIT": "1"}):
        l0, ok0, w0 = _eval(prog, ds, loss, dict(ee, SRHIP_NO_PERSISTENT="1"), monkeypatch)
        assert not ok0.all() and ok0.any()  # failing trees and live ones
        for wgs in WGS:
            for probe in ("0", "1"):
                for units in UNITS:
                    env = dict(ee, SRHIP_PERSISTENT_WGS=wgs, SRHIP_PROBE_BLOCKS=probe, SRHIP_TAIL_SLICES=units)
                    l, ok, wk = _eval(prog, ds, loss, env, monkeypatch)
                    assert np.array_equal(ok, ok0), env
                    assert np.array_equal(_bits(l), _bits(l0)), env
                    assert wk["nominal_node_rows"] == w0["nominal_node_rows"], env
                    if ee:
                        assert wk == w0, (env, wk, w0)
                        assert wk["node_rows"] == wk["nominal_node_rows"]
                    else:
                        assert 0 < wk["node_rows"] < wk["nominal_node_rows"], (env, wk)


def test_plans_take_the_share_path(pops, monkeypatch):
    """The settings above reach what they are meant to reach: the item counts of their plans."""
    opts, X, y, w, nodes, offs = pops[44_100]
    ctx = srhip.Context(0)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
    ds = srhip.DeviceDataset(ctx, X, y)
    loss = srhip.L2DistLoss()
    # (workgroups, probe blocks) -> whole blocks + shares
    for wgs, probe, items in ((5, 0, 20 + 5), (6, 0, 18 + 6), (11, 0, 22), (32, 0, 0 + 32),
                              (5, 1, 20 + 5), (6, 1, 18 + 6), (11, 1, 11 + 11), (32, 1, 0 + 32)):
        env = {"SRHIP_PERSISTENT_WGS": str(wgs), "SRHIP_PROBE_BLOCKS": str(probe)}
        assert _expected_items(prog, ds, loss, env, 2, monkeypatch) == items, env
        env["SRHIP_TAIL_BALANCE"] = "0"
        assert _expected_items(prog, ds, loss, env, 2, monkeypatch) == 22 - probe, env
    env = {"SRHIP_PERSISTENT_WGS": "6", "SRHIP_PROBE_BLOCKS": "0", "SRHIP_TAIL_SHARE_ROUNDS": "2"}
    assert _expected_items(prog, ds, loss, env, 2, monkeypatch) == 18 + 12


def test_default_plan_matches_the_oracle(pops, oracle):
    opts, X, y, w, nodes, offs = pops[44_100]
    ctx = srhip.Context(0)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
    ds = srhip.DeviceDataset(ctx, X, y)
    l0, ok0 = prog.eval_loss(ds, srhip.L2DistLoss())
    ol, _, ook, _ = oracle.eval_loss_batch(nodes, offs, opts.binop_codes, opts.unaop_codes, X, y, None, 0, 0.0)
    assert np.array_equal(ok0, ook)
    live = np.nonzero(ook)[0]
    rel = np.abs(l0[live] - ol[live]) / np.maximum(np.abs(ol[live]), 1e-300)
    assert np.all((l0[live] == ol[live]) | (rel <= 1e-6)), live[rel > 1e-6]


def test_fewer_trees_than_units_on_both_sides_of_the_gate(monkeypatch):
    """37 trees: at S = 64 and 128 most units of a block are empty.  The gate (an average share holds a
    tree per wave: trees x leftover blocks >= 16 x shares) passes with 6 workgroups (4 leftover blocks)
    and fails with 5 (2 leftover blocks: whole blocks, as without balancing)."""
    opts, X, y, trees, nodes, offs = workloads.c2(0, 37, 44_100)
    ctx = srhip.Context(0)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
    ds = srhip.DeviceDataset(ctx, X, y)
    loss = srhip.L2DistLoss()
    base = {"SRHIP_PROBE_BLOCKS": "0"}
    assert _expected_items(prog, ds, loss, dict(base, SRHIP_PERSISTENT_WGS="6"), 1, monkeypatch) == 18 + 6
    assert _expected_items(prog, ds, loss, dict(base, SRHIP_PERSISTENT_WGS="5"), 1, monkeypatch) == 22
    l0, ok0, w0 = _eval(prog, ds, loss, dict(base, SRHIP_NO_PERSISTENT="1", SRHIP_NO_EARLY_EXIT="1"), monkeypatch)
    for wgs in ("5", "6", "32"):
        for units in UNITS:
            for ee in ({}, {"SRHIP_NO_EARLY_EXIT": "1"}):
                env = dict(base, SRHIP_PERSISTENT_WGS=wgs, SRHIP_TAIL_SLICES=units, **ee)
                l, ok, wk = _eval(prog, ds, loss, env, monkeypatch)
                assert np.array_equal(ok, ok0), env
                assert np.array_equal(_bits(l), _bits(l0)), env
                if ee:
                    assert wk == w0, env


def test_no_slab_entry_is_left_stale(pops, monkeypatch):
    """Another population over another dataset fills the context's slabs first: an entry the share
    launch did not write would carry its partials into the sums."""
    opts, X, y, w, nodes, offs = pops[44_100]
    o2, X2, y2, _, n2, f2 = workloads.c2(1, 260, 60_000)
    ctx = srhip.Context(0)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
    other = srhip.Program(ctx, n2, f2, o2, np.float32)
    ds, ds2 = srhip.DeviceDataset(ctx, X, y), srhip.DeviceDataset(ctx, X2, y2)
    loss = srhip.L2DistLoss()
    res = []
    for env in ({"SRHIP_NO_PERSISTENT": "1"}, {"SRHIP_PERSISTENT_WGS": "5"}, {"SRHIP_PERSISTENT_WGS": "6"},
                {"SRHIP_PERSISTENT_WGS": "32", "SRHIP_TAIL_SLICES": "128"}, {}):
        other.eval_loss(ds2, srhip.L1DistLoss())
        res.append((env, _eval(prog, ds, loss, dict(env, SRHIP_PROBE_BLOCKS="0"), monkeypatch)))
    for env, (l, ok, _) in res[1:]:
        assert np.array_equal(ok, res[0][1][1]), env
        assert np.array_equal(_bits(l), _bits(res[0][1][0])), env


@pytest.mark.parametrize("wgs", ["6", None])
def test_three_tickets_in_flight_waited_out_of_order(pops, monkeypatch, wgs):
    if wgs:
        monkeypatch.setenv("SRHIP_PERSISTENT_WGS", wgs)
    ctx = srhip.Context(0)
    jobs = []
    for rows, loss in ((44_100, srhip.L2DistLoss()), (43_500, srhip.L1DistLoss()), (44_100, srhip.L1DistLoss())):
        opts, X, y, w, nodes, offs = pops[rows]
        prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
        jobs.append((prog, srhip.DeviceDataset(ctx, X, y), loss))
    want = [prog.eval_loss(ds, loss) for prog, ds, loss in jobs]
    tickets = [prog.eval_loss_submit(ds, loss) for prog, ds, loss in jobs]
    for i in (2, 0, 1):
        l, ok = tickets[i].wait()
        assert np.array_equal(ok, want[i][1]), i
        assert np.array_equal(_bits(l), _bits(want[i][0])), i


def test_partials_equal_whole_block_claiming_bitwise(pops, monkeypatch):
    opts, X, y, w, nodes, offs = pops[44_100]
    ctx = srhip.Context(0)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
    ds = srhip.DeviceDataset(ctx, X, y)
    loss = srhip.L2DistLoss()
    nt = len(offs) - 1
    # every row of every tree: the partials are a function of the inputs, compared whole.  With the early
    # exit a failed tree's partials depend on which row block reached it first (its loss sum is NaN or
    # not, its statistic Inf or NaN), with or without balancing: there the partials of the trees that
    # succeed, the feature statistics and the finalized results are compared.
    for ee in (True, False):
        if not ee:
            monkeypatch.setenv("SRHIP_NO_EARLY_EXIT", "1")
        monkeypatch.setenv("SRHIP_TAIL_BALANCE", "0")
        s0, c0 = prog.eval_loss_partials(ds, loss)
        monkeypatch.delenv("SRHIP_TAIL_BALANCE")
        l0, ok0, st0 = prog.finalize(X.shape[0], s0, c0)
        assert ok0.any() and not ok0.all()
        keep = np.concatenate([np.repeat(ok0, 2), np.ones(len(s0) - 2 * nt, dtype=bool)]) if ee else np.ones(len(s0), dtype=bool)
        keep_c = ok0 if ee else np.ones(nt, dtype=bool)
        for wgs in ("5", "6", "32", None):
            if wgs:
                monkeypatch.setenv("SRHIP_PERSISTENT_WGS", wgs)
            s, c = prog.eval_loss_partials(ds, loss)
            if wgs:
                monkeypatch.delenv("SRHIP_PERSISTENT_WGS")
            assert np.array_equal(_bits(s)[keep], _bits(s0)[keep]), (ee, wgs)
            assert np.array_equal(_bits(c)[keep_c], _bits(c0)[keep_c]), (ee, wgs)
            l, ok, st = prog.finalize(X.shape[0], s, c)
            assert np.array_equal(ok, ok0) and np.array_equal(st, st0), (ee, wgs)
            assert np.array_equal(_bits(l)[ok0], _bits(l0)[ok0]), (ee, wgs)
        if not ee:
            monkeypatch.delenv("SRHIP_NO_EARLY_EXIT")


def test_lost_item_is_reported_in_both_ranges_then_recovered(pops, monkeypatch):
    """5 workgroups, no probe: items 0..19 are whole blocks, 20..24 shares.  A claim counter seeded
    inside either range skips items; the launch reports it and the next one is clean."""
    opts, X, y, w, nodes, offs = pops[44_100]
    ctx = srhip.Context(0)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
    ds = srhip.DeviceDataset(ctx, X, y)
    loss = srhip.L2DistLoss()
    env = {"SRHIP_PERSISTENT_WGS": "5", "SRHIP_PROBE_BLOCKS": "0"}
    l0, ok0, _ = _eval(prog, ds, loss, env, monkeypatch)
    for seed in (3, 22):
        assert _expected_items(prog, ds, loss, env, seed, monkeypatch) == 25
        l1, ok1, _ = _eval(prog, ds, loss, env, monkeypatch)
        assert np.array_equal(ok1, ok0), seed
        assert np.array_equal(_bits(l1), _bits(l0)), seed
