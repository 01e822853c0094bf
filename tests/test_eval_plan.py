"""The launch decision of a population evaluation (csrc/srhip_plan.cpp plan_eval, through
srhip_plan_eval; no device): which launch, kernel variant, row blocks, LDS bytes, probe, last-round
shares and kernel form a shape gets.  The expected values are worked out from the rules in the code
comments and DESIGN.md 3.1 (16 rows per lane x 64 lanes = 1024-row tiles, 2048-row blocks, LDS bytes =
staged columns x block rows x 4 + 16, a probe of 4 blocks from 64 blocks on, the leftover blocks past
the last whole round dealt as 256 shares when the average share holds 16 trees), not read off the
code."""
import ctypes

import pytest

import srhip._lib as L

SWITCHES = ("NO_PERSISTENT", "PRB_ROWS", "PROBE_BLOCKS", "SMALL_POP", "DERIVE_ALWAYS", "NO_FUSED_REDUCE",
            "PERSISTENT_WGS", "TAIL_BALANCE", "TAIL_SLICES", "TAIL_SHARE_ROUNDS", "NO_HOT_FORM", "PROBE_TREE_CLAIMS",
            "RB_ROWS", "NO_WIDE", "DEBUG_STOP", "TRACE")
SMALL, PERSISTENT, GRID = 0, 1, 2
WIDE_MIN_ROWS = 4096


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv("SRHIP_" + s, raising=False)


def plan(**kw):
    q = dict(dtype=L.F32, mode=0, nlive=1024, m=1_000_000, maxfeat=5, nd=0, kmax=2, dkmax=0, wide_ops=0, weighted=0,
             sharded=0, have_recs=1, loss_kind=0, num_cu=256, lds_max=163840)
    q.update(kw)
    out = L.PlanInfo()
    assert L.load().srhip_plan_eval(ctypes.byref(L.PlanQuery(**q)), ctypes.byref(out)) == 0
    return {n: getattr(out, n) for n, _ in L.PlanInfo._fields_ if n != "pad"}


def expect(p, **kw):
    got = {k: p[k] for k in kw}
    assert got == kw


A = dict(kind=PERSISTENT, R=16, K=2, rb_rows=2048, nrb=489, lds=49168, use_d=0, probe_blocks=4, wgs=256,
         tail_slices=128, tail_blocks=229, tail_shares=256, expect_items=512, nch=977, cpb=2, fused=0, hot=1)


def test_persistent_cases():
    expect(plan(), **A)                                                     # A
    expect(plan(nd=10, dkmax=2), **{**A, "use_d": 1, "lds": 131088})        # B
    expect(plan(nd=14, dkmax=2), **A)                                       # C: the derived columns do not fit
    assert plan(nd=10, dkmax=4)["kind"] != PERSISTENT                       # D
    expect(plan(weighted=1), **{**A, "lds": 57360})                         # E
    expect(plan(m=100_000), kind=PERSISTENT, nrb=49, probe_blocks=0, wgs=256, tail_blocks=49, tail_shares=256,
           expect_items=256, nch=98)                                        # F
    expect(plan(nlive=32, m=8192), kind=PERSISTENT, nrb=4, probe_blocks=0, wgs=4, tail_slices=1, tail_blocks=0,
           tail_shares=0, expect_items=4, hot=1)                            # G
    assert plan(dtype=L.F64)["kind"] != PERSISTENT                          # L
    expect(plan(have_recs=0), **{**A, "hot": 0})                            # Q
    assert plan(sharded=1)["fused"] == 0                                    # R


def test_grid_and_small_cases():
    H = dict(kind=GRID, R=8, K=2, rb_rows=2048, nrb=1, xlds=1, lds=49168, groups=2, tpg=16, fused=1, hot=0)
    expect(plan(nlive=32, m=2048), **H)                                     # H
    expect(plan(nlive=32, m=2048, sharded=1), **{**H, "fused": 0})          # R
    expect(plan(nlive=2, m=10_000_000), kind=SMALL, R=16, K=2, rb_rows=1024, nrb=9766, groups=1, tpg=2, xlds=0,
           lds=16, wg_waves=2, hot=0)                                       # I
    expect(plan(nlive=16, m=262_143), kind=PERSISTENT, nrb=128, probe_blocks=4, wgs=124, tail_blocks=0,
           expect_items=124)                                                # J: one row short of a small launch
    assert plan(nlive=17, m=262_144)["kind"] != SMALL                       # K: one tree too many
    assert plan(nlive=16, m=262_144)["kind"] == SMALL


def test_switches(monkeypatch):
    monkeypatch.setenv("SRHIP_NO_PERSISTENT", "1")                          # M
    assert plan()["kind"] == GRID
    monkeypatch.delenv("SRHIP_NO_PERSISTENT")
    monkeypatch.setenv("SRHIP_PROBE_BLOCKS", "0")                           # N
    expect(plan(), **{**A, "probe_blocks": 0, "tail_blocks": 233, "expect_items": 512})
    monkeypatch.delenv("SRHIP_PROBE_BLOCKS")
    monkeypatch.setenv("SRHIP_PRB_ROWS", "1024")                            # O
    expect(plan(), kind=PERSISTENT, rb_rows=1024, nrb=977, cpb=1, lds=24592, probe_blocks=4, tail_blocks=205,
           expect_items=1024)
    monkeypatch.delenv("SRHIP_PRB_ROWS")
    monkeypatch.setenv("SRHIP_NO_HOT_FORM", "1")                            # P
    expect(plan(), **{**A, "hot": 0})
    monkeypatch.delenv("SRHIP_NO_HOT_FORM")
    expect(plan(), **A)


GRID_NLIVE, GRID_ND, GRID_M = (17, 100, 1024), (0, 3, 10, 14), (4096, 8192, 100_000, 1_000_000)


def test_preplan_matches_the_launch():
    """The order planned at program creation assumes WIDE_MIN_ROWS unweighted rows: wherever that plan is
    persistent, the launch over the real rows is persistent with the same order key."""
    for nlive in GRID_NLIVE:
        for nd in GRID_ND:
            pre = plan(nlive=nlive, nd=nd, dkmax=2, m=WIDE_MIN_ROWS)
            assert pre["kind"] == PERSISTENT
            for m in GRID_M:
                p = plan(nlive=nlive, nd=nd, dkmax=2, m=m)
                assert p["kind"] == PERSISTENT, (nlive, nd, m)
                assert [p[k] for k in ("groups", "tpg", "use_d")] == [pre[k] for k in ("groups", "tpg", "use_d")]


def test_plans_stay_inside_the_lds_budget():
    n = 0
    for dtype in (L.F32, L.F64):
        for weighted in (0, 1):
            for nlive in GRID_NLIVE + (2,):
                for nd in GRID_ND:
                    for m in GRID_M + (2048, 10_000_000):
                        for kmax in (2, 4):
                            p = plan(dtype=dtype, weighted=weighted, nlive=nlive, nd=nd, dkmax=kmax, kmax=kmax, m=m)
                            if p["xlds"]:
                                assert p["lds"] <= 163840, p
                            if p["kind"] == PERSISTENT:
                                n += 1
                                assert p["expect_items"] == p["nrb"] - p["probe_blocks"] - p["tail_blocks"] + p["tail_shares"]
                                assert p["tail_blocks"] < p["wgs"] or p["tail_shares"] == 0, p
    assert n > 50


def test_plan_arguments_out_of_range():
    lib = L.load()
    out = L.PlanInfo()
    ok = dict(dtype=L.F32, mode=0, nlive=8, m=4096, maxfeat=5, kmax=2, num_cu=256, lds_max=163840)
    assert lib.srhip_plan_eval(ctypes.byref(L.PlanQuery(**ok)), ctypes.byref(out)) == 0
    assert lib.srhip_plan_eval(None, ctypes.byref(out)) < 0
    assert lib.srhip_plan_eval(ctypes.byref(L.PlanQuery(**ok)), None) < 0
    for bad in (dict(nlive=-1), dict(m=0), dict(num_cu=0), dict(dtype=3), dict(dtype=-1), dict(mode=3), dict(mode=-1)):
        assert lib.srhip_plan_eval(ctypes.byref(L.PlanQuery(**{**ok, **bad})), ctypes.byref(out)) < 0, bad
