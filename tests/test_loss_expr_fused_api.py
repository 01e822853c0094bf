"""The one-launch form of a loss expression without a device: its geometry function (srhip_plan_eval_lossx,
csrc/srhip_plan.cpp), the new entries of the C ABI, and the mirror's choice of coalescer constructor."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import srhip
from srhip import _lib
from srhip import device

from conftest import ROOT

import loss_expr_common as X

CU, LDS = 256, 160 * 1024  # an MI355X
NEW = ("srhip_eval_loss_expr_fused", "srhip_eval_loss_expr_submit", "srhip_batcher_create_expr", "srhip_plan_eval_lossx")


def _plan(dtype, nlive, m, maxfeat, num_cu=CU, lds_max=LDS):
    q = _lib.LossxPlanQuery(dtype=_lib.dtype_code(dtype), nlive=nlive, maxfeat=maxfeat, num_cu=num_cu, m=m, lds_max=lds_max)
    out = _lib.LossxPlanInfo()
    assert _lib.load().srhip_plan_eval_lossx(ctypes.byref(q), ctypes.byref(out)) == 0
    return out


SHAPES = [(1, 1), (24, 100), (3, 37 * 4096 + 5), (1500, 3), (64, 8193), (1024, 1_000_000), (1000, 10_000_000)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_geometry(dtype):
    lib = _lib.load()
    block = lib.srhip_lossx_block_rows()
    es = np.dtype(dtype).itemsize
    for nlive, m in SHAPES:
        for maxfeat in (0, 1, 4, 5, 9, 10, 40):
            for num_cu, lds_max in ((CU, LDS), (64, 64 * 1024), (1, LDS)):
                p = _plan(dtype, nlive, m, maxfeat, num_cu, lds_max)
                assert p.rb_rows > 0 and p.rb_rows % block == 0
                assert p.nblocks == -(-m // p.rb_rows)
                # XLDS goes off exactly where the columns exceed the budget it reports
                assert p.lds_cols == maxfeat * p.rb_rows * es
                assert 0 < p.lds_budget < lds_max
                assert bool(p.xlds) == (p.lds_cols <= p.lds_budget)
                assert p.lds == (p.lds_cols if p.xlds else 0) + 16 and p.lds <= lds_max
                # whole trees, every tree in one group
                assert 1 <= p.tpg <= max(1, nlive) and p.ngroups == -(-max(1, nlive) // p.tpg)
                # no more workgroups than the CUs it was given (one is resident per CU), nor than items
                assert p.wg_per_cu == 1
                assert 1 <= p.wgs <= num_cu and p.wgs <= p.nblocks * p.ngroups
                # the predictions' scratch: the launch geometry, never ntrees x m
                assert p.scratch_bytes == p.wgs * p.tpg * p.rb_rows * es
                assert p.scratch_bytes <= num_cu * 16 * block * es
    # Float64 with 5 features does not fit LDS at 4096 rows; Float32 does
    assert bool(_plan(dtype, 1024, 1_000_000, 5).xlds) == (dtype == np.float32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_scratch_does_not_grow_with_the_population(dtype):
    a = _plan(dtype, 1024, 1_000_000, 5)
    b = _plan(dtype, 2048, 2_000_000, 5)
    c = _plan(dtype, 1 << 20, 1 << 30, 5)
    assert a.scratch_bytes == b.scratch_bytes == c.scratch_bytes
    assert a.scratch_bytes < 1024 * 1_000_000 * np.dtype(dtype).itemsize // 16


def test_geometry_arguments():
    lib = _lib.load()
    q = _lib.LossxPlanQuery(dtype=_lib.dtype_code(np.float32), nlive=4, maxfeat=2, num_cu=8, m=100, lds_max=LDS)
    out = _lib.LossxPlanInfo()
    assert ctypes.sizeof(_lib.LossxPlanQuery) == 32 and ctypes.sizeof(_lib.LossxPlanInfo) == 72
    assert lib.srhip_plan_eval_lossx(ctypes.byref(q), ctypes.byref(out)) == 0
    assert lib.srhip_plan_eval_lossx(None, ctypes.byref(out)) < 0 and lib.srhip_plan_eval_lossx(ctypes.byref(q), None) < 0
    for field, bad in (("m", 0), ("nlive", -1), ("maxfeat", -1), ("num_cu", 0), ("lds_max", 0),
                       ("dtype", _lib.dtype_code(np.int32))):
        q2 = _lib.LossxPlanQuery.from_buffer_copy(q)
        setattr(q2, field, bad)
        assert lib.srhip_plan_eval_lossx(ctypes.byref(q2), ctypes.byref(out)) < 0, field


def test_abi_declares_and_exports_the_new_entries():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srhip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (srhip_\w+)", out))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported and name in _lib.SIGNATURES, name
    # the ticket type is the existing one: the new submit is completed by srhip_eval_loss_wait
    assert re.search(r"srhip_eval_loss_expr_submit\([^;]*srhip_eval_ticket\*\*\s*out_ticket\)", header, re.S)
    # the Julia lines
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW[:3]:
        assert ":%s" % name in integ, name


class _StubLib:
    """Records which batcher constructor the mirror calls; everything else is the real library's."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        if name in ("srhip_batcher_create", "srhip_batcher_create_expr"):
            def create(ctx, ds, ops, loss, max_batch, max_wait_us, out):
                self.calls.append((name, loss, int(max_batch), int(max_wait_us)))
                out._obj.value = 0xBA7C
                return 0
            return create
        if name in ("srhip_batcher_destroy", "srhip_batcher_set_clients"):
            return lambda *a: self.calls.append((name,)) or 0
        return getattr(self._real, name)


class _FakeHandle:
    handle = None


def test_coalescer_picks_its_constructor(monkeypatch):
    stub = _StubLib(_lib.load())
    monkeypatch.setattr(device._lib, "load", lambda: stub)
    opts = srhip.Options(binary_operators=("+", "*"), unary_operators=("cos",))
    ds = _FakeHandle()
    ds.dtype = np.dtype(np.float32)
    expr = srhip.ExprLoss(X.N("square", X.diff()), X.options())
    co = device.Coalescer(_FakeHandle(), ds, opts, expr, max_batch=7, max_wait_us=11)
    assert [c[0] for c in stub.calls] == ["srhip_batcher_create_expr"]
    assert stub.calls[0][1].value == expr.handle(np.float32).value and stub.calls[0][2:] == (7, 11)
    co.close()
    stub.calls.clear()
    co = device.Coalescer(_FakeHandle(), ds, opts, srhip.L2DistLoss(), nclients=3)
    assert [c[0] for c in stub.calls] == ["srhip_batcher_create", "srhip_batcher_set_clients"]
    assert not isinstance(stub.calls[0][1], ctypes.c_void_p)  # a srhip_loss by reference
    co.close()
    assert stub.calls[-1] == ("srhip_batcher_destroy",)
