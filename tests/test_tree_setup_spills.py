"""Register allocation of the interpreter's hot form, from the compiler's own report:
scripts/spill_report.py compiles the wide Float32 slice to assembly and counts the v_readlane_b32 /
v_writelane_b32 that move spilled scalars in and out of vector lanes -- VALU-pipe instructions, in a
kernel that is VALU-issue bound.  No GPU needed; skipped without hipcc.  Looks only at
register-allocation metadata and lane moves."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

SLICE = os.path.join(ROOT, "symbolicregression.jl_amd", "csrc", "srhip_eval_f32w.hip")
# eval_kernel<T, R, K, MODE, XLDS, FORM>: the wide Float32 loss kernel over staged row blocks
HOT = "eval_kernel<float, 16, 2, 0, true, 1>"      # FORM_HOT
GENERAL = "eval_kernel<float, 16, 2, 0, true, 0>"  # FORM_GENERAL
# the general form before the hot form existed, by the same script (profiles/r08_tree_setup_spills.txt):
# lane moves inside the tree loop, and spilled vector registers
PARENT_TREE_LOOP_LANE_MOVES = 157
PARENT_VGPR_SPILLS = 16
# Out-of-line callees whose call blocks inside the tile loop may hold lane moves:
#  - loss_rows_generic: the generic-loss call path (the exception the bound was set with);
#  - heavy_un<float, 16, 24>, erfc: a DEVIATION from that bound.  Its body, compiled in the same unit,
#    clobbers eight scalar registers the tile loop keeps, so the caller reloads them after the call (8
#    v_readlane_b32 per erfc instruction per tile).  erfc is not among C2's operators; no other operator's
#    call block -- exp and the slow path of cos, which C2 runs, included -- may hold any.
ALLOWED_CALLEES = ("srhip::loss_rows_generic<float, 16>(", "srhip::heavy_un<float, 16, 24>(")


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def report():
    if not _hipcc():
        pytest.skip("hipcc not found")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "spill_report.py"), SLICE, "--json"],
                         capture_output=True, text=True, check=True).stdout
    return json.loads(out)


def _kernel(report, name):
    """The report of the kernel whose demangled name holds `name`."""
    hits = [r for r in report.values() if name in r["name"]]
    assert len(hits) == 1, (name, sorted(r["name"] for r in report.values()))
    assert "tile_loop" in hits[0], "the tree / tile / dispatch loop nest was not found in " + hits[0]["name"]
    return hits[0]


def test_hot_form_tile_loop_has_no_lane_moves(report):
    """Nothing between the tile loop's header and its back edge moves a scalar through a vector lane, other
    than in the call blocks of the callees named above: not in any block without a call, and not in the
    call block of any other out-of-line operator body."""
    r = _kernel(report, HOT)
    assert r["tile_loop"]["outside_call_blocks"] == 0, r["tile_loop"]
    assert r["tile_loop"]["writelane"] == 0, r["tile_loop"]
    callees = r["tile_calls"]
    # (the operators C2 runs per instruction are among the call blocks looked at)
    # (exp's body and the slow path of cos / sin, whose fast path is inline)
    assert any("heavy_un<float, 16, 8>(" in c for c in callees) and any("jtrigf_slow<16" in c for c in callees), sorted(callees)
    other = {c: n for c, n in callees.items() if n and not any(a in c for a in ALLOWED_CALLEES)}
    assert not other, other


def test_hot_form_tree_loop_holds_a_quarter_of_the_lane_moves(report):
    r = _kernel(report, HOT)
    assert r["tree_loop"]["lane_moves"] <= PARENT_TREE_LOOP_LANE_MOVES // 4, r["tree_loop"]


def test_hot_form_registers(report):
    r = _kernel(report, HOT)
    assert r["vgpr_count"] <= 128 and r["vgpr_spill_count"] <= PARENT_VGPR_SPILLS, r
    g = _kernel(report, GENERAL)  # the general form of this slice: as before
    assert g["vgpr_count"] <= 128 and g["vgpr_spill_count"] <= PARENT_VGPR_SPILLS, g
    assert g["tree_loop"]["lane_moves"] <= PARENT_TREE_LOOP_LANE_MOVES, g["tree_loop"]
