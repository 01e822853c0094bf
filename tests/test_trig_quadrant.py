"""Float32 cos / sin, the quadrant word and the fused Cody-Waite step (include/srhip_math.h srm_jqword /
srm_jqword_wide / srm_jred_cw_fma; srhip_eval_impl.h jtrigf_*).  No GPU needed.

* tools/check_trig_quadrant.c proves over all 2^32 inputs, per tier and kind, that the new reduction equals
  the old one bit for bit, that the word's two bits are the integer quadrant's, that SRM_JQW_MAXF is the
  largest valid end of tier C, and that the composed rows return srm_jtrigf's bits on every unflagged input
  with the flagged set unchanged -- its dump must reproduce tests/golden/trig_tie_inputs.npy.
* The code shape, from the compiler (scripts/trig_body_valu.py, scripts/spill_report.py; skipped without
  hipcc): every tier-B and tier-C body, R = 16 and R = 8, runs at least 2 VALU instructions per row fewer
  than its parent's recorded count, and the wide Float32 kernels' registers, scratch and spills are not
  above the parent's (profiles/r13_trig_quadrant_ab.txt)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "symbolicregression.jl_amd", "csrc")

# The parent's bodies (the integer quadrant code, the four-instruction Cody-Waite step, sin's x == 0 select in
# every row), by scripts/trig_body_valu.py: v_* instructions from the body's label to its return.
PARENT_VALU = {
    "bc<R=16,cos,B>": 404, "bc<R=16,cos,C>": 436, "bc<R=16,sin,B>": 420, "bc<R=16,sin,C>": 532,
    "bc<R=8,cos,B>": 204, "bc<R=8,cos,C>": 220, "bc<R=8,sin,B>": 212, "bc<R=8,sin,C>": 268,
}
# The parent's wide Float32 loss kernels over staged row blocks, by scripts/spill_report.py
PARENT_KERNELS = {
    "eval_kernel<float, 16, 2, 0, true, 1>": dict(vgpr_count=123, private_segment_fixed_size=160,
                                                  vgpr_spill_count=16, sgpr_spill_count=124),
    "eval_kernel<float, 16, 2, 0, true, 0>": dict(vgpr_count=128, private_segment_fixed_size=160,
                                                  vgpr_spill_count=16, sgpr_spill_count=214),
}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("check_trig_quadrant")
    exe, dump = str(d / "check_trig_quadrant"), str(d / "ties.bin")
    subprocess.run(["gcc", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fopenmp",
                    os.path.join(ROOT, "tools", "check_trig_quadrant.c"), "-lm", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, SRHIP_TIE_DUMP=dump))
    return r, dump


def test_quadrant_word_and_fused_reduction_exhaustive(checker):
    r, _ = checker
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert "fn = 1048576.0 there, 1048575.0 at the float below" in out[0], out[0]
    for kind in ("cos", "sin"):
        red = [ln for ln in out if ln.startswith(kind + " reduction:")]
        assert len(red) == 1 and red[0].endswith("differs on 0"), red
        word = [ln for ln in out if ln.startswith(kind + " quadrant word:")]
        assert len(word) == 1 and " 0 with |fn| >= 2^20" in word[0] and word[0].count("differ on 0") == 2, word
        rows = [ln for ln in out if ln.startswith(kind + " new rows")]
        assert len(rows) == 1 and rows[0].count(" / 0") == 3 and rows[0].endswith("row on 0"), rows
        for part in rows[0].split(":", 1)[1].split(";")[0].split(","):
            n_in, flagged = int(part.split()[1]), int(part.split("inputs")[1].split("/")[0])
            assert 0 < flagged < 1e-6 * n_in, rows[0]


def test_flagged_inputs_are_the_fixture(checker):
    r, dump = checker
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dump, dtype=np.uint32)
    want = np.load(os.path.join(ROOT, "tests", "golden", "trig_tie_inputs.npy")).view(np.uint32).ravel()
    assert np.array_equal(got, want), (len(got), len(want))


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def shape(tmp_path_factory):
    """The assembly of the two slices that hold the R = 16 and R = 8 bodies, compiled side by side:
    (body counts, kernel report of the wide slice)."""
    if not _hipcc():
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("trig_quadrant_asm")
    jobs = []
    for name in ("srhip_eval_f32w", "srhip_eval_f32_loss"):
        asm = str(d / (name + ".s"))
        jobs.append((asm, subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "scripts", "spill_report.py"), os.path.join(CSRC, name + ".hip"),
             "--json", "--keep-asm", asm], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    reports = []
    for asm, p in jobs:
        out, err = p.communicate()
        assert p.returncode == 0, err
        reports.append(json.loads(out))
    bodies = json.loads(subprocess.run(
        [sys.executable, os.path.join(ROOT, "scripts", "trig_body_valu.py"), "--json"] + [a for a, _ in jobs],
        capture_output=True, text=True, check=True).stdout)
    return bodies, reports[0]


@pytest.mark.parametrize("body", sorted(PARENT_VALU))
def test_tier_bodies_run_two_valu_per_row_fewer(shape, body):
    bodies, _ = shape
    rows = int(body.split("R=")[1].split(",")[0])
    new, parent = bodies[body]["valu"], PARENT_VALU[body]
    print("%s: parent %d, new %d VALU: %.3f per row fewer" % (body, parent, new, (parent - new) / rows))
    assert parent - new >= 2 * rows, (body, parent, new)


@pytest.mark.parametrize("kernel", sorted(PARENT_KERNELS))
def test_wide_kernel_registers_not_above_the_parent(shape, kernel):
    _, report = shape
    hits = [r for r in report.values() if kernel in r["name"]]
    assert len(hits) == 1, sorted(r["name"] for r in report.values())
    for field, bound in PARENT_KERNELS[kernel].items():
        assert hits[0][field] <= bound, (kernel, field, hits[0][field], bound)
