#!/usr/bin/env python3
"""VALU instructions on the straight path of each Float32 cos / sin leaf body (no GPU needed).

usage: scripts/trig_body_valu.py [--json] [--extra FLAGS] [slice.hip | slice.s ...]

Compiles the interpreter slices that hold the bodies (default: srhip_eval_f32w.hip, R = 16 and 4, and
srhip_eval_f32_loss.hip, R = 8 and 4) to gfx950 assembly with the Makefile's device flags
(scripts/spill_report.py) and counts, per jtrigf_a / jtrigf_bc / jtrigf_slow instance, the v_* instructions
from the body's label to its first return (s_setpc_b64).  The compiler lays the rare blocks -- the tie
re-evaluation by Julia's own kernels, and in the slow body the Payne-Hanek rows -- after the return, so
for A, B and C this is the path every unflagged wave runs; for the slow body it is the count of whatever
lies before the return, a figure to compare builds by and not a cost per row.  `per_row` divides by R (the
body's set-up, four v_mov of the leading coefficients, is spread over the rows).
--extra: the Makefile's EXTRA, e.g. "-DSRHIP_TRIG_QWORD=0 -DSRHIP_TRIG_CWFMA=0" for the bodies before the
quadrant word and the fused Cody-Waite step.
"""
import argparse
import json
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spill_report  # noqa: E402

ROOT = spill_report.ROOT
CSRC = os.path.join(spill_report.PKG, "csrc")
DEFAULT = [os.path.join(CSRC, "srhip_eval_f32w.hip"), os.path.join(CSRC, "srhip_eval_f32_loss.hip")]
# _ZN5srhip8jtrigf_aILi16ELi0EEE... / 9jtrigf_bcILi16ELi0ELb1EEE... / 11jtrigf_slowILi16ELi0EEE...
BODY = re.compile(r"^_ZN5srhip\d+jtrigf_(a|bc|slow)ILi(\d+)ELi([01])E(?:Lb([01])E)?E\w*:")
VALU = re.compile(r"^\s+v_\w+")
RET = re.compile(r"^\s+s_setpc_b64\b")


def bodies(asm_path):
    """{"bc<R=16,cos,C>": {"valu": n, "per_row": n / R}} for every body of the assembly file."""
    out, cur = {}, None
    for ln in open(asm_path):
        m = BODY.match(ln)
        if m:
            which, rows, kind, cw = m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)
            tier = {"a": "A", "slow": "slow"}.get(which) or ("C" if cw == "1" else "B")
            cur = "%s<R=%d,%s,%s>" % (which, rows, "sin" if kind else "cos", tier)
            out[cur] = {"valu": 0, "rows": rows}
        elif cur and RET.match(ln):
            cur = None
        elif cur and VALU.match(ln):
            out[cur]["valu"] += 1
    for r in out.values():
        r["per_row"] = round(r["valu"] / r.pop("rows"), 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sources", nargs="*", default=DEFAULT)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--extra", default="")
    a = ap.parse_args()
    res = {}
    for src in a.sources:
        src = os.path.abspath(src)
        if src.endswith(".s"):
            res.update(bodies(src))
            continue
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "slice.s")
            spill_report.compile_asm(src, out, a.extra)
            res.update(bodies(out))
    if a.json:
        print(json.dumps(res, indent=1, sort_keys=True))
        return 0
    for k, r in sorted(res.items()):
        print("%-24s valu=%-5d per_row=%.3f" % (k, r["valu"], r["per_row"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
