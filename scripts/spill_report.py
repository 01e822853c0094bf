#!/usr/bin/env python3
"""Register-allocation report of one kernel slice (no GPU needed).

usage: scripts/spill_report.py symbolicregression.jl_amd/csrc/srhip_eval_f32w.hip [--json] [--keep-asm FILE]

Compiles the slice to gfx950 assembly with the Makefile's device flags and prints, per kernel symbol:
.sgpr_spill_count, .vgpr_spill_count, .vgpr_count, the private segment size, and the number of
v_readlane_b32 / v_writelane_b32 (the moves of spilled SGPRs in and out of vector lanes; VALU-pipe
instructions) in the whole kernel, inside the tree loop and inside the tile loop (all of it, and outside
the basic blocks that make an out-of-line call, and per callee in the blocks that do).  For the interpreter kernels it also counts the full
memory waits in the tree loop's blocks laid out before the tile loop.

The loops are found by the assembler's "Loop Header: Depth=" / "Parent Loop" / "in Loop: Header=" block
comments (block placement scatters a loop's blocks, so membership is by those comments, not by line
range).  The interpreter kernel's nest is
    Depth=1  items of the launch (row blocks)      Depth=2  trees (claims)
    Depth=3  tiles of the row block                Depth=4  bytecode dispatch
so: dispatch loop = the Depth=4 loop with the most instructions, tile loop = its parent, tree loop = the
tile loop's parent, each with everything nested in it.
"""
import argparse
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "symbolicregression.jl_amd")


def make_var(text, name):
    m = re.search(r"^%s\s*[:?]?=\s*(.*)$" % re.escape(name), text, re.M)
    return m.group(1).strip() if m else ""


def device_flags(extra=""):
    """DEVFLAGS of the package Makefile, expanded."""
    mk = open(os.path.join(PKG, "Makefile")).read()
    flags = make_var(mk, "DEVFLAGS")
    subst = {"ARCH": make_var(mk, "ARCH"), "MLLVM": make_var(mk, "MLLVM"), "EXTRA": extra}
    flags = re.sub(r"\$\((\w+)\)", lambda m: subst.get(m.group(1), ""), flags)
    return make_var(mk, "HIPCC") or "hipcc", shlex.split(flags)


def compile_asm(src, out, extra=""):
    hipcc, flags = device_flags(extra)
    hipcc = os.environ.get("HIPCC", hipcc)
    cmd = [hipcc] + flags + ["--offload-device-only", "-S", "-I", os.path.join(ROOT, "include"), src, "-o", out]
    subprocess.run(cmd, check=True, cwd=PKG)


LABEL = re.compile(r"^([.\w$]+):")
BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)")
IN_LOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=(\d+)")
HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")
INSN = re.compile(r"^\s+[a-z]\w+")
READLANE = re.compile(r"^\s+v_readlane_b32\b")
WRITELANE = re.compile(r"^\s+v_writelane_b32\b")
CALL = re.compile(r"^\s+s_swappc_b64\b")
CALLEE = re.compile(r"^\s+s_add_u32\s+\w+,\s*\w+,\s*([.\w$]+)@rel32@lo", re.M)


def kernel_bodies(lines):
    """{symbol: (first line, last line)} of every kernel: from its label to its .Lfunc_end."""
    meta = set(re.findall(r"^\s+\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    out, cur = {}, None
    for i, ln in enumerate(lines):
        m = LABEL.match(ln)
        if m and m.group(1) in meta:
            cur = m.group(1)
            out[cur] = [i, i]
        elif cur and re.match(r"^\.Lfunc_end\d+:", ln):
            out[cur][1] = i
            cur = None
    return out


class Block:
    def __init__(self, start):
        self.start, self.end = start, start  # lines [start, end)
        self.loop = None                     # header label of the innermost loop, or None


def blocks_and_loops(lines, lo, hi):
    """The basic blocks of lines[lo:hi] with the innermost loop each lies in, and the loops:
    {header label: (depth, parent header label or None, header line)}, from the assembler's comments."""
    blocks, loops = [], {}
    i = lo
    while i < hi:
        m = BLOCK.match(lines[i])
        if not m:
            i += 1
            continue
        b = Block(i)
        if blocks:
            blocks[-1].end = i
        blocks.append(b)
        label = m.group(1)
        # the block's comment: this line and the comment-only lines that follow
        j, parents, depth, inl = i, [], None, None
        while j < hi and (j == i or lines[j].startswith("  ")) and (j == i or lines[j].lstrip().startswith(";")):
            c = lines[j]
            for pm in PARENT.finditer(c):
                parents.append((int(pm.group(2)), pm.group(1)))
            h = HEADER.search(c)
            if h:
                depth = int(h.group(1))
            il = IN_LOOP.search(c)
            if il:
                inl = il.group(1)
            j += 1
        if depth is not None and label:
            par = max(parents)[1] if parents else None
            loops[label] = (depth, par, i)
            b.loop = label
        else:
            b.loop = inl
        i += 1
    if blocks:
        blocks[-1].end = hi
    return blocks, loops


def within(loops, inner, outer):
    """inner loop is outer or nested in it"""
    while inner is not None:
        if inner == outer:
            return True
        inner = loops[inner][1] if inner in loops else None
    return False


def count_blocks(lines, blocks, pat, keep):
    return sum(1 for b in blocks if keep(b) for i in range(b.start, b.end) if pat.match(lines[i]))


def count(lines, lo, hi, pat):
    return sum(1 for i in range(lo, hi + 1) if pat.match(lines[i]))


def metadata(text):
    """{symbol: {field: value}} from the amdhsa.kernels notes."""
    out = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        d = {}
        for f in ("sgpr_spill_count", "vgpr_spill_count", "vgpr_count", "sgpr_count", "private_segment_fixed_size",
                  "kernarg_segment_size"):
            m = re.search(r"\.%s:\s+(\d+)" % f, blk)
            d[f] = int(m.group(1)) if m else None
        out[name.group(1)] = d
    return out


def report(asm_path):
    text = open(asm_path).read()
    lines = text.split("\n")
    meta = metadata(text)
    res = {}
    for sym, (lo, hi) in kernel_bodies(lines).items():
        r = dict(meta.get(sym, {}))
        r["name"] = demangle(sym)
        r["readlane"], r["writelane"] = count(lines, lo, hi, READLANE), count(lines, lo, hi, WRITELANE)
        blocks, loops = blocks_and_loops(lines, lo, hi)
        # the dispatch loop: the Depth=4 loop with the most instructions
        d4 = [(count_blocks(lines, blocks, INSN, lambda b, h=h: b.loop == h), h) for h, v in loops.items() if v[0] == 4]
        if d4:
            disp = max(d4)[1]
            tile = loops[disp][1]
            tree = loops[tile][1] if tile else None
            if tree:
                def moves(keep):
                    rl = count_blocks(lines, blocks, READLANE, keep)
                    wl = count_blocks(lines, blocks, WRITELANE, keep)
                    return {"readlane": rl, "writelane": wl, "lane_moves": rl + wl}
                in_tree = lambda b: within(loops, b.loop, tree)
                in_tile = lambda b: within(loops, b.loop, tile)
                r["tree_loop"] = moves(in_tree)
                r["tree_loop"]["instructions"] = count_blocks(lines, blocks, INSN, in_tree)
                r["tile_loop"] = moves(in_tile)
                # ... of which outside the blocks that make an out-of-line call (the generic losses, the rare
                # operators with out-of-line bodies): around a call the caller reloads what the callee may clobber
                calls = lambda b: any(CALL.match(lines[i]) for i in range(b.start, b.end))
                r["tile_loop"]["outside_call_blocks"] = moves(lambda b: in_tile(b) and not calls(b))["lane_moves"]
                # ... and per callee: the lane moves in the tile loop's blocks that call it ("?": a call whose
                # target is not named in its block), so that a caller can allow named rare callees only
                per = {}
                for b in blocks:
                    if in_tile(b) and calls(b):
                        names = set(CALLEE.findall("\n".join(lines[b.start:b.end]))) or {"?"}
                        n = moves(lambda x, b=b: x is b)["lane_moves"]
                        for c in names:
                            c = demangle(c)
                            per[c] = per.get(c, 0) + n
                r["tile_calls"] = per
                # a tree's set-up: the tree loop's blocks laid out before the tile loop's header
                tile_at = loops[tile][2]
                pro = lambda b: in_tree(b) and not in_tile(b) and b.start < tile_at
                r["tree_prologue"] = {
                    "lane_moves": moves(pro)["lane_moves"],
                    "vmcnt0_waits": count_blocks(lines, blocks, re.compile(r"^\s+s_waitcnt\s+.*vmcnt\(0\)"), pro),
                    "lgkmcnt0_waits": count_blocks(lines, blocks, re.compile(r"^\s+s_waitcnt\s+.*lgkmcnt\(0\)"), pro),
                }
        res[sym] = r
    return res


def demangle(sym):
    try:
        p = subprocess.run(["c++filt", sym], capture_output=True, text=True)
        return p.stdout.strip() or sym
    except OSError:
        return sym


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help="a .hip slice (compiled), or a .s file (read as is)")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--keep-asm", metavar="FILE")
    ap.add_argument("--extra", default="", help="extra compiler flags (the Makefile's EXTRA)")
    a = ap.parse_args()
    src = os.path.abspath(a.source)
    if src.endswith(".s"):
        res = report(src)
    else:
        with tempfile.TemporaryDirectory() as td:
            out = os.path.abspath(a.keep_asm) if a.keep_asm else os.path.join(td, "slice.s")
            compile_asm(src, out, a.extra)
            res = report(out)
    if a.json:
        print(json.dumps(res, indent=1, sort_keys=True))
        return 0
    for sym, r in sorted(res.items()):
        print(sym)
        print("  " + demangle(sym))
        print("  sgpr_spill_count=%s vgpr_spill_count=%s vgpr_count=%s sgpr_count=%s private_segment=%s kernarg=%s" % (
            r.get("sgpr_spill_count"), r.get("vgpr_spill_count"), r.get("vgpr_count"), r.get("sgpr_count"),
            r.get("private_segment_fixed_size"), r.get("kernarg_segment_size")))
        print("  whole kernel: v_readlane_b32=%d v_writelane_b32=%d" % (r["readlane"], r["writelane"]))
        for k in ("tree_loop", "tile_loop", "tree_prologue"):
            if k in r:
                print("  %-13s %s" % (k + ":", " ".join("%s=%d" % kv for kv in sorted(r[k].items()))))
        for c, n in sorted(r.get("tile_calls", {}).items()):
            if n:
                print("  tile-loop block calling %s: lane_moves=%d" % (c, n))
    return 0


if __name__ == "__main__":
    sys.exit(main())
