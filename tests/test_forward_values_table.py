"""The golden table of exact forward values (tests/golden/forward_values.npz) and the trees that carry it to
the interpreter, without a device: the table regenerates bit for bit, the oracle (glibc) meets the bars the
device is held to on every point -- so the points are fair -- and the trees of tests/forward_values_common.py
compile to every handler of the instruction set, by name (srhip_program_handlers)."""
import os

import numpy as np
import pytest

import forward_values_common as fv
from conftest import GOLDEN

DTS = ("f32", "f64")


def _sr():
    import srhip

    return srhip


def test_table_regenerates_bit_for_bit():
    pytest.importorskip("mpmath")
    fresh = fv.GEN.build_table()
    z = fv.table()
    assert set(fresh) == set(z)
    for k in z:
        assert fv.GEN.same_bits(np.asarray(fresh[k]), np.asarray(z[k])), k


def test_table_size_and_operator_lists():
    from srhip.operators import BINARY, UNARY

    assert os.path.getsize(os.path.join(GOLDEN, "forward_values.npz")) < 256 * 1024
    z = fv.table()
    assert fv.P % 2 == 1 and fv.P >= 191
    # every operator of the package, once, under a name the package resolves
    assert sorted(UNARY[o][1] for o in fv.UN_OPS) == sorted({c for _, c in UNARY.values()})
    assert sorted(BINARY[o][1] for o in fv.BIN_OPS) == sorted({c for _, c in BINARY.values()})
    assert len(fv.UN_OPS) == 33 and len(fv.BIN_OPS) == 13
    cls = dict(zip(list(z["un_ops"]) + list(z["bin_ops"]), list(z["un_class"]) + list(z["bin_class"])))
    exact = "+ - * / neg abs square cube relu sign round floor ceil max min greater cond logical_or logical_and sqrt mod"
    rounded = ("log log2 log10 log1p acosh atanh_clip sinh cosh tanh asin acos atan asinh erf erfc gamma exp2 expm1 "
               "cbrt ^ atan2")
    assert sorted(o for o, c in cls.items() if c == "exact") == sorted(exact.split())
    assert sorted(o for o, c in cls.items() if c == "rounded") == sorted(rounded.split())
    assert sorted(o for o, c in cls.items() if c == "ulp1") == sorted("exp sin cos tan".split())
    for dt in DTS:
        assert z[f"un_x_{dt}"].dtype == fv.NP[dt] and z[f"un_x_{dt}"].shape == (fv.NUN, fv.P)
        assert z[f"un_y_{dt}"].shape == (33, fv.P) and z[f"bin_y_{dt}"].shape == (13, fv.P)
        # the special block counts almost everywhere: a mask is a rare rounding-boundary rejection
        assert z[f"un_sm_{dt}"].mean() > 0.98 and z[f"bin_sm_{dt}"].mean() > 0.98


@pytest.mark.parametrize("dt", DTS)
def test_oracle_meets_the_same_bars(oracle, dt):
    """scalar_un / scalar_bin on every point: bitwise for the exact and rounded-once classes, 1 ulp for
    exp sin cos tan in Float32, the relative bar in Float64."""
    from srhip.operators import BINARY, UNARY

    z = fv.table()
    T = fv.NP[dt]
    bad = []
    for i, op in enumerate(fv.UN_OPS):
        s = z["un_set"][i]
        x = np.concatenate([z[f"un_x_{dt}"][s], z[f"un_sx_{dt}"]])
        want = np.concatenate([z[f"un_y_{dt}"][i], z[f"un_sy_{dt}"][i]])
        mask = np.concatenate([np.ones(fv.P, bool), z[f"un_sm_{dt}"][i]])
        got = np.array([oracle.scalar_un(UNARY[op][1], v, T) for v in x], T)
        bad += [(op, x[r], got[r], want[r]) for r in fv.failing_rows(op, dt, got, want, mask)]
    for i, op in enumerate(fv.BIN_OPS):
        s = z["bin_set"][i]
        a = np.concatenate([z[f"bin_a_{dt}"][s], z[f"bin_sa_{dt}"]])
        b = np.concatenate([z[f"bin_b_{dt}"][s], z[f"bin_sb_{dt}"]])
        want = np.concatenate([z[f"bin_y_{dt}"][i], z[f"bin_sy_{dt}"][i]])
        mask = np.concatenate([np.ones(fv.P, bool), z[f"bin_sm_{dt}"][i]])
        got = np.array([oracle.scalar_bin(BINARY[op][1], u, v, T) for u, v in zip(a, b)], T)
        bad += [(op, a[r], b[r], got[r], want[r]) for r in fv.failing_rows(op, dt, got, want, mask)]
    assert not bad, (len(bad), bad[:12])


def oracle_worst_ulps(oracle, dt):
    """{operator: worst error in ulp of the oracle against the table over the finite points}."""
    from srhip.operators import BINARY, UNARY

    z = fv.table()
    T = fv.NP[dt]
    out = {}
    for i, op in enumerate(fv.UN_OPS):
        x = np.concatenate([z[f"un_x_{dt}"][z["un_set"][i]], z[f"un_sx_{dt}"]])
        want = np.concatenate([z[f"un_y_{dt}"][i], z[f"un_sy_{dt}"][i]])
        got = np.array([oracle.scalar_un(UNARY[op][1], v, T) for v in x], T)
        out[op] = float(np.nanmax(np.where(np.isfinite(want) & np.isfinite(got), fv.ulp_distance(got, want), 0)))
    for i, op in enumerate(fv.BIN_OPS):
        s = z["bin_set"][i]
        a = np.concatenate([z[f"bin_a_{dt}"][s], z[f"bin_sa_{dt}"]])
        b = np.concatenate([z[f"bin_b_{dt}"][s], z[f"bin_sb_{dt}"]])
        want = np.concatenate([z[f"bin_y_{dt}"][i], z[f"bin_sy_{dt}"][i]])
        got = np.array([oracle.scalar_bin(BINARY[op][1], u, v, T) for u, v in zip(a, b)], T)
        out[op] = float(np.nanmax(np.where(np.isfinite(want) & np.isfinite(got), fv.ulp_distance(got, want), 0)))
    return out


# ---- coverage: which handlers the trees compile to -------------------------------------------------------------
# Handlers no tree can compile to.  PUSHLCk is a push fused with the constant load that follows it, and a
# plain constant load inside a tree comes only from a heavy operator (^ mod atan2) whose left operand is a
# constant leaf and whose right operand is a feature leaf (every other constant operand is an immediate of its
# operator, or folded with its subtree); that operator then needs slot k + 1, so k = 7 does not fit K_MAX = 8.
# Int32 has no heavy operator at all, hence none of PUSHLCk, SLOADFk, SLOADCk.
UNREACHABLE = {
    "f32": {"PUSHLC7"}, "f64": {"PUSHLC7"},
    "i32": {f"{n}{k}" for n in ("PUSHLC", "SLOADF", "SLOADC") for k in range(8)},
}


def _used(prog, ntrees, names, derived=True):
    return {names[h] for t in range(ntrees) for h in prog.handlers(t, derived)}


@pytest.mark.parametrize("dt", DTS)
def test_trees_reach_every_handler(dt, monkeypatch):
    sr = _sr()
    names = fv.handler_names(sr)
    T = fv.NP[dt]
    exist = {n for h, n in enumerate(names) if sr.isa_handler_ok(h, T)}
    assert len(names) == 354 and exist == set(names)
    used = {}
    for K in (2, 4, 8):
        opts, sel, nodes, offs = fv.program_nodes(sr, dt, K)
        prog = sr.Program(None, nodes, offs, opts, T)
        assert prog.stats()["max_stack"] == K, (K, prog.stats())
        assert len(prog.derived_columns()) == 16
        u = _used(prog, len(sel), names) | _used(prog, len(sel), names, derived=False)
        slots = {n: fv.slot_of(n) for n in u}
        assert all(s is None or s < K for s in slots.values()), sorted(n for n, s in slots.items() if s is not None and s >= K)
        if K < 8:
            assert not any(n == f"UN.{w}" for n in u for w in fv.WIDE)
        used[K] = u
        # the stack need every tree was built for
        monkeypatch.setenv("SRHIP_NO_DERIVE", "1")
        for t in (0, len(sel) // 2, len(sel) - 1):
            one = sr.Program(None, nodes[offs[t]:offs[t + 1]], np.array([0, offs[t + 1] - offs[t]]), opts, T)
            assert one.stats()["max_stack"] == sel[t]["need"], sel[t]["label"]
        monkeypatch.delenv("SRHIP_NO_DERIVE")
    # the wide operators exist only in the K = 8 kernels: that is where their trees must land
    assert {f"UN.{w}" for w in fv.WIDE} <= used[8]
    assert used[2] <= used[4] | {"LOADC"} and used[4] <= used[8]
    missing = exist - used[8]
    assert missing == UNREACHABLE[dt], (sorted(missing - UNREACHABLE[dt]), sorted(UNREACHABLE[dt] - missing))
    # every form with k < K is in every variant that has it
    for K in (2, 4):
        want = {n for n in used[8] if (fv.slot_of(n) is None or fv.slot_of(n) < K) and n not in {f"UN.{w}" for w in fv.WIDE}}
        lost = {n for n in want - used[K] if not (n.startswith("PUSHLC") and fv.slot_of(n) == K - 1)}
        assert not lost, (K, sorted(lost))


def test_int32_trees_reach_every_handler():
    sr = _sr()
    names = fv.handler_names(sr)
    exist = {n for h, n in enumerate(names) if sr.isa_handler_ok(h, np.int32)}
    assert "DIV.AF" not in exist and "POW.SA0" not in exist and "UN.cos" not in exist and "UN.neg" in exist
    opts, trees, X, _ = fv.int_problem(sr)
    used = {}
    for K in (2, 4, 8):
        sel = [t for t in trees if t["need"] <= K]
        nodes, offs = sr.flatten([t["tree"] for t in sel], opts, np.int32)
        prog = sr.Program(None, nodes, offs, opts, np.int32)
        assert prog.stats()["max_stack"] == K
        used[K] = _used(prog, len(sel), names)
        assert all(fv.slot_of(n) is None or fv.slot_of(n) < K for n in used[K])
    missing = exist - used[8]
    assert missing == UNREACHABLE["i32"], (sorted(missing - UNREACHABLE["i32"]), sorted(UNREACHABLE["i32"] - missing))


def test_handler_names_are_unique_and_parse():
    sr = _sr()
    names = fv.handler_names(sr)
    assert len(set(names)) == len(names)
    assert names[0] == "END" and names[1] == "LOADF" and names[2] == "LOADC"
    assert {"SUB.SA3", "POW.AS0", "UN.erfc", "PUSHLC2", "COND.AS5", "MOD.SA3", "GREATER.CA", "ADD.FF"} <= set(names)
