"""Float32 cos / sin through the quadrant word, the fused Cody-Waite step and tier C's new end
(srhip_eval_impl.h jtrigf_*; include/srhip_math.h srm_jqword / srm_jqword_wide / srm_jred_cw_fma /
SRM_JQW_MAXF), on the device: tools/check_trig_quadrant.c proves the arithmetic on the host, this drives
whole waves through every leaf body -- as an operator output and as a derived feature column, in
prediction and loss mode, at 1024 rows (R = 8), 8192 rows (R = 16, a grid launch) and 64 x 2048 rows (the
persistent hot form) -- and requires the oracle's bits.

One dataset per body: every row of a dataset lies in one tier's range, so every wave of it takes that
body.  Each holds the tier's special rows and its flagged inputs (tests/golden/trig_tie_inputs.npy),
placed so that every row slot of a lane holds a flagged row in some wave: a tile's row at offset o sits
in slot (o / 256) * 4 + o % 4 of lane (o / 4) % 64."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
PIO4 = F(0.78539819)       # SRM_JPIO4F: tier A below it
B_END = F(7.068583)        # SRM_J9PIO4F: tier B up to it
C_END = F(1647098.625)     # SRM_JQW_MAXF: tier C below it
BIG = F(421657440.0)       # Float32(2^28 pi/2): Payne-Hanek from it
SIZES = (1024, 8192, 64 * 2048)


def _near(ks):
    """Float32(k pi/2) and its two neighbours, both signs."""
    c = np.array([k * (np.pi / 2) for k in ks], dtype=np.float64).astype(F)
    v = np.concatenate([np.nextafter(c, F(0)), c, np.nextafter(c, F(np.inf))])
    return np.concatenate([v, -v])


def _log_uniform(rng, lo, hi, n):
    return (np.exp(rng.uniform(np.log(lo), np.log(hi), n)) * rng.choice([-1.0, 1.0], n)).astype(F)


def _groups(n, rng, ties):
    """{name: the n rows of one dataset}: padding that keeps every wave in the body, the special rows at the
    front of the tiles, the flagged inputs spread over the row slots."""
    a = np.abs(ties)
    below = lambda v: np.nextafter(F(v), F(0))
    k20 = 1 << 20
    spec = {
        "A": (rng.uniform(-0.78, 0.78, n).astype(F), ties[a < PIO4],
              [0.0, -0.0, 1e-30, -1e-30, 2.44140625e-4, 3.4526698e-4, below(PIO4), -below(PIO4)]),
        "B": (rng.uniform(-7.0, 7.0, n).astype(F), ties[(a >= PIO4) & (a <= B_END)],
              np.concatenate([[0.0, -0.0, PIO4, -PIO4, B_END, -B_END], _near([1, 2, 3, 4])])),
        "C": (_log_uniform(rng, 0.5, 1.6e6, n), ties[(a > B_END) & (a < C_END)],
              np.concatenate([[0.0, -0.0, below(C_END), -below(C_END), B_END, np.nextafter(B_END, F(8)), 3.0061, -3.0061],
                              _near([1, 3, 4, 5, 6, 7, 8, 1000, k20 - 3, k20 - 2, k20 - 1])])),
        # the first float past tier C in every 512 rows: the slow body, all of its rows fast (the wide word)
        "C_end": (_log_uniform(rng, 0.5, 1.6e6, n), ties[(a > B_END) & (a < C_END)],
                  [C_END, -C_END, np.nextafter(C_END, F(np.inf)), below(C_END), 0.0, -0.0]),
        "wide": (_log_uniform(rng, float(C_END), 4.2e8, n), ties,
                 np.concatenate([[C_END, -C_END, below(BIG), -below(BIG), 0.0, -0.0, 1.0, -7.0],
                                 _near([k20 - 1, k20, k20 + 1, k20 + 2, 3 * k20 + 1, (1 << 28) - 2, (1 << 28) - 1])])),
        "payne_hanek": (_log_uniform(rng, 0.5, 1.6e6, n), ties[a >= PIO4],
                        [3.0e30, -3.0e30, BIG, -BIG, 1e38, 0.0, -0.0]),
    }
    out = {}
    ntiles = n // 1024
    for name, (pad, tv, sp) in spec.items():
        sp = np.asarray(sp, dtype=F)
        if name == "wide":
            sp = sp[np.abs(sp) < BIG]
        # flagged input i: slot i % 16, one lane and tile per (slot, i // 16), so no two share a row
        assert len(tv) <= 16 * 64
        slot, j = np.arange(len(tv)) % 16, np.arange(len(tv)) // 16
        pos = (j % ntiles) * 1024 + (slot // 4) * 256 + ((13 * j + slot) % 64) * 4 + slot % 4
        assert len(np.unique(pos)) == len(tv) and set(((pos % 1024) // 256) * 4 + pos % 4) == set(range(min(16, len(tv))))
        pad[pos] = tv
        # the special rows on the first rows no flagged input took; a body's forcing row (its first two specials,
        # one per sign) again in every 512 rows, the rows of one wave at R = 8
        free = np.setdiff1d(np.arange(n), pos)
        pad[free[:len(sp)]] = sp
        if name in ("C_end", "payne_hanek"):
            for t in range(0, n, 512):
                pad[free[free >= t + 300][0]] = sp[(t // 512) % 2]
        out[name] = pad
    return out


@pytest.fixture(scope="module")
def setup(ctx):
    import srhip

    opts = srhip.Options(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "sin"))
    x1, x2 = srhip.Node("x1"), srhip.Node("x2")
    trees = [srhip.cos(x1 * x2), srhip.sin(x1 * x2), srhip.cos(x1), srhip.sin(x1),
             srhip.cos(x1) + srhip.sin(x1 * x2)]
    nodes, offs = srhip.flatten(trees, opts, np.float32)
    prog = srhip.Program(ctx, nodes, offs, opts, np.float32)
    ties = np.load(os.path.join(HERE, "golden", "trig_tie_inputs.npy")).view(np.float32).ravel()
    assert len(ties) > 300  # every flagged input of every tier, both kinds
    return opts, nodes, offs, prog, ties, len(trees)


@pytest.mark.parametrize("n", SIZES)
def test_every_trig_body_returns_the_oracles_bits(ctx, oracle, setup, n):
    import srhip

    opts, nodes, offs, prog, ties, ntrees = setup
    for name, x in _groups(n, np.random.default_rng(n), ties).items():
        a = np.abs(x)
        if name == "A":
            assert a.max() < PIO4
        elif name == "B":
            assert a.max() <= B_END
        elif name == "C":
            assert a.max() < C_END
        elif name in ("C_end", "wide"):
            assert C_END <= a.max() < BIG and all(a[t:t + 512].max() >= C_END for t in range(0, n, 512))
        else:
            assert all(a[t:t + 512].max() >= BIG for t in range(0, n, 512))
        X = np.stack([x, np.ones_like(x)])
        pred, ok = prog.eval_predict(srhip.DeviceDataset(ctx, X))
        for t in range(ntrees):
            ref, rok = oracle.eval_tree(nodes[offs[t]:offs[t + 1]], opts.binop_codes, opts.unaop_codes, X)
            assert bool(ok[t]) == rok, (name, t)
            assert rok, (name, t)  # every row is finite: no tree may fail
            bad = np.nonzero(pred[t].view(np.uint32) != ref.view(np.uint32))[0]
            assert len(bad) == 0, (name, t, bad[:8], x[bad[:8]], pred[t][bad[:8]], ref[bad[:8]])
        # loss mode (at 64 x 2048 rows the persistent launch and its derived columns) against the oracle's losses
        y = np.zeros_like(x)
        dl, dok = prog.eval_loss(srhip.DeviceDataset(ctx, X, y), srhip.L2DistLoss())
        ol, _, ook, _ = oracle.eval_loss_batch(nodes, offs, opts.binop_codes, opts.unaop_codes, X, y, None, 0, 0.0)
        assert np.array_equal(dok, ook), name
        for t in np.nonzero(ook)[0]:
            assert dl[t] == ol[t] or abs(dl[t] - ol[t]) <= 1e-6 * abs(ol[t]), (name, t, dl[t], ol[t])
