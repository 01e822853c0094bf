"""The share arithmetic of the persistent launch's last round (csrc/srhip_tail_shares.h, through
srhip_tail_share_parts; no device): the shares of Lb leftover blocks of S units partition the unit
space exactly, have at most two parts each, and every (block, order slot) lies in exactly one part."""
import ctypes

import numpy as np

import srhip._lib as L


def _parts(lib, lb, s, nshares, w):
    out = (ctypes.c_int32 * 6)()
    n = lib.srhip_tail_share_parts(lb, s, nshares, w, ctypes.cast(out, ctypes.c_void_p))
    assert 0 <= n <= 2, (lb, s, nshares, w, n)
    return [(out[3 * i], out[3 * i + 1], out[3 * i + 2]) for i in range(n)]


def test_shares_partition_the_leftover_blocks():
    lib = L.load()
    ntrees = 37  # fewer trees than some S, more than others, a multiple of none
    for wgs in range(1, 13):
        for lb in range(1, wgs + 1):  # (the launch plan only has Lb < wgs; the arithmetic needs Lb <= nshares)
            for s in (2, 3, 8, 32, 64, 128):
                for nshares in (wgs, 2 * wgs):
                    nxt = 0  # the shares are contiguous and in order: each starts where the last ended
                    seen = np.zeros((lb, ntrees), dtype=np.int32)
                    sizes = []
                    for w in range(nshares):
                        parts = _parts(lib, lb, s, nshares, w)
                        n = 0
                        for b, u0, u1 in parts:
                            assert 0 <= b < lb and 0 <= u0 < u1 <= s, (lb, s, nshares, w, parts)
                            assert b * s + u0 == nxt, (lb, s, nshares, w, parts)
                            nxt = b * s + u1
                            n += u1 - u0
                            # the kernel's mapping: tree index ti of the part -> order slot
                            wd = u1 - u0
                            cnt = ntrees // s * wd + min(max(ntrees % s - u0, 0), wd)
                            slots = [(ti // wd) * s + u0 + ti % wd for ti in range(cnt)]
                            assert slots == sorted(slots) and all(x < ntrees for x in slots)
                            assert slots == [x for x in range(ntrees) if u0 <= x % s < u1]
                            seen[b, slots] += 1
                        sizes.append(n)
                    assert nxt == lb * s, (lb, s, nshares)
                    assert max(sizes) - min(sizes) <= 1, (lb, s, nshares, sizes)
                    assert np.all(seen == 1), (lb, s, nshares)


def test_share_arguments_out_of_range():
    lib = L.load()
    out = (ctypes.c_int32 * 6)()
    p = ctypes.cast(out, ctypes.c_void_p)
    assert lib.srhip_tail_share_parts(3, 64, 2, 0, p) < 0      # fewer shares than blocks
    assert lib.srhip_tail_share_parts(3, 64, 4, 4, p) < 0      # share past the last
    assert lib.srhip_tail_share_parts(0, 64, 4, 0, p) < 0
    assert lib.srhip_tail_share_parts(3, 64, 4, 0, None) < 0
    assert lib.srhip_tail_share_parts(1 << 12, 1 << 10, 1 << 12, 0, p) < 0  # the product leaves 32 bits
