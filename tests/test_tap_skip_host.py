"""rn_conv_tap_skip_plan (pure host arithmetic) against an independent count.

A pixel-major launch (rn_ctx_set_tap_skip, resnet.c_amd/csrc/rn_conv.hip) leaves out the K tiles of the taps that
fall into the padding.  Here the (output pixel, tap) pairs outside the image are counted one by one in numpy; the
plan must say pairs x K tiles per tap (Cin / 32) x N tiles x image blocks.  The tile of a candidate is the
documented table: 128x128, 128x64, 64x128, 64x64 for candidates 1-4 and again for 5-8; a layer on the chunked K
sum (K tiles >= 32, Cout % 4 == 0) runs 128x64 where the table says 128x128."""
import ctypes

import numpy as np
import pytest

from resnet_c_amd import _lib as L

F32, BF16 = L.RN_DTYPE_F32, L.RN_DTYPE_BF16
TILES = ((128, 128), (128, 64), (64, 128), (64, 64))

# (B, Cin, Cout, H, W, k, s, p): the shapes of tests/test_tap_skip_gpu.py
CASES = [(70, 64, 72, 3, 3, 3, 1, 1), (5, 32, 64, 1, 1, 3, 1, 1), (66, 128, 64, 5, 4, 3, 1, 1),
         (64, 64, 64, 6, 6, 3, 2, 1), (3, 32, 64, 7, 7, 5, 1, 2), (130, 32, 64, 19, 19, 3, 1, 1)]


def plan(case, tile, dtype=F32, dil=1):
    B, Cin, Cout, H, W, k, s, p = case
    m, kt, sk, rule = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
    st = L.lib().rn_conv_tap_skip_plan(dtype, B, Cin, Cout, H, W, k, s, p, dil, tile, ctypes.byref(m), ctypes.byref(kt),
                                       ctypes.byref(sk), ctypes.byref(rule))
    return st, int(m.value), int(kt.value), int(sk.value), int(rule.value)


def tile_of(case, cand):
    B, Cin, Cout, H, W, k, s, p = case
    bm, bn = TILES[(cand - 1) % 4]
    if k * k * Cin // 32 >= 32 and Cout % 4 == 0 and (bm, bn) == (128, 128):
        bn = 64
    return bm, bn


def invalid_pairs(case):
    """(output pixel, tap) pairs whose input pixel lies outside the image, and the output size"""
    B, Cin, Cout, H, W, k, s, p = case
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    n = 0
    for oh in range(ho):
        for ow in range(wo):
            for kh in range(k):
                for kw in range(k):
                    ih, iw = oh * s - p + kh, ow * s - p + kw
                    n += not (0 <= ih < H and 0 <= iw < W)
    return n, ho, wo


@pytest.mark.parametrize("case", CASES, ids=str)
def test_plan_is_the_count_of_padding_taps(case):
    B, Cin, Cout, H, W, k, s, p = case
    bad, ho, wo = invalid_pairs(case)
    assert bad > 0
    for cand in range(1, 9):
        bm, bn = tile_of(case, cand)
        blocks, tiles_n, cseg = -(-B // bm), -(-Cout // bn), Cin // 32
        st, m_tiles, k_tiles, skipped, _ = plan(case, cand)
        assert st == 1, (case, cand)
        assert m_tiles == ho * wo * blocks
        assert k_tiles == m_tiles * tiles_n * k * k * cseg
        assert skipped == bad * cseg * tiles_n * blocks, (case, cand)


def test_ineligible_forms():
    base = (8, 64, 64, 14, 14, 3, 1, 1)
    assert plan(base, 4)[0] == 1
    assert plan((8, 64, 64, 14, 14, 1, 1, 0), 4)[:4] == (0, 0, 0, 0)       # 1x1
    assert plan((8, 64, 64, 14, 14, 3, 1, 0), 4)[:4] == (0, 0, 0, 0)       # no padding
    assert plan((8, 64, 64, 14, 14, 3, 1, 2), 4, dil=2)[:4] == (0, 0, 0, 0)  # dilated
    assert plan((8, 48, 64, 14, 14, 3, 1, 1), 4)[:4] == (0, 0, 0, 0)       # Cin % 32 != 0
    assert plan(base, 4, dtype=BF16)[:4] == (0, 0, 0, 0)                   # bf16
    assert plan(base, 9)[0] == -1 and plan(base, 4, dtype=7)[0] == -1      # bad arguments


# every 3x3 layer of ResNet-50 at B = 256: (Cin = Cout, input side, stride) -> padded share of its K tiles in per
# cent, as (1 - valid taps / all taps) of the map: side n at stride 1 has (3n - 2)^2 valid of 9 n^2; stride 2 from
# side 2n loses the top row and the left column only, (3n - 1)^2 of 9 n^2
RESNET50 = {"layer1.x": ((64, 56, 1), 2.4), "layer2.0": ((128, 56, 2), 2.4), "layer2.x": ((128, 28, 1), 4.7),
            "layer3.0": ((256, 28, 2), 4.7), "layer3.x": ((256, 14, 1), 9.3), "layer4.0": ((512, 14, 2), 9.3),
            "layer4.x": ((512, 7, 1), 18.1)}


@pytest.mark.parametrize("name", sorted(RESNET50))
def test_resnet50_layers(name):
    (C, side, s), share = RESNET50[name]
    case = (256, C, C, side, side, 3, s, 1)
    bad, ho, wo = invalid_pairs(case)
    assert round(100.0 * bad / (9 * ho * wo), 1) == share
    for cand in range(0, 9):
        st, m_tiles, k_tiles, skipped, rule = plan(case, cand)
        assert st == 1 and k_tiles > 0
        assert round(100.0 * skipped / k_tiles, 1) == share, (name, cand)   # B = 256: whole image blocks
        if cand:
            bm, _ = tile_of(case, cand)
            assert m_tiles == ho * wo * (256 // bm)
