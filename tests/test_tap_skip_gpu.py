"""Pixel-major tiles that skip the padding taps (rn_ctx_set_tap_skip) on poisoned outputs between guard bands.

In the manner of tests/test_schedules_gpu.py: every launch gets a fresh output filled with 0xA5 between fresh
guards and NaN guards around every input (the typed runners of tests/views.py), and is held to "written
everywhere", the guards, test_ops_gpu.assert_close against the float64 reference (K, K + 4 with an epilogue) and,
bit for bit, the row-major launch (mode 1) on the same tile candidate.  No tolerance of its own.

A launch in mode 2 counts only if the context's counters say it took the pixel-major kernel and left out exactly
the K tiles rn_conv_tap_skip_plan gives for the shape and the candidate (held against an independent count in
tests/test_tap_skip_host.py); a launch in mode 1 must leave the counters alone.  Nothing falls back silently.

Cases (B, Cin, Cout, H, W, k, s, p):
  ragged     (70, 64, 72, 3, 3, 3, 1, 1)   70 images: ragged image block for BM 64 and BM 128; Cout 72: ragged N
  centre     (5, 32, 64, 1, 1, 3, 1, 1)    a 1x1 map: only the centre tap is inside; Cin 32: one K tile per tap
  chunked    (66, 128, 64, 5, 4, 3, 1, 1)  36 K tiles: the chunked K sum, fold points at multiples of 6, four K tiles
                                           per tap -- the fold point 6 lies inside tap 1, which the top row skips
  stride2    (64, 64, 64, 6, 6, 3, 2, 1)   stride 2: padding at the top and on the left only
  taps25     (3, 32, 64, 7, 7, 5, 1, 2)    25 taps, one K tile each: pairs of K tiles straddle taps and kernel rows
"""
import ctypes

import numpy as np
import pytest

import resnet_c_amd as R
import views as V
from resnet_c_amd import _lib as L
from test_schedules_gpu import F32, Figures, conv_operands, conv_reference, schedule

pytestmark = pytest.mark.gpu

CASES = {"ragged": (70, 64, 72, 3, 3, 3, 1, 1), "centre": (5, 32, 64, 1, 1, 3, 1, 1),
         "chunked": (66, 128, 64, 5, 4, 3, 1, 1), "stride2": (64, 64, 64, 6, 6, 3, 2, 1),
         "taps25": (3, 32, 64, 7, 7, 5, 1, 2)}


class tap_skip:
    """rn_ctx_set_tap_skip for the block; the library's rule afterwards"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        R.get_ctx().set_tap_skip(self.mode)

    def __exit__(self, *exc):
        R.get_ctx().set_tap_skip(0)


def planned(case, cand):
    B, Cin, Cout, H, W, k, s, p = case
    sk = ctypes.c_uint64()
    st = L.lib().rn_conv_tap_skip_plan(F32, B, Cin, Cout, H, W, k, s, p, 1, cand, None, None, ctypes.byref(sk), None)
    assert st == 1, f"{case} candidate {cand}: not eligible"
    return int(sk.value)


def run_counted(case, cand, mode, x, w, s, p, sc, sh, res, relu):
    """one launch in `mode` on candidate `cand`; the counters must say what it did"""
    ctx = R.get_ctx()
    before = ctx.tap_skip_stats()
    with schedule(tile=cand), tap_skip(mode):
        got = V.run_conv_dt(x, w, s, p, sc, sh, res, relu, F32, F32)
    after = ctx.tap_skip_stats()
    took = after["launches"] - before["launches"], after["k_tiles_skipped"] - before["k_tiles_skipped"]
    want = (1, planned(case, cand)) if mode == 2 else (0, 0)
    assert took == want, f"{case} candidate {cand} mode {mode}: (pixel-major launches, K tiles skipped) {took}, planned {want}"
    return got


@pytest.mark.parametrize("epilogue", [True, False], ids=["epilogue", "raw"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_tap_skip_tiles(name, epilogue):
    case = CASES[name]
    B, Cin, Cout, H, W, k, s, p = case
    x, w, sc, sh, res = conv_operands(case, 700 + sum(case), F32)
    if not epilogue:
        sc = sh = res = None
    ref = conv_reference(x, w, s, p, sc, sh, res, epilogue, F32, name)
    fig = Figures(f"test_tap_skip_tiles[{name}-{'epilogue' if epilogue else 'raw'}]")
    for cand in range(1, 9):
        off = run_counted(case, cand, 1, x, w, s, p, sc, sh, res, epilogue)
        on = run_counted(case, cand, 2, x, w, s, p, sc, sh, res, epilogue)
        what = f"{name} candidate {cand}"
        fig.values(on, ref, Cin * k * k, False, epilogue, what)
        assert on.shape == off.shape and np.array_equal(on, off), f"{what}: pixel-major bits differ from row-major"
    fig.done()


# The resident grid walking pixel-major tiles: (130, 32, 64, 19, 19, 3, 1, 1) has 361 pixels x 3 blocks of 64
# images = 1083 M tiles (x one N tile) on the 64-row candidates and 361 x 2 = 722 on the 128-row ones.  A resident
# grid is 256 CUs x the blocks per CU of the instantiation, which __launch_bounds__ gives as 2 (128x128), 3
# (128x64, 64x128), 4 (64x64): 512 / 768 / 768 / 1024 slots.  Candidates 5 (722 tiles on 512 slots) and 7 (1083 on
# 768) must walk; 6 (722 on 768) cannot, and 8 (1083 on 1024) walks only if the occupancy query allows no fifth
# block per CU, so for these two the grid is only held to the tile count.  Every block writes debug-stamp slot 0
# when it starts, so the blocks that wrote it are the grid (as in test_resident_grid_walks).
def test_tap_skip_resident_grid_walks():
    from resnet_c_amd.tensor import _DeviceBuffer
    case = (130, 32, 64, 19, 19, 3, 1, 1)
    B, Cin, Cout, H, W, k, s, p = case
    x, w, sc, sh, res = conv_operands(case, 800 + sum(case), F32)
    ref = conv_reference(x, w, s, p, sc, sh, res, True, F32, "resident")
    ctx, lib = R.get_ctx(), L.lib()
    nblk = 1083
    stamps = _DeviceBuffer(ctx, nblk * 16 * 8)
    fig = Figures("test_tap_skip_resident_grid_walks")
    off = run_counted(case, 8, 1, x, w, s, p, sc, sh, res, True)
    try:
        for cand in range(5, 9):
            tiles = H * W * -(-B // (128 if cand in (5, 6) else 64))
            L.check(lib.rn_memset(ctx.handle, stamps.ptr, 0, nblk * 128), "memset", ctx.handle)
            L.check(lib.rn_ctx_set_debug_stamps(ctx.handle, stamps.ptr), "stamps", ctx.handle)
            on = run_counted(case, cand, 2, x, w, s, p, sc, sh, res, True)
            L.check(lib.rn_ctx_set_debug_stamps(ctx.handle, None), "stamps", ctx.handle)
            slots = np.zeros(nblk * 16, np.uint64)
            L.check(lib.rn_memcpy_d2h(ctx.handle, slots.ctypes.data, stamps.ptr, slots.nbytes), "d2h", ctx.handle)
            grid = int((slots.reshape(nblk, 16)[:, 0] != 0).sum())
            what = f"pixel-major resident candidate {cand}: grid {grid}, {tiles} tiles"
            print(f"\n  {what}")
            if cand in (5, 7):
                assert 0 < grid < tiles, what + ": the resident grid does not walk at this size"
            else:
                assert 0 < grid <= tiles, what
            fig.values(on, ref, Cin * k * k, False, True, what)
            assert np.array_equal(on, off), f"{what}: pixel-major bits differ from row-major"
    finally:
        lib.rn_ctx_set_debug_stamps(ctx.handle, None)
    fig.done()


def test_resnet50_logits_do_not_depend_on_the_mode():
    """ResNet-50, B = 4: the logits with the pixel-major tiles wherever eligible are those without them, bit for
    bit, and the forward in mode 2 really took pixel-major launches (16 3x3 layers, all eligible)."""
    state = R.weights.generate_state("resnet50", seed=0)
    x = R.weights.generate_input(4, seed=11)
    ctx = R.get_ctx()
    model = R.NativeModel("resnet50", state=state)
    try:
        with tap_skip(1):
            n0 = ctx.tap_skip_stats()["launches"]
            off = model.forward(x, fused=True)
            assert ctx.tap_skip_stats()["launches"] == n0
        with tap_skip(2):
            on = model.forward(x, fused=True)
            assert ctx.tap_skip_stats()["launches"] - n0 == 16
    finally:
        model.close()
    assert off.shape == on.shape == (4, 1000) and np.isfinite(off).all()
    assert np.array_equal(on, off)
