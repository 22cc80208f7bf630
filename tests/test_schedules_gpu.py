"""Every contraction schedule on a poisoned output between guard bands (tests/views.py).

"This schedule changes which block computes a tile, never a bit of the result" is asserted elsewhere by calling
a helper of resnet_c_amd/ops.py in a loop and comparing each result with the first.  Those helpers allocate the
output, never fill it and free it again; if the allocator hands the same block to the next call, a tile that the
next schedule never writes still holds the previous schedule's correct result.  And a ReLU zero that was never
stored is within every value bound of the suite (tests/test_written_host.py shows both on emulations).

Here every single launch gets a fresh output filled with 0xA5 between fresh guards of 256 output rows, and fresh
NaN guards around every input (the typed runners of tests/views.py).  Each launch is held to

  written everywhere   no element left at the fill (fetch(written=True)); the reference is checked on the CPU to
                       hold no element with the fill's bit pattern (V.assert_no_poison)
  guards               every guard byte of every operand as uploaded
  values               test_ops_gpu.assert_close(K, K + 4 with an epilogue) for fp32 results,
                       bf16_ref.assert_bf16_rounded for bf16 results, against bf16_ref.conv64 / epilogue64
  bits                 equal to the first schedule's where the project documents it (not for split-K: bound +
                       the same bits on a second run)

No tolerance of its own.  No ops.* helper allocates an output here.

Schedule (resnet.c_amd/csrc/)                          reached by
  launch_gemm: conv_tile 1-4, one block per tile          test_four_wave_tiles[*] (candidates 1-4)
  launch_one: resident grid, 256 x blocks per CU          test_four_wave_tiles[*] (5-8: grid = tiles), test_resident_grid_walks[*]
  choose_tile_order / tile_origin: xg, xrows              test_xcd_orders[*]
  launch_gemm: chunked K sum, cut tail, row0              test_chunked_k_sum[*], test_xcd_orders[chunked-f32]
  splitk_finish_kernel (out + row0 * Cout)                test_chunked_k_sum[*], test_split_k[*]
  launch_gemm: split_k > 1                                test_split_k[*], test_split_k_pair[*]
  rn_conv_wide_launch, rn_conv_strip_launch               test_wide_tiles_and_strip[*]
  choose: the wide / strip / 4-wave rules, candidate 0    test_own_choice[*]
  chain_launch (rn_chain.hip)                             test_chain[*]
  stem_pool_launch: seg_len, segs (rn_stem.hip)           test_fused_stem[*]
  GemmParams::out_nchw                                    test_nchw_output_of_the_transposing_route

Every test prints one line of figures (launches, the largest share of its value bound any launch used); the
lines of the MI355X run are in profiles/schedules/README.md."""
import numpy as np
import pytest

import bf16_ref as BR
import resnet_c_amd as R
import views as V
from resnet_c_amd import _lib as L
from resnet_c_amd import ops
from test_ops_gpu import assert_close

pytestmark = pytest.mark.gpu

F32, BF16 = L.RN_DTYPE_F32, L.RN_DTYPE_BF16
TYPES = {"f32": (F32, F32), "bf16": (BF16, BF16), "bf16_f32": (BF16, F32)}
rb = ops.bf16_round


def rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def bn_consts(C, seed):
    g = np.random.default_rng(seed)
    return g.random(C, dtype=np.float32) + np.float32(0.5), g.standard_normal(C, dtype=np.float32)


class schedule:
    """conv tile candidate, XCD groups and split-K for the block; the dispatcher's own choices afterwards"""

    def __init__(self, tile=0, xcd=0, split_k=0):
        self.tile, self.xcd, self.split_k = tile, xcd, split_k

    def __enter__(self):
        ctx = R.get_ctx()
        try:
            L.check(L.lib().rn_ctx_set_conv_tile(ctx.handle, self.tile), "rn_ctx_set_conv_tile", ctx.handle)
            ctx.set_xcd_groups(self.xcd)
            ctx.set_split_k(self.split_k)
        except Exception:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        ctx = R.get_ctx()
        L.lib().rn_ctx_set_conv_tile(ctx.handle, 0)
        ctx.set_xcd_groups(0)
        ctx.set_split_k(0)


class Figures:
    """launch count and the largest share of the value bound of one test, printed as one line"""

    def __init__(self, name):
        self.name, self.launches, self.share = name, 0, 0.0

    def values(self, got, ref, k, bf16_out, epilogue, what):
        """the project's bound for this element type; the share of it that the worst element used"""
        self.launches += 1
        if bf16_out:
            share = BR.assert_bf16_rounded(got, ref, k, what)["max_bound_used"]
        else:
            kt = k + (4 if epilogue else 0)
            assert_close(got, ref, kt)
            # eps_sum is assert_close's bound but for the 1e-6 that assert_close adds to max|ref|: a share, not a check
            share = float(np.abs(got - ref).max()) / BR.eps_sum(ref, kt)
        self.share = max(self.share, share)

    def same(self, got, first, what):
        assert got.shape == first.shape and np.array_equal(got, first), f"{what}: other bits than the first schedule"

    def done(self):
        print(f"\nschedules: {self.name}: {self.launches} launches, largest share of the value bound {self.share:.3f}")


def launches_of(fn):
    """fn's result and the kernel launches it issued on the shared context (rn_ctx_launch_count)"""
    ctx, lib = R.get_ctx(), L.lib()
    n0 = int(lib.rn_ctx_launch_count(ctx.handle))
    out = fn()
    return out, int(lib.rn_ctx_launch_count(ctx.handle)) - n0


_PLAIN = {}


def plain_launches(dt_in, dt_out):
    """What V.run_conv_dt issues when the contraction is ONE kernel (packer included): a 64 -> 64 channel 1x1
    layer on 8 rows, K far below the chunked sum, no split.  A launch whose tail was cut, or whose K loop was
    split, issues exactly one more: the finishing kernel."""
    if (dt_in, dt_out) not in _PLAIN:
        x, w = rnd((1, 64, 2, 4), 1), rnd((64, 64, 1, 1), 2) / np.float32(8)
        with schedule():
            _, n = launches_of(lambda: V.run_conv_dt(x, w, 1, 0, None, None, None, False, dt_in, dt_out))
        _PLAIN[(dt_in, dt_out)] = n
    return _PLAIN[(dt_in, dt_out)]


def conv_operands(case, seed, dt_in):
    """x, w (bf16-rounded when the kernel reads bf16: the operands as it sees them), scale, shift, fp32 residual"""
    B, Cin, Cout, H, W, k, s, p = case
    x, w = rnd((B, Cin, H, W), seed), rnd((Cout, Cin, k, k), seed + 1) / np.float32(np.sqrt(Cin * k * k))
    if dt_in == BF16:
        x, w = rb(x), rb(w)
    sc, sh = bn_consts(Cout, seed + 2)
    res = rnd((B, Cout, V.out_size(H, k, s, p), V.out_size(W, k, s, p)), seed + 3)
    return x, w, sc, sh, res


def conv_reference(x, w, s, p, sc, sh, res, relu, dt_out, what):
    r = None if res is None else (rb(res) if dt_out == BF16 else res)
    ref = BR.epilogue64(BR.conv64(x, w, s, p), sc, sh, r, relu)
    V.assert_no_poison(ref, dt_out == BF16, what)
    return ref


# ---- 1. the 4-wave tiles ------------------------------------------------------------------------------------
# launch_gemm, conv_tile 1..8: tiles 128x128, 128x64, 64x128, 64x64, one block per tile (1-4) or the resident
# grid (5-8; here fewer tiles than CU slots, so a grid of one block per tile again).  722 = 2 x 19 x 19 rows:
# 5 x 128 + 82 and 11 x 64 + 18, ragged for both tile heights; Cout = 72 = 64 + 8: ragged for both tile widths
# and % 8 == 0 (whole 16-byte bf16 stores).  Cin = 64: one bf16 K tile per tap, two fp32 ones.  K = 576 / 64:
# below the chunked sum (nk >= 32).
TILE_CASES = {"3x3": (2, 64, 72, 19, 19, 3, 1, 1), "1x1s2": (2, 64, 72, 37, 37, 1, 2, 0)}


@pytest.mark.parametrize("epilogue", [True, False], ids=["epilogue", "raw"])
@pytest.mark.parametrize("types", sorted(TYPES))
@pytest.mark.parametrize("name", sorted(TILE_CASES))
def test_four_wave_tiles(name, types, epilogue):
    case = TILE_CASES[name]
    B, Cin, Cout, H, W, k, s, p = case
    dt_in, dt_out = TYPES[types]
    x, w, sc, sh, res = conv_operands(case, 100 + sum(case), dt_in)
    if not epilogue:
        sc = sh = res = None
    ref = conv_reference(x, w, s, p, sc, sh, res, epilogue, dt_out, name)
    fig, first = Figures(f"test_four_wave_tiles[{name}-{types}-{'epilogue' if epilogue else 'raw'}]"), None
    for cand in range(1, 9):
        with schedule(tile=cand):
            got = V.run_conv_dt(x, w, s, p, sc, sh, res, epilogue, dt_in, dt_out)
        what = f"{name} {types} candidate {cand}"
        fig.values(got, ref, Cin * k * k, dt_out == BF16, epilogue, what)
        first = got if first is None else first
        fig.same(got, first, what)
    fig.done()


# ---- 2. the resident grid really walking ----------------------------------------------------------------------
# launch_one caps the grid at 256 CUs x the blocks per CU of the instantiation; __launch_bounds__ of
# conv_gemm_kernel gives 2 (128x128), 3 (128x64, 64x128), 4 (64x64), so a block walks more than one tile only
# past 512 / 768 / 768 / 1024 tiles of the candidate's own size.  1x1, Cout = 72 (one N tile of 128, two of 64),
# 70007 = 7 x 73 x 137 rows (odd: ragged for every tile height): 547 / 1094 / 1094 / 2188 tiles.  The occupancy
# query may allow more blocks per CU than the bound, and the context exposes no grid size (rn_ctx_launch_count
# counts launches); every block of the contraction kernel writes debug-stamp slot 0 when it starts
# (rn_ctx_set_debug_stamps, 16 slots per block), so the number of blocks that wrote it IS the grid: equal to the
# tile count for candidates 1-4, required to be smaller for 5-8.
@pytest.mark.parametrize("types", ["f32", "bf16"])
def test_resident_grid_walks(types):
    from resnet_c_amd.tensor import _DeviceBuffer
    dt_in, dt_out = TYPES[types]
    Cin = 32 if dt_in == F32 else 64       # one K tile: the shortest K loop, the walk is what is tested
    case = (7, Cin, 72, 73, 137, 1, 1, 0)
    B, _, Cout, H, W, k, s, p = case
    M = B * H * W
    x, w, sc, sh, _ = conv_operands(case, 200 + sum(case), dt_in)
    ref = conv_reference(x, w, s, p, sc, sh, None, True, dt_out, "resident")
    ctx, lib = R.get_ctx(), L.lib()
    nblk = -(-M // 64) * -(-Cout // 64)     # the most blocks any candidate launches: one per 64 x 64 tile
    stamps = _DeviceBuffer(ctx, nblk * 16 * 8)
    tiles_of = {c: -(-M // bm) * -(-Cout // bn) for c, (bm, bn) in enumerate(((128, 128), (128, 64), (64, 128), (64, 64)), 1)}
    fig, first = Figures(f"test_resident_grid_walks[{types}]"), None
    try:
        for cand in range(1, 9):
            tiles = tiles_of[(cand - 1) % 4 + 1]
            assert tiles <= nblk
            L.check(lib.rn_memset(ctx.handle, stamps.ptr, 0, nblk * 128), "memset", ctx.handle)
            with schedule(tile=cand):
                L.check(lib.rn_ctx_set_debug_stamps(ctx.handle, stamps.ptr), "stamps", ctx.handle)
                got = V.run_conv_dt(x, w, s, p, sc, sh, None, True, dt_in, dt_out)
                L.check(lib.rn_ctx_set_debug_stamps(ctx.handle, None), "stamps", ctx.handle)
            slots = np.zeros(nblk * 16, np.uint64)
            L.check(lib.rn_memcpy_d2h(ctx.handle, slots.ctypes.data, stamps.ptr, slots.nbytes), "d2h", ctx.handle)
            grid = int((slots.reshape(nblk, 16)[:, 0] != 0).sum())
            what = f"resident {types} candidate {cand}: grid {grid}, {tiles} tiles"
            print(f"\n  {what}")
            if cand <= 4:
                assert grid == tiles, what
            else:
                assert 0 < grid < tiles, what + ": the resident grid does not walk at this size"
            fig.values(got, ref, Cin, dt_out == BF16, True, what)
            first = got if first is None else first
            fig.same(got, first, what)
    finally:
        lib.rn_ctx_set_debug_stamps(ctx.handle, None)
    fig.done()


# ---- 3. the XCD tile orders -----------------------------------------------------------------------------------
# choose_tile_order remaps when tiles_n >= 2 and the remapped tiles are at least 8 * tiles_n; forced groups that
# do not divide tiles_n are halved until they do.  1190 = 2 x 17 x 35 rows: 9 M panels of 128 plus a ragged tenth
# (38 rows), 18 of 64 plus the same.
#   grouped  Cout = 500: 8 N tiles of 64 (the last 52 wide) or 4 of 128 -- 152 / 80 / 76 / 40 tiles, every group
#            count applies (8 only to the 64-wide tiles); 76 tiles: 4 left over when dealt to 8 XCDs
#   odd      Cout = 320: 5 N tiles of 64, 3 of 128: no grouping possible, the deal to the XCDs alone (95 = 8 x 11 + 7)
#   chunked  fp32, 3x3, Cin = 128: K = 1152 >= 1024; 9000 = 5 x 40 x 45 rows x Cout 128 on 64 x 64 tiles: 141 M
#            panels (the last 40 rows) x 2 = 282 tiles = 256 remapped (>= 16) + 26 cut into 6 chunks behind them;
#            the 128-row candidates have 142 tiles, all cut, and 64 x 128 has tiles_n = 1: no remap
XCD_CASES = {"grouped-f32": ((2, 64, 500, 17, 35, 1, 1, 0), "f32"), "grouped-bf16": ((2, 64, 500, 17, 35, 1, 1, 0), "bf16"),
             "odd-f32": ((2, 64, 320, 17, 35, 1, 1, 0), "f32"), "chunked-f32": ((5, 128, 128, 40, 45, 3, 1, 1), "f32")}


@pytest.mark.parametrize("name", sorted(XCD_CASES))
def test_xcd_orders(name):
    case, types = XCD_CASES[name]
    B, Cin, Cout, H, W, k, s, p = case
    dt_in, dt_out = TYPES[types]
    x, w, sc, sh, res = conv_operands(case, 300 + sum(case), dt_in)
    ref = conv_reference(x, w, s, p, sc, sh, res, True, dt_out, name)
    fig, first = Figures(f"test_xcd_orders[{name}]"), None
    for groups in (1, 0, 2, 4, 8):        # 1: the logical order first
        for cand in range(1, 9):
            with schedule(tile=cand, xcd=groups):
                got, n = launches_of(lambda: V.run_conv_dt(x, w, s, p, sc, sh, res, True, dt_in, dt_out))
            what = f"{name} groups {groups} candidate {cand}"
            # the chunked case cuts a tail on every candidate (26 of 282, all 142, all 141 tiles): the finishing kernel ran
            assert n == plain_launches(dt_in, dt_out) + (1 if name.startswith("chunked") else 0), f"{what}: {n} launches"
            fig.values(got, ref, Cin * k * k, dt_out == BF16, True, what)
            first = got if first is None else first
            fig.same(got, first, what)
    fig.done()


# ---- 4. the chunked K sum -------------------------------------------------------------------------------------
# launch_gemm: fp32 -> fp32 and bf16 -> fp32 with nk >= 32 (fp32 K >= 1024, bf16 K >= 2048) and Cout % 4 == 0 add
# their products in chunks (nk = 32: 8 chunks of 4 K tiles).  tail = total % 256 (all of them up to 256 tiles),
# less tail % tiles_n; the tail is cut into (tile, chunk) pieces when ceil(tail * 8 / 256) < 8, i.e. up to 224
# tiles; the pieces go to a workspace addressed through a base moved back by row0 rows, and
# splitk_finish_kernel writes out + row0 * Cout (residual + row0 * Cout) with plain stores.  1x1, so a row's
# value depends on its own input row only.  On 64 x 64 tiles (the only tile of bf16 -> fp32):
#   all-tail   98 rows x Cout 72: 4 tiles, everything through the workspace and the finishing kernel, row0 = 0
#   cut-tail   4200 = 8 x 25 x 21 rows x Cout 256: 66 M panels x 4 = 264 tiles = 256 whole + 8 cut (two panels,
#              the last 40 rows); row0 = 4096
#   ragged-n   3360 = 8 x 20 x 21 rows x Cout 264: 53 panels x 5 N tiles (the last 8 wide) = 265; 265 % 256 = 9
#              is no whole row of tiles: 5 are cut (the last panel, 32 rows), 260 whole; row0 = 3328
# The other candidates cut elsewhere (128-row tiles: 132 / 135 tiles, all cut) -- the same bits.  The first image
# sits in whole tiles of the large launches and is all cut in a launch of its own: whole against cut.
CHUNK_CASES = {"all-tail": ((2, 72, 7, 7), range(0, 9)), "cut-tail": ((8, 256, 25, 21), (4, 0, 2, 8)),
               "ragged-n": ((8, 264, 20, 21), (4, 0, 2, 8))}


@pytest.mark.parametrize("types", ["f32", "bf16_f32"])
@pytest.mark.parametrize("name", sorted(CHUNK_CASES))
def test_chunked_k_sum(name, types):
    (B, Cout, H, W), cands = CHUNK_CASES[name]
    dt_in, dt_out = TYPES[types]
    Cin = 1024 if dt_in == F32 else 2048
    case = (B, Cin, Cout, H, W, 1, 1, 0)
    x, w, sc, sh, res = conv_operands(case, 400 + sum(case), dt_in)
    ref = conv_reference(x, w, 1, 0, sc, sh, res, True, dt_out, name)
    fig, first = Figures(f"test_chunked_k_sum[{name}-{types}]"), None
    # every candidate cuts a tail at these sizes (above), so every launch is followed by the finishing kernel: one
    # launch more than a contraction that is one kernel.  Pins the geometry against a change of launch_gemm's constants.
    cut = plain_launches(dt_in, dt_out) + 1
    for cand in cands:
        with schedule(tile=cand):
            got, n = launches_of(lambda: V.run_conv_dt(x, w, 1, 0, sc, sh, res, True, dt_in, dt_out))
        what = f"chunked {name} {types} candidate {cand}"
        assert n == cut, f"{what}: {n} launches, {cut} with a cut tail: splitk_finish_kernel did not run"
        fig.values(got, ref, Cin, False, True, what)
        first = got if first is None else first
        fig.same(got, first, what)
    if B > 2:      # the first image alone: at most 224 tiles, every one of them cut
        with schedule(tile=4):
            alone, n = launches_of(lambda: V.run_conv_dt(x[:1], w, 1, 0, sc, sh, res[:1], True, dt_in, dt_out))
        assert n == cut, f"chunked {name} {types} first image alone: {n} launches, {cut} with a cut tail"
        fig.values(alone, ref[:1], Cin, False, True, f"chunked {name} {types} first image alone")
        fig.same(alone, first[:1], f"chunked {name} {types}: whole tiles against cut ones")
    fig.done()


# ---- 5. split-K -----------------------------------------------------------------------------------------------
# launch_gemm with rn_ctx_set_split_k(16): fewer than 512 tiles, nk >= 8, Cout % 4 == 0.  S = min(ceil(1024 /
# tiles), 16, nk / 4), each split ceil(nk / S) K tiles; every split writes a raw M x Cout slice and
# splitk_finish_kernel adds them and runs the epilogue.  722 rows x Cout 72 (24 tiles of 64 x 64):
#   3x3, Cin = 64    fp32 nk = 18: S = 4 of 5, 5, 5, 3 K tiles; bf16 nk = 9: S = 2 of 5, 4 -- the last split shorter
#   1x1, Cin = 512   fp32 nk = 16: S = 4 of 4; bf16 nk = 8: S = 2 of 4 -- nk divisible by the split count
# Split-K adds in another order than the unsplit launch: within the bound and the same bits on a second run, no
# more.  That the launch was split shows in rn_ctx_launch_count: one launch (the finishing kernel) more.
SPLIT_CASES = {"3x3-short-last": (2, 64, 72, 19, 19, 3, 1, 1), "1x1-divisible": (2, 512, 72, 19, 19, 1, 1, 0)}


@pytest.mark.parametrize("types", ["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(SPLIT_CASES))
def test_split_k(name, types):
    case = SPLIT_CASES[name]
    B, Cin, Cout, H, W, k, s, p = case
    dt_in, dt_out = TYPES[types]
    x, w, sc, sh, res = conv_operands(case, 500 + sum(case), dt_in)
    ref = conv_reference(x, w, s, p, sc, sh, res, True, dt_out, name)
    raw_ref = conv_reference(x, w, s, p, None, None, None, False, dt_out, name + " raw")
    fig = Figures(f"test_split_k[{name}-{types}]")
    for cand in (0, 4):
        with schedule(tile=cand):
            _, plain = launches_of(lambda: V.run_conv_dt(x, w, s, p, sc, sh, res, True, dt_in, dt_out))
        with schedule(tile=cand, split_k=16):
            got, split = launches_of(lambda: V.run_conv_dt(x, w, s, p, sc, sh, res, True, dt_in, dt_out))
            again = V.run_conv_dt(x, w, s, p, sc, sh, res, True, dt_in, dt_out)
            raw = V.run_conv_dt(x, w, s, p, None, None, None, False, dt_in, dt_out)
        what = f"split-K {name} {types} candidate {cand}"
        assert split == plain + 1, f"{what}: {split} launches against {plain} unsplit: the K loop was not split"
        fig.values(got, ref, Cin * k * k, dt_out == BF16, True, what)
        fig.values(raw, raw_ref, Cin * k * k, dt_out == BF16, False, what + " raw")
        fig.same(again, got, what + " (second run)")
    fig.done()


# the fp32 pair: K = Cin + Cin2.  160 + 128 channels: nk = 9, S = 2 of 5 and 4 K tiles; 128 + 128: nk = 8, 4 and 4.
@pytest.mark.parametrize("Cin", [160, 128], ids=["short-last", "divisible"])
def test_split_k_pair(Cin):
    B, Cout, H, W, Cin2 = 2, 72, 19, 19, 128
    K = Cin + Cin2
    seed = 550 + Cin
    t, x2 = rnd((B, Cin, H, W), seed), rnd((B, Cin2, 2 * H - 1, 2 * W - 1), seed + 1)
    w, w2 = rnd((Cout, Cin, 1, 1), seed + 2) / np.float32(np.sqrt(K)), rnd((Cout, Cin2, 1, 1), seed + 3) / np.float32(np.sqrt(K))
    sc1, shift = bn_consts(Cout, seed + 4)
    sc2, _ = bn_consts(Cout, seed + 5)
    res = rnd((B, Cout, H, W), seed + 6)
    # the packer folds the scales into the panel in fp32: the kernel multiplies fl32(w * scale)
    y64 = BR.conv64(t, w * sc1[:, None, None, None], 1, 0) + BR.conv64(x2, w2 * sc2[:, None, None, None], 2, 0)
    ref = BR.epilogue64(y64, None, shift, res, True)
    fig = Figures(f"test_split_k_pair[{Cin}+{Cin2}]")
    run = lambda: V.run_conv_pair_dt(t, w, x2, w2, 1, 0, 2, sc1, sc2, shift, res, True, F32)
    for cand in (0, 4):
        with schedule(tile=cand):
            plain_got, plain = launches_of(run)
        with schedule(tile=cand, split_k=16):
            got, split = launches_of(run)
            again = run()
        what = f"split-K pair {Cin}+{Cin2} candidate {cand}"
        assert split == plain + 1, f"{what}: {split} launches against {plain} unsplit: the K loop was not split"
        fig.values(plain_got, ref, K, False, True, what + " unsplit")
        fig.values(got, ref, K, False, True, what)
        fig.same(again, got, what + " (second run)")
    fig.done()


# ---- 6. the wide tiles and the strip kernel (bf16 -> bf16) ------------------------------------------------------
# Candidates 9 .. rn_conv_tile_candidates(): the wide tiles 256x256, 256x128, 128x256, 256x64, 224x256, 128x128
# (rn_conv_wide_eligible: whole channel segments, Cout % 8 == 0) and last the strip kernel
# (rn_conv_strip_eligible: 3x3 / stride 1 / pad 1, 64 -> 64 with W + 3 <= 64 or 128 -> 128 with W + 3 <= 32).
# A forced candidate whose predicate fails runs the dispatcher's own choice -- still a launch on a poisoned
# output, but no coverage of the candidate: which kernel ran is read from the debug stamps of every launch (the
# strip kernels alone write slot 10, the 4-wave kernel alone slot 7, every kernel slot 0 once per block) and
# asserted.  Candidates 9-14 are real wide-tile launches in every case below (also on the 64- and 128-channel
# strip shapes); candidate 15 is the strip kernel in the strip* cases only and a 4-wave tile in the other three.
# 722 rows: 2 x 256 + 210, 3 x 224 + 50, 5 x 128 + 82; Cout = 264 = 256 + 8 = 2 x 128 + 8 = 4 x 64 + 8.
#   3x3      Cin = 128: two channel segments per tap
#   1x1s2    stride 2 on 37 x 37 -> 19 x 19
#   pair     the two-source form on every wide tile (64 + 64 channels, the second source at stride 2)
#   strip*   3 images of 7 x 9 and 4 one-row images of 1 x 9: 189 / 36 rows, image boundaries inside a strip
WIDE_CASES = {"3x3": (2, 128, 264, 19, 19, 3, 1, 1), "1x1s2": (2, 64, 264, 37, 37, 1, 2, 0), "pair": None,
              "strip64": (3, 64, 64, 7, 9, 3, 1, 1), "strip64-row": (4, 64, 64, 1, 9, 3, 1, 1),
              "strip128": (3, 128, 128, 7, 9, 3, 1, 1), "strip128-row": (4, 128, 128, 1, 9, 3, 1, 1)}


@pytest.mark.parametrize("name", sorted(WIDE_CASES))
def test_wide_tiles_and_strip(name):
    from resnet_c_amd.tensor import _DeviceBuffer
    ncand = L.lib().rn_conv_tile_candidates()
    assert ncand == 15, "6 wide tiles + the strip kernel behind the 8 four-wave candidates"
    fig, first = Figures(f"test_wide_tiles_and_strip[{name}]"), None
    if name == "pair":
        B, Cin, Cout, H, W, Cin2 = 2, 64, 264, 19, 19, 64
        K, seed = Cin + Cin2, 640
        t, x2 = rb(rnd((B, Cin, H, W), seed)), rb(rnd((B, Cin2, 2 * H - 1, 2 * W - 1), seed + 1))
        w, w2 = rnd((Cout, Cin, 1, 1), seed + 2) / np.float32(np.sqrt(K)), rnd((Cout, Cin2, 1, 1), seed + 3) / np.float32(np.sqrt(K))
        sc1, shift = bn_consts(Cout, seed + 4)
        sc2, _ = bn_consts(Cout, seed + 5)
        res = rnd((B, Cout, H, W), seed + 6)
        # the scales are folded into the packed panel: the kernel multiplies bf16(fl32(w * scale))
        y64 = BR.conv64(t, rb(w * sc1[:, None, None, None]), 1, 0) + BR.conv64(x2, rb(w2 * sc2[:, None, None, None]), 2, 0)
        ref = BR.epilogue64(y64, None, shift, rb(res), True)
        run = lambda: V.run_conv_pair_dt(t, w, x2, w2, 1, 0, 2, sc1, sc2, shift, res, True, BF16)
    else:
        case = WIDE_CASES[name]
        B, Cin, Cout, H, W, k, s, p = case
        K = Cin * k * k
        x, w, sc, sh, res = conv_operands(case, 600 + sum(case), BF16)
        ref = conv_reference(x, w, s, p, sc, sh, res, True, BF16, name)
        run = lambda: V.run_conv_dt(x, w, s, p, sc, sh, res, True, BF16, BF16)
    ctx, lib = R.get_ctx(), L.lib()
    M = int(np.prod(ref.shape)) // Cout      # output rows
    nblk = 1 << 12      # room for the grid of any kernel that could run here (at most 60 tiles of 64 x 64)
    stamps = _DeviceBuffer(ctx, nblk * 16 * 8)
    wide_tiles = ((256, 256), (256, 128), (128, 256), (256, 64), (224, 256), (128, 128))     # kTiles of rn_conv_wide.hip
    ran = []
    for cand in [4] + list(range(9, ncand + 1)):
        what = f"wide {name} candidate {cand}"
        L.check(lib.rn_memset(ctx.handle, stamps.ptr, 0, nblk * 128), "memset", ctx.handle)
        with schedule(tile=cand):
            try:
                L.check(lib.rn_ctx_set_debug_stamps(ctx.handle, stamps.ptr), "stamps", ctx.handle)
                got = run()
            finally:
                lib.rn_ctx_set_debug_stamps(ctx.handle, None)
        slots = np.zeros(nblk * 16, np.uint64)
        L.check(lib.rn_memcpy_d2h(ctx.handle, slots.ctypes.data, stamps.ptr, slots.nbytes), "d2h", ctx.handle)
        wrote = slots.reshape(nblk, 16) != 0
        kernel = "strip" if wrote[:, 10].any() else "tile" if wrote[:, 7].any() else "wide"
        grid = int(wrote[:, 0].sum())
        ran.append(f"{cand}:{kernel}")
        if cand == 4:
            assert kernel == "tile" and grid == -(-M // 64) * -(-Cout // 64), f"{what}: {kernel}, grid {grid}"
        elif cand < ncand:      # a wide tile, one block per tile of ITS size: the forced candidate did not fall back
            bm, bn = wide_tiles[cand - 9]
            assert kernel == "wide" and grid == -(-M // bm) * -(-Cout // bn), f"{what}: {kernel}, grid {grid}"
        else:                   # the strip kernel where its predicate holds, the dispatcher's own 4-wave tile elsewhere
            assert kernel == ("strip" if name.startswith("strip") else "tile"), f"{what}: {kernel}"
        fig.values(got, ref, K, True, True, what)
        first = got if first is None else first
        fig.same(got, first, what + " (against candidate 4)")
    print(f"\n  test_wide_tiles_and_strip[{name}]: kernel per candidate: {' '.join(ran)}")
    fig.done()


# ---- 6b. the dispatcher's own choice between the wide, strip and 4-wave kernels (bf16 -> bf16, candidate 0) ------
# choose (rn_conv.hip) with nothing forced.  The smallest shapes at which each rule flips, from its constants:
#   wide       1x1, Cin = 512 (nk = 8 K tiles of 64), Cout = 256, 4 x 64 x 64 = 16384 rows.  Cost = ceil(tiles / 256) x
#              tile area / eff_wide: 128x128 256 tiles, 16384 / 0.55 = 29789; 256x64 256 tiles, 16384 / 0.50 = 32768;
#              256x128 and 128x256 128 tiles, 32768 / 0.80 = 40960; 256x256 (64 tiles) and 224x256 (74) have fewer
#              than 128 tiles.  So the 128x128 wide tile, one block per tile: grid 256
#   not-wide   the same with Cin = 448: nk = 7 < 8, no wide tile is considered -- a 4-wave tile
#   strip      3x3 / 1 / 1, 64 -> 64, 16 x 128 x 32 = 65536 rows = 256 * 256, W + 3 = 35 <= 64: the strip kernel
#   not-strip  the same with 15 images: 61440 rows < 256 * 256, and Cout < 128 rules the wide tiles out -- a 4-wave tile
# Which kernel ran is read from the debug stamps as in test_wide_tiles_and_strip.  One launch per case.
OWN_CASES = {"wide": ((4, 512, 256, 64, 64, 1, 1, 0), "wide", 256), "not-wide": ((4, 448, 256, 64, 64, 1, 1, 0), "tile", None),
             "strip": ((16, 64, 64, 128, 32, 3, 1, 1), "strip", None), "not-strip": ((15, 64, 64, 128, 32, 3, 1, 1), "tile", None)}


@pytest.mark.parametrize("name", sorted(OWN_CASES))
def test_own_choice(name):
    from resnet_c_amd.tensor import _DeviceBuffer
    case, want_kernel, want_grid = OWN_CASES[name]
    B, Cin, Cout, H, W, k, s, p = case
    K = Cin * k * k
    x, w, sc, sh, res = conv_operands(case, 650 + sum(case), BF16)
    ref = conv_reference(x, w, s, p, sc, sh, res, True, BF16, name)
    ctx, lib = R.get_ctx(), L.lib()
    M = int(np.prod(ref.shape)) // Cout
    nblk = -(-M // 64) * -(-Cout // 64)      # the most blocks any kernel launches here: one per 64 x 64 tile
    stamps = _DeviceBuffer(ctx, nblk * 16 * 8)
    L.check(lib.rn_memset(ctx.handle, stamps.ptr, 0, nblk * 128), "memset", ctx.handle)
    with schedule():
        try:
            L.check(lib.rn_ctx_set_debug_stamps(ctx.handle, stamps.ptr), "stamps", ctx.handle)
            got = V.run_conv_dt(x, w, s, p, sc, sh, res, True, BF16, BF16)
        finally:
            lib.rn_ctx_set_debug_stamps(ctx.handle, None)
    slots = np.zeros(nblk * 16, np.uint64)
    L.check(lib.rn_memcpy_d2h(ctx.handle, slots.ctypes.data, stamps.ptr, slots.nbytes), "d2h", ctx.handle)
    wrote = slots.reshape(nblk, 16) != 0
    kernel = "strip" if wrote[:, 10].any() else "tile" if wrote[:, 7].any() else "wide"
    grid = int(wrote[:, 0].sum())
    what = f"own choice {name}: {kernel} kernel, grid {grid}"
    print(f"\n  test_own_choice[{name}]: {M} rows, K = {K}: {kernel} kernel, grid {grid}")
    assert kernel == want_kernel and grid > 0, f"{what}; expected the {want_kernel} kernel"
    assert want_grid is None or grid == want_grid, f"{what}; expected a grid of {want_grid}"
    fig = Figures(f"test_own_choice[{name}]")
    fig.values(got, ref, K, True, True, what)
    fig.done()


# ---- 7. the chain kernels -------------------------------------------------------------------------------------
# chain_launch: (mid, channels, next_mid) = (64, 256, 64 | 128) on 64-row steps, bf16 also (128, 512, 128) on
# 32-row steps; the pair form 64 + 64 -> 256 -> 64 (bf16: | 128).  189 = 3 x 9 x 7 rows: 2 x 64 + 61 = 5 x 32 + 29;
# 585 = 5 x 13 x 9 rows: 9 x 64 + 9 = 18 x 32 + 9 -- a ragged last step of either walk, one step and several.
# y AND t1 are outputs.  Bit for bit the two separate launches, run on poisoned outputs as well.
CHAINS = [("f32", 64, 64, False), ("f32", 64, 128, False), ("f32", 64, 64, True),
          ("bf16", 64, 64, False), ("bf16", 64, 128, False), ("bf16", 128, 128, False), ("bf16", 64, 64, True), ("bf16", 64, 128, True)]


@pytest.mark.parametrize("types,MID,N1,pair", CHAINS, ids=[f"{t}-{m}-{n}{'-pair' if pr else ''}" for t, m, n, pr in CHAINS])
def test_chain(types, MID, N1, pair):
    dt = TYPES[types][0]
    bf, C = dt == BF16, 4 * MID
    r = rb if bf else (lambda a: a)
    fig = Figures(f"test_chain[{types}-{MID}-{N1}{'-pair' if pair else ''}]")
    for (B, H, W) in ((3, 9, 7), (5, 13, 9)):
        seed = 700 + B * H * W + MID + N1
        t2, x = r(rnd((B, MID, H, W), seed)), r(rnd((B, 64 if pair else C, H, W), seed + 1))
        K3 = MID + (64 if pair else 0)
        w3, w1 = rnd((C, MID, 1, 1), seed + 2) / np.float32(np.sqrt(K3)), r(rnd((N1, C, 1, 1), seed + 3) / np.float32(np.sqrt(C)))
        wd = rnd((C, 64, 1, 1), seed + 4) / np.float32(np.sqrt(K3))
        sc3, sh3 = bn_consts(C, seed + 5)
        scd, _ = bn_consts(C, seed + 6)
        sc1, sh1 = bn_consts(N1, seed + 7)
        what = f"chain {types} {MID}->{C}->{N1} pair={pair} {B * H * W} rows"
        if pair:     # scales folded into the panel (fp32 product, then the panel's element type)
            y64 = BR.conv64(t2, r(w3 * sc3[:, None, None, None])) + BR.conv64(x, r(wd * scd[:, None, None, None]))
            ref_y = BR.epilogue64(y64, None, sh3, None, True)
            got_y, got_t1 = V.run_chain_dt(t2, x, w3, sc3, sh3, w1, sc1, sh1, dt, pair_w=wd, pair_scale=scd)
            sep_y = V.run_conv_pair_dt(t2, w3, x, wd, 1, 0, 1, sc3, scd, sh3, None, True, dt)
        else:
            w3 = r(w3)
            ref_y = BR.epilogue64(BR.conv64(t2, w3), sc3, sh3, x, True)
            got_y, got_t1 = V.run_chain_dt(t2, x, w3, sc3, sh3, w1, sc1, sh1, dt)
            sep_y = V.run_conv_dt(t2, w3, 1, 0, sc3, sh3, x, True, dt, dt)
        sep_t1 = V.run_conv_dt(sep_y, w1, 1, 0, sc1, sh1, None, True, dt, dt)
        fig.values(got_y, ref_y, K3, bf, True, what + ": y")
        # t1's operand is the y that was written (for bf16 already rounded): y is not its own reference
        ref_t1 = BR.epilogue64(BR.conv64(got_y, w1), sc1, sh1, None, True)
        fig.values(got_t1, ref_t1, C, bf, True, what + ": t1")
        fig.same(got_y, sep_y, what + ": y against the separate launch")
        fig.same(got_t1, sep_t1, what + ": t1 against the separate launches")
    fig.done()


# ---- 8. the fused stem ----------------------------------------------------------------------------------------
# stem_pool_launch: conv output width a multiple of 8 (8 is the narrowest: W = 16), the NCHW forms W % 4 == 0,
# the padded bf16 form an even padded width.  A block walks seg_len items (pairs of pooled rows) of an image;
# rn_ctx_set_stem_items forces seg_len.
#   (2, 3, 26, 16)  conv 13 x 8, pooled 7 x 4: 4 items, the last one a single pooled row whose window hangs over the
#                   bottom edge; not square
#   (3, 1, 21, 32)  conv 11 x 16, pooled 6 x 8: 3 items, the last pooled row's window one conv row short; one channel
# items 1, 2, 3, 5, 100 and 0 (the launch's own choice), the values of
# test_fused_stem_segments_change_blocks_not_results; padded and NCHW input, and in fp32 the form that also
# writes the stem tensor: both outputs checked.
@pytest.mark.parametrize("types", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 3, 26, 16), (3, 1, 21, 32)], ids=["26x16", "21x32"])
def test_fused_stem(shape, types):
    B, Cin, H, W = shape
    dt = TYPES[types][0]
    bf, K = dt == BF16, Cin * 49
    seed = 800 + sum(shape)
    x, w = rnd(shape, seed), rnd((64, Cin, 7, 7), seed + 1) / np.float32(np.sqrt(K))
    if bf:
        x, w = rb(x), rb(w)
    sc, sh = bn_consts(64, seed + 2)
    sh = sh * np.float32(0.3)
    ref_y = BR.epilogue64(BR.conv64(x, w, 2, 3), sc, sh, None, True)
    ref = BR.maxpool64(ref_y, 3, 2, 1)     # (rounding is monotone: the maximum of the rounded values is the rounded maximum)
    ctx, lib = R.get_ctx(), L.lib()
    fig, first = Figures(f"test_fused_stem[{shape[2]}x{shape[3]}-{types}]"), None
    try:
        for items in (1, 2, 3, 5, 100, 0):
            L.check(lib.rn_ctx_set_stem_items(ctx.handle, items), "rn_ctx_set_stem_items", ctx.handle)
            for form in ("padded", "nchw") + (() if bf else ("y",)):
                what = f"stem {shape} {types} items {items} {form}"
                got = V.run_stem_pool(form, x, w, sc, sh, dt)
                if form == "y":
                    got, y = got
                    fig.values(y, ref_y, K, False, True, what + ": stem tensor")
                    # the pooled tensor is the maximum of the very values that were written
                    assert np.array_equal(got, BR.maxpool64(y.astype(np.float64), 3, 2, 1)), what
                fig.values(got, ref, K, bf, True, what)
                first = got if first is None else first
                fig.same(got, first, what)
    finally:
        lib.rn_ctx_set_stem_items(ctx.handle, 0)
    fig.done()


# ---- 9. the NCHW output of the transposing route ----------------------------------------------------------------
# rn_conv2d_forward on NCHW tensors with rn_ctx_set_nchw_taps(0): a 3x3 layer is transposed to NHWC and the
# contraction's epilogue writes NCHW itself (GemmParams::out_nchw), quads of pixels per store.  Ho x Wo = 49 is no
# multiple of 4 (quads straddle the planes), 98 rows: ragged M; Cout = 72: ragged N.  No ReLU: the reference is
# checked for the fill pattern.
def test_nchw_output_of_the_transposing_route():
    case = (2, 32, 72, 7, 7, 3, 1, 1)
    B, Cin, Cout, H, W, k, s, p = case
    x, w, _, _, _ = conv_operands(case, 900, F32)
    ref = conv_reference(x, w, s, p, None, None, None, False, F32, "nchw out")
    fig, first = Figures("test_nchw_output_of_the_transposing_route"), None
    for cand in range(0, 9):
        with schedule(tile=cand):
            got = V.run_conv2d(x, w, s, p, "nchw", 0, {}, guard_bytes=V.contraction_guard(Cout * 4))
        what = f"nchw out candidate {cand}"
        fig.values(got, ref, Cin * k * k, False, False, what)
        first = got if first is None else first
        fig.same(got, first, what)
    fig.done()
