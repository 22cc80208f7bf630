"""Op entry points on offset views: pointers that are 4-byte but not 16-byte aligned, guard bands around
every operand (tests/views.py).

Nearly every entry point chooses its kernel by pointer alignment at run time.  Every other test of the
suite allocates each tensor on its own, page-aligned and followed by allocator slack, so it reaches the
"else" side of those decisions through the SHAPE only, and a store a few elements past a tensor lands
in slack.  Here every operand sits at +0 (the control: the aligned kernels' first guard-band check), +4,
+8 or +12 bytes from a 16-byte boundary, each operand on its own and all together, between 256-byte
guards that are compared byte for byte.

Expectations: bit-exact with the oracle / numpy, bit-equal to the aligned call, or within a bound of
test_ops_gpu.py (assert_close; the 2e-6 * sqrt(K) bound of test_nchw_route_writes_the_nhwc_routes_bits).
No tolerance of its own.  The alignment contract these tests pin is written down in include/rn_hip.h
("Alignment").

Decision (resnet.c_amd/csrc/)                   reached through the pointer by
  rn_eltwise.hip:325  relu, aligned16            test_relu_add[*]
  rn_eltwise.hip:341  add, three operands        test_relu_add[*]
  rn_eltwise.hip:370  batch-norm, NHWC float4    test_batchnorm[shape0-nhwc], [shape1-nhwc] (fixed / not fixed grid)
  rn_eltwise.hip:394  batch-norm, batch walk     test_batchnorm[shape3-nchw]; [shape4-nchw] is its N % 4 != 0 side
  rn_eltwise.hip:409  batch-norm, plane float4   test_batchnorm[shape5-nchw], [shape7-nchw]
  rn_pool.hip:450     fp32 pools, NHWC float4    test_pools[case0-nhwc], [case1-nhwc], [case4-nhwc]
  rn_pool.hip:474     fp32 max-pool, NCHW quads  test_pools[case0-nchw], [case3-nchw]
  rn_pool.hip:412     bf16 pools: refusal        test_16_byte_entry_points_refuse[pool_bf16_max], [pool_bf16_avg]
  rn_layout.hip:436   bordered image, bf16       test_bf16_bordered_image
  rn_layout.hip:453   bordered image, fp32       test_padded_images
  rn_layout.hip:482   both transposes            test_transposes[r64s16]
  rn_layout.hip:526   rn_nchw_to_nhwc_pad, 4     test_padded_images
  rn_conv.hip  gemm_eligible                     test_linear[*], test_conv_nhwc_epilogue[*]
  rn_conv.hip  epilogue_aligned16                test_conv_nhwc_epilogue[*] (scale / shift / residual), test_linear[*] (bias)
  rn_conv.hip  rn_conv2d_forward, 1x1 weight     test_conv2d_forward[case0-nchw-*], [case1-nchw-*]
  rn_conv.hip  rn_conv2d_forward, inp / out      test_conv2d_forward[*-nhwc-*], [case2-nchw-0] (out of the transposing route)
  rn_conv_nchw.hip:314  gathering form           test_conv2d_forward[case0-nchw-*]
  rn_conv.hip  bf16 / exact / pair refusals      test_16_byte_entry_points_refuse[conv_bf16], [conv_exact], [conv_pair]
  rn_stem.hip:545/560 refusals                   test_16_byte_entry_points_refuse[stem_pool], [stem_pool_nchw], [stem_conv_pool]
  rn_chain.hip:649    refusal                    test_16_byte_entry_points_refuse[chain_f32], [chain_bf16], [chain_pair_f32], [chain_pair_bf16]
  rn_defer.hip:259    fusable_conv               test_deferred_chain_on_views[inp], [out]; test_deferred_basic_block_on_views[x], [t1], [out]
  rn_defer.hip:447    residual of the fold       test_deferred_chain_on_views[other], test_deferred_basic_block_on_views[x]
  rn_defer.hip:505    fused stem launch          test_deferred_stem_on_views[inp], [pool_out]
"""
import ctypes

import numpy as np
import pytest

import views as V
from oracle import oracle as O
from resnet_c_amd import _lib as L
from resnet_c_amd import ops
from test_ops_gpu import assert_close

pytestmark = pytest.mark.gpu


def rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), what


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, 70001])
def test_relu_add(n):
    a, b = rnd((n,), n), rnd((n,), n + 1)
    a[::7] = -a[::7]
    want_relu, want_add = O.relu(a), O.add(a, b)
    for inplace in (True, False):
        for offs in V.offset_configs(("inp",) if inplace else ("inp", "out")):
            same(V.run_relu(a, offs, inplace), want_relu, f"relu n={n} inplace={inplace} {offs}")
        for offs in V.offset_configs(("inp1", "inp2") if inplace else ("inp1", "inp2", "out")):
            same(V.run_add(a, b, offs, inplace), want_add, f"add n={n} inplace={inplace} {offs}")


BN_SHAPES = [(2, 64, 28, 28),   # NHWC: float4 kernel, grid stride a multiple of C/4 (fixed channels per thread)
             (1, 268, 3, 3),    # NHWC: C/4 = 67 divides no nearby grid: parameters from the prepared table
             (3, 7, 5, 5),      # NHWC: C % 4 != 0, element-wise whatever the pointer
             (9, 256, 14, 14),  # NCHW: N <= 256, B >= 8, N % 4 == 0: batch walk in float4s
             (16, 64, 7, 7),    # NCHW: batch walk, N % 4 != 0: one float per lane
             (2, 16, 56, 56),   # NCHW: large planes of N % 4 == 0: one wave per plane, float4s
             (3, 32, 7, 7),     # NCHW: 7x7 planes, too few images to walk: plane kernel by shape
             (2, 5, 4, 6)]      # C = 5


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=[f"shape{i}" for i in range(len(BN_SHAPES))])
def test_batchnorm(shape, layout):
    g = np.random.default_rng(sum(shape))
    x = g.standard_normal(shape, dtype=np.float32) * 3
    C = shape[1]
    w, b = g.random(C, dtype=np.float32) + 0.5, g.standard_normal(C, dtype=np.float32)
    m, v = g.standard_normal(C, dtype=np.float32), g.random(C, dtype=np.float32) + 0.5
    want = O.batchnorm2d(x, w, b, m, v)
    for inplace in (True, False):
        names = ("inp",) if inplace else ("inp", "out")
        cfgs = V.offset_configs(names) + [{n: 4 for n in names + ("weight", "bias", "mean", "var")}]
        for offs in cfgs:
            same(V.run_batchnorm(x, w, b, m, v, layout, offs, inplace), want, f"bn {layout} {shape} inplace={inplace} {offs}")


POOLS = [(2, 64, 112, 112, 3, 2, 1),   # the network's max-pool: NHWC column walk, NCHW quads (W % 8 == 0)
         (2, 256, 7, 7, 7, 1, 0),      # the global average, both layouts
         (3, 5, 8, 6, 3, 1, 1),        # C % 4 != 0
         (3, 5, 13, 24, 3, 2, 1),      # NCHW quads on odd heights
         (2, 8, 9, 9, 3, 2, 1)]        # NHWC float4 kernels without the column walk


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("case", POOLS, ids=[f"case{i}" for i in range(len(POOLS))])
def test_pools(case, layout):
    B, C, H, W, k, s, p = case
    x = rnd((B, C, H, W), 7 + sum(case))
    for kind, want in (("max", O.maxpool2d(x, k, s, p)), ("avg", O.avgpool2d(x, k, s, p))):
        for offs in V.offset_configs(("inp", "out")):
            same(V.run_pool(kind, x, k, s, p, layout, offs), want, f"{kind}pool {layout} {case} {offs}")


@pytest.mark.parametrize("dims", [(2, 64, 4, 4), (2, 3, 5, 7), (1, 64, 9, 9), (3, 33, 4, 4)], ids=["r64s16", "r3s35", "r64s81", "r33s16"])
def test_transposes(dims):
    """(2, 64, 4, 4): R and S multiples of 4, the 64 x 64 float4 tile kernel when both pointers allow it."""
    B, C, H, W = dims
    x = rnd(dims, sum(dims))
    nhwc = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    for offs in V.offset_configs(("src", "dst")):
        same(V.run_transpose("rn_nchw_to_nhwc", x, nhwc.shape, dims, offs), nhwc, f"nchw_to_nhwc {dims} {offs}")
        same(V.run_transpose("rn_nhwc_to_nchw", nhwc, x.shape, dims, offs), x, f"nhwc_to_nchw {dims} {offs}")


def test_padded_images():
    for shape in ((2, 3, 6, 8), (2, 3, 5, 7), (1, 4, 9, 9)):
        x = rnd(shape, 40 + sum(shape))
        for offs in V.offset_configs(("src", "dst")):
            for Cpad in (4, 8):
                same(V.run_pad(x, Cpad, 0, offs, False), V.pad_reference(x, Cpad, 0), f"pad {shape} {Cpad} {offs}")
                for border in (0, 3):
                    same(V.run_pad(x, Cpad, border, offs, True), V.pad_reference(x, Cpad, border),
                         f"pad_dt {shape} Cpad={Cpad} border={border} {offs}")
            if shape[1] == 3:   # the exact-K stem image: three channels per pixel, rows of no particular alignment
                same(V.run_pad(x, 3, 3, offs, True), V.pad_reference(x, 3, 3), f"pad_dt {shape} Cpad=3 border=3 {offs}")


def test_bf16_bordered_image():
    """rn_nchw_to_nhwc_pad_dt(BF16): two pixels per 16-byte store when dst allows it, element-wise otherwise
    (any 2-byte boundary)."""
    x = rnd((2, 3, 6, 8), 5)
    want = ops.to_bf16_bits(V.pad_reference(x, 4, 3))
    for off_dst in (0, 2, 4, 8):
        for off_src in (0, 4):
            vi, vo = V.place(x, off_src), V.place_out(want.size * 2, off_dst)
            V.must("rn_nchw_to_nhwc_pad_dt", L.RN_DTYPE_BF16, vi.ptr, vo.ptr, 2, 3, 6, 8, 4, 3)
            what = f"pad_dt bf16 src+{off_src} dst+{off_dst}"
            V.check_guards(what, vi)
            same(V.fetch(vo, np.uint16, what), want.reshape(-1), what)


@pytest.mark.parametrize("case", [(3, 64, 10), (70, 96, 130), (1, 2048, 1000)])
def test_linear(case):
    """Any operand (the bias included: it is the contraction's epilogue shift) off a 16-byte boundary: the direct
    kernel, which keeps the reference's summation order -- bit-exact with the oracle."""
    B, fin, fout = case
    x, w, b = rnd((B, fin), sum(case)), rnd((fout, fin), 1 + sum(case)) / np.sqrt(fin), rnd((fout,), 2)
    for bias in (b, None):
        want = O.linear(x, w, bias)
        names = ("inp", "out", "weight") + (("bias",) if bias is not None else ())
        for offs in V.offset_configs(names):
            got = V.run_linear(x, w, bias, offs)
            if V.linear_is_direct(fin, bias, offs):
                same(got, want, f"linear {case} bias={bias is not None} {offs}")
            else:
                assert_close(got, want, fin)


CONV_NHWC = [(2, 64, 64, 12, 12, 1, 1, 0), (2, 32, 96, 7, 7, 3, 1, 1), (1, 4, 16, 9, 9, 3, 1, 1)]


@pytest.mark.parametrize("case", CONV_NHWC, ids=[f"case{i}" for i in range(len(CONV_NHWC))])
def test_conv_nhwc_epilogue(case):
    """rn_conv2d_nhwc_forward with scale, shift, residual and ReLU.  The contraction reads all of its operands,
    those of the epilogue included, in 16-byte pieces; with any of them off a 16-byte boundary the entry point
    runs the direct kernel (reference order).  Its epilogue without a scale is the oracle's op sequence
    conv -> + shift -> + residual -> relu in fp32: bit-exact.  With a scale it is ONE fmaf(sum, scale, shift)
    where the op sequence rounds twice, so that form is compared with assert_close(K + 4), the bound of
    test_fused_epilogue_matches_unfused_sequence."""
    B, Cin, Cout, H, W, k, s, p = case
    seed = 100 + sum(case)
    x, w = rnd((B, Cin, H, W), seed), rnd((Cout, Cin, k, k), seed + 1)
    g = np.random.default_rng(seed + 2)
    scale, shift = g.random(Cout, dtype=np.float32) + 0.5, g.standard_normal(Cout, dtype=np.float32)
    y = O.conv2d(x, w, s, p)
    res = rnd(y.shape, seed + 3)
    want_full = np.maximum(y * scale[None, :, None, None] + shift[None, :, None, None] + res, 0)
    want_noscale = np.maximum(y + shift[None, :, None, None] + res, 0)
    K = Cin * k * k
    # the direct kernel's bits with a scale present, reached through inp: what every unaligned view must give
    direct_full = V.run_conv_nhwc(x, w, s, p, scale, shift, res, True, {"inp": 4})
    for offs in V.offset_configs(("inp", "out", "weight", "scale", "shift", "residual")):
        got = V.run_conv_nhwc(x, w, s, p, scale, shift, res, True, offs)
        assert_close(got, want_full, K + 4)
        if V.conv_nhwc_is_direct(Cin, k, offs):
            same(got, direct_full, f"conv_nhwc {case} {offs}: not the direct kernel's bits")
        else:   # (the contraction sums in another order: an aligned call that fell to the direct kernel would show)
            assert not np.array_equal(got, direct_full), f"conv_nhwc {case} {offs}: the direct kernel's bits"
        if "scale" in offs and len(offs) == 1:
            continue
        offs = {n: o for n, o in offs.items() if n != "scale"}
        got = V.run_conv_nhwc(x, w, s, p, None, shift, res, True, offs)
        if V.conv_nhwc_is_direct(Cin, k, offs):
            same(got, want_noscale, f"conv_nhwc {case} no scale {offs}")
        else:
            assert_close(got, want_noscale, K + 4)


CONV2D = [(3, 64, 256, 8, 8, 1, 1, 0),    # 1x1 stride 1, H*W % 4 == 0: quads by 16-byte loads or the gathering form
          (2, 64, 128, 8, 8, 1, 2, 0),    # 1x1 stride 2
          (3, 32, 64, 14, 14, 3, 1, 1),   # 3x3 padding 1: transposing route or gathered taps
          (5, 64, 72, 7, 7, 1, 1, 0),     # 49 pixels per image
          (2, 48, 64, 8, 8, 1, 1, 0)]     # Cin not a multiple of 32: direct whatever the pointer


@pytest.mark.parametrize("taps", [0, 2])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("case", CONV2D, ids=[f"case{i}" for i in range(len(CONV2D))])
def test_conv2d_forward(case, layout, taps):
    """Every route of rn_conv2d_forward.  Where the route is a contraction (NCHW-native kernel, gathered taps,
    transposing route, NHWC call) the view gives the bits of the aligned call; where an operand's alignment
    sends the call to the direct kernel, the oracle's bits.  Every result within the 2e-6 * sqrt(K) bound."""
    B, Cin, Cout, H, W, k, s, p = case
    x, w = rnd((B, Cin, H, W), 300 + sum(case)), rnd((Cout, Cin, k, k), 301 + sum(case)) / np.sqrt(Cin * k * k)
    want = O.conv2d(x, w, s, p)
    bound = 2e-6 * np.sqrt(Cin * k * k) * float(np.abs(want).max()) + 1e-6
    aligned = None
    for offs in V.offset_configs(("inp", "out", "weight")):
        got = V.run_conv2d(x, w, s, p, layout, taps, offs)
        what = f"conv2d {layout} taps={taps} {case} {offs}"
        if not offs:
            aligned = got
        assert got.shape == want.shape and float(np.abs(got - want).max()) <= bound, what
        if V.conv2d_is_direct(case, layout, taps, offs):
            same(got, want, what + " (direct kernel: reference order)")
        else:
            same(got, aligned, what + " (same bits as the aligned call)")


def test_argmax_on_a_view():
    g = np.random.default_rng(0)
    logits = g.standard_normal((9, 1000), dtype=np.float32)
    logits[1, [10, 500]] = 50.0
    logits[2, 999] = 60.0
    logits[3, 0] = np.nan
    logits[4, 77] = np.nan
    logits[5, :] = -np.inf
    logits[6, 64] = 70.0
    for off in (0, 4, 8, 12):
        assert np.array_equal(V.run_argmax(logits, {"logits": off}), O.argmax(logits)), off


# ---- entry points whose contract is "16-byte aligned": the refusal ---------------------------------------
def _bf16(a):
    return ops.to_bf16_bits(np.ascontiguousarray(np.asarray(a, dtype=np.float32).transpose(0, 2, 3, 1)))


def _conv_bf16(offs):
    B, Cin, Cout, H, W = 2, 64, 64, 6, 6
    x, w = rnd((B, Cin, H, W), 1), rnd((Cout, Cin, 1, 1), 2) / 8
    sc, sh, res = rnd((Cout,), 3), rnd((Cout,), 4), rnd((B, Cout, H, W), 5)
    return V.launch_conv_dt(x, w, 1, 0, sc, sh, res, True, L.RN_DTYPE_BF16, L.RN_DTYPE_BF16, offs)


def _conv_exact(offs):
    B, Cin, Cout, H, W, k = 1, 1, 8, 9, 9, 3
    x, w = rnd((B, Cin, H, W), 6), rnd((Cout, Cin, k, k), 7)
    sc, sh, res = rnd((Cout,), 8), rnd((Cout,), 9), rnd((B, Cout, H, W), 10)
    n = int(L.lib().rn_conv2d_packed_weight_numel_exact(Cin, Cout, k))
    vw0, vp = V.place(w), V.place_out(n * 4)
    V.must("rn_conv2d_pack_weight_exact", vw0.ptr, vp.ptr, Cin, Cout, k)
    vi = V.place(V.pad_reference(x, Cin, 1), offs.get("inp", 0))
    vw = V.place(V.fetch(vp, np.float32, "pack_exact"), offs.get("weight", 0))
    vsc, vsh = V.place(sc, offs.get("scale", 0)), V.place(sh, offs.get("shift", 0))
    vr = V.place(np.ascontiguousarray(res.transpose(0, 2, 3, 1)), offs.get("residual", 0))
    vo = V.place_out(B * Cout * H * W * 4, offs.get("out", 0))
    ep = L.Epilogue(vsc.ptr, vsh.ptr, vr.ptr, 1)
    st = V.call("rn_conv2d_nhwc_exact_forward", vi.ptr, vo.ptr, vw.ptr, k, 1, H, W, B, Cin, Cout, H + 2, W + 2, ctypes.byref(ep))
    return st, [vo], [vi, vw, vsc, vsh, vr]


def _conv_pair(offs):
    B, Cin, Cout, H, W, Cin2 = 3, 64, 64, 9, 9, 32
    t, w = rnd((B, Cin, H, W), 11), rnd((Cout, Cin, 1, 1), 12) / 8
    x2, w2 = rnd((B, Cin2, H, W), 13), rnd((Cout, Cin2, 1, 1), 14) / 6
    sh, res = rnd((Cout,), 15), rnd((B, Cout, H, W), 16)
    return V.launch_conv_pair_dt(t, w, x2, w2, 1, 0, 1, None, None, sh, res, True, L.RN_DTYPE_F32, offs)


def _pool_bf16(kind):
    def run(offs):
        B, C, H, W = 2, 8, 9, 9
        x = rnd((B, C, H, W), 17)
        vi, vo = V.place(_bf16(x), offs.get("inp", 0)), V.place_out(B * C * 5 * 5 * 2, offs.get("out", 0))
        st = V.call(f"rn_{kind}pool2d_nhwc_forward_dt", L.RN_DTYPE_BF16, vi.ptr, vo.ptr, 3, 2, 1, 5, 5, B, C, H, W)
        return st, [vo], [vi]
    return run


def _stem(form):
    """form: "padded" (rn_stem_pool_forward_dt), "nchw" (rn_stem_pool_nchw_forward_dt) or "y"
    (rn_stem_conv_pool_nchw_forward, which also writes the stem tensor)."""
    def run(offs):
        B, H, W = 1, 16, 16   # conv 7x7/2/3 -> 8 x 8, pool 3x3/2/1 -> 4 x 4
        x, w = rnd((B, 3, H, W), 18), rnd((64, 3, 7, 7), 19) / 12
        g = np.random.default_rng(20)
        sc, sh = g.random(64, dtype=np.float32) + 0.5, g.standard_normal(64, dtype=np.float32)
        return V.launch_stem_pool(form, x, w, sc, sh, L.RN_DTYPE_F32, offs)
    return run


def _chain(pair, bf16):
    """rn_conv_chain_forward_dt / rn_conv_chain_pair_forward_dt, 64 -> 256 -> 64 channels on 128 rows (the case of
    test_chain_refuses_misaligned_or_aliased_tensors)."""
    def run(offs):
        dt = L.RN_DTYPE_BF16 if bf16 else L.RN_DTYPE_F32
        t2, x = rnd((2, 64, 8, 8), 21), rnd((2, 64 if pair else 256, 8, 8), 22)
        w3, w1 = rnd((256, 64, 1, 1), 23) / 8, rnd((64, 256, 1, 1), 24) / 16
        g = np.random.default_rng(25)
        sc3, sh3 = g.random(256, dtype=np.float32) + 0.5, g.standard_normal(256, dtype=np.float32)
        sc1, sh1 = g.random(64, dtype=np.float32) + 0.5, g.standard_normal(64, dtype=np.float32)
        if pair:
            return V.launch_chain_dt(t2, x, w3, None, sh3, w1, sc1, sh1, dt, pair_w=rnd((256, 64, 1, 1), 26) / 8, offs=offs)
        return V.launch_chain_dt(t2, x, w3, sc3, sh3, w1, sc1, sh1, dt, offs=offs)
    return run


_CHAIN = ("t2", "x", "y", "w3", "scale3", "shift3", "t1", "w1", "scale1", "shift1")
REFUSING = {
    "conv_bf16": (_conv_bf16, ("inp", "out", "weight", "scale", "shift", "residual")),
    # (the exact-K form gathers its image by dwords: inp may sit on any 4-byte boundary)
    "conv_exact": (_conv_exact, ("out", "weight", "scale", "shift", "residual")),
    "conv_pair": (_conv_pair, ("inp", "out", "weight", "second", "shift", "residual")),
    "pool_bf16_max": (_pool_bf16("max"), ("inp", "out")),
    "pool_bf16_avg": (_pool_bf16("avg"), ("inp", "out")),
    "stem_pool": (_stem("padded"), ("inp", "out", "weight")),
    "stem_pool_nchw": (_stem("nchw"), ("inp", "out", "weight")),
    "stem_conv_pool": (_stem("y"), ("inp", "out", "weight", "y")),
    "chain_f32": (_chain(False, False), _CHAIN),
    "chain_bf16": (_chain(False, True), _CHAIN),
    "chain_pair_f32": (_chain(True, False), tuple(n for n in _CHAIN if n != "scale3")),
    "chain_pair_bf16": (_chain(True, True), tuple(n for n in _CHAIN if n != "scale3")),
}
# operands these entry points read element by element: any 4-byte boundary, the same bits
FREE = {"stem_pool": ("scale", "shift"), "stem_pool_nchw": ("scale", "shift"), "stem_conv_pool": ("scale", "shift"),
        "conv_exact": ("inp",)}


@pytest.mark.parametrize("entry", sorted(REFUSING))
def test_16_byte_entry_points_refuse(entry):
    """The bf16 / exact / pair / stem / bf16-pool entry points document "16-byte aligned" (include/rn_hip.h):
    each pointer operand in turn at +2 (16-bit element types only), +4 and +8 bytes is refused with
    RN_ERR_INVALID and a message that names alignment, before anything is launched -- the output and its
    guards stay as they were; the same call at +0 succeeds and leaves the guards clean."""
    run, names = REFUSING[entry]
    two_byte = entry in ("conv_bf16", "pool_bf16_max", "pool_bf16_avg", "chain_bf16", "chain_pair_bf16")
    for name in names:
        fp32_operand = not two_byte or name.startswith(("scale", "shift"))
        for off in (4, 8) if fp32_operand else (2, 4, 8):
            (st, msg), outs, _ = run({name: off})
            assert st == L.RN_ERR_INVALID and "align" in msg.lower(), f"{entry}: {name}+{off}: status {st} ({msg})"
            for vo in outs:
                V.assert_untouched(vo, f"{entry}: {name}+{off}")
    (st, msg), outs, ins = run({})
    assert st == L.RN_OK, f"{entry}: aligned call: status {st} ({msg})"
    V.check_guards(entry, *outs, *ins)
    aligned = [V.fetch(vo, np.uint8, entry) for vo in outs]
    for a, vo in zip(aligned, outs):
        assert not np.array_equal(a, np.full(vo.nbytes, V.OUT_BYTE, np.uint8)), entry
    for off in (4, 8, 12):
        if entry in FREE:
            (st, msg), outs, ins = run({n: off for n in FREE[entry]})
            assert st == L.RN_OK, f"{entry}: {FREE[entry]}+{off}: status {st} ({msg})"
            V.check_guards(entry, *ins)
            for a, vo in zip(aligned, outs):
                assert np.array_equal(a, V.fetch(vo, np.uint8, entry)), f"{entry}: {FREE[entry]}+{off}: other bits"


def test_packer_and_fold_on_views():
    """rn_conv2d_pack_weight and rn_batchnorm2d_fold read and write element by element: any 4-byte boundary."""
    w = rnd((40, 32, 3, 3), 50)
    want = np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(-1)   # [Cout][kh][kw][Cin]
    for offs in V.offset_configs(("weight", "packed")):
        vw, vp = V.place(w, offs.get("weight", 0)), V.place_out(w.nbytes, offs.get("packed", 0))
        V.must("rn_conv2d_pack_weight", vw.ptr, vp.ptr, 32, 40, 3)
        V.check_guards(f"pack {offs}", vw)
        same(V.fetch(vp, np.float32, f"pack {offs}"), want, f"pack {offs}")
    C = 70
    g = np.random.default_rng(5)
    P = (g.random(C, dtype=np.float32) + 0.5, g.standard_normal(C, dtype=np.float32),
         g.standard_normal(C, dtype=np.float32), g.random(C, dtype=np.float32) + 0.5)
    names, first = ("weight", "bias", "mean", "var", "scale", "shift"), None
    for offs in V.offset_configs(names):
        vin = [V.place(a, offs.get(n, 0)) for n, a in zip(names, P)]
        vsc, vsh = V.place_out(C * 4, offs.get("scale", 0)), V.place_out(C * 4, offs.get("shift", 0))
        V.must("rn_batchnorm2d_fold", *(v.ptr for v in vin), vsc.ptr, vsh.ptr, C)
        V.check_guards(f"fold {offs}", *vin)
        got = (V.fetch(vsc, np.float32, f"fold {offs}"), V.fetch(vsh, np.float32, f"fold {offs}"))
        if first is None:
            first = got
            s64 = P[0].astype(np.float64) / np.sqrt(P[3].astype(np.float64) + 1e-5)
            same(got[0], s64.astype(np.float32), "fold scale")   # (test_batchnorm_fold_entry_point)
        same(got[0], first[0], f"fold scale {offs}")
        same(got[1], first[1], f"fold shift {offs}")


# ---- the deferred route (rn_ctx_set_deferred) on views -----------------------------------------------------
def _rec(name, *args):
    import resnet_c_amd as R
    ctx = R.get_ctx()
    L.check(getattr(L.lib(), name)(ctx.handle, *args), name, ctx.handle)   # (no sync: a sync runs the recorded list)


def _deferred(program, deferred):
    """Run `program()` -- a sequence of _rec calls that returns the views to observe -- literally or recorded;
    recorded buffers get their NCHW content back (rn_observe, then deferred off) before anything is read.
    Returns the fused-launch count of the run."""
    import resnet_c_amd as R
    ctx = R.get_ctx()
    ctx.set_deferred(deferred)
    try:
        f0 = ctx.deferred_stats()["fused_launches"]
        observed = program()
        for v in observed:
            L.check(L.lib().rn_observe(ctx.handle, v.ptr), "rn_observe", ctx.handle)
        ctx.sync()
        return ctx.deferred_stats()["fused_launches"] - f0
    finally:
        ctx.set_deferred(False)
        st = ctx.deferred_stats()
        assert st["pending_ops"] == 0 and st["nhwc_buffers"] == 0


def _near_literal(got, literal, what):   # the deferred-against-literal comparison of test_defer_gpu.py
    assert np.abs(got - literal).max() <= 2e-5 * max(1.0, float(np.abs(literal).max())), what


@pytest.mark.parametrize("which", ["aligned", "inp", "out", "other"])
def test_deferred_chain_on_views(which):
    """conv -> bn -> add -> relu (in place) recorded with the conv's inp, its out, or the add's other operand at
    +4 bytes: the deferred route declines to fold what the contraction cannot read in 16-byte pieces
    (rn_defer.hip: fusable_conv for inp / out, the residual check for the add's other operand) and runs it
    literally.  Against the literal route on the same views; guards clean."""
    B, Cin, Cout, H, W, k, s, p = 2, 64, 64, 14, 14, 3, 1, 1
    x, w = rnd((B, Cin, H, W), 60), rnd((Cout, Cin, k, k), 61) / np.sqrt(Cin * k * k)
    g = np.random.default_rng(62)
    bn = (g.random(Cout, dtype=np.float32) + 0.5, g.standard_normal(Cout, dtype=np.float32) * 0.1,
          g.standard_normal(Cout, dtype=np.float32) * 0.1, g.random(Cout, dtype=np.float32) + 0.5)
    res = rnd((B, Cout, H, W), 63)
    offs = {} if which == "aligned" else {which: 4}
    n = B * Cout * H * W

    def run(deferred):
        vx, vw, vr = V.place(x, offs.get("inp", 0)), V.place(w.astype(np.float32)), V.place(res, offs.get("other", 0))
        vp = [V.place(a) for a in bn]
        vo = V.place_out(n * 4, offs.get("out", 0))

        def program():
            _rec("rn_conv2d_forward", vx.ptr, vo.ptr, vw.ptr, k, s, p, H, W, B, Cin, Cout, H, W)
            _rec("rn_batchnorm2d_forward", vo.ptr, vo.ptr, *(t.ptr for t in vp), B, Cout, H * W)
            _rec("rn_add_forward", vo.ptr, vr.ptr, vo.ptr, n)
            _rec("rn_relu_forward", vo.ptr, vo.ptr, n)
            return [vo]
        fused = _deferred(program, deferred)
        what = f"deferred chain {offs} deferred={deferred}"
        V.check_guards(what, vx, vw, vr, *vp)
        return V.fetch(vo, np.float32, what).reshape(B, Cout, H, W), fused

    literal, _ = run(False)
    got, fused = run(True)
    want = O.relu_(O.add_(O.batchnorm2d_(O.conv2d(x, w.astype(np.float32), s, p), *bn), res))
    assert np.array_equal(literal, want) or np.abs(literal - want).max() <= 3e-6 * np.sqrt(Cin * k * k) * float(np.abs(want).max()) + 1e-5
    _near_literal(got, literal, f"deferred chain {offs}")
    if which in ("inp", "out"):
        assert fused == 0, f"{offs}: the convolution was folded ({fused} fused launches)"
        same(got, literal, f"deferred chain {offs}: the literal route's bits")
    else:
        assert fused == 1, f"{offs}: {fused} fused launches"


@pytest.mark.parametrize("which", ["aligned", "x", "t1", "out"])
def test_deferred_basic_block_on_views(which):
    """A basic block -- conv1 -> bn1 -> relu -> conv2 -> bn2 -> add(x) -> relu -- recorded with the block input
    (conv1's inp and the add's other operand), the middle tensor (conv1's out, conv2's inp) or the block output
    at +4 bytes; against the literal route on the same views."""
    B, C, H, W = 2, 64, 8, 8
    x = rnd((B, C, H, W), 70)
    w1, w2 = ((rnd((C, C, 3, 3), 71 + i) / np.sqrt(C * 9)).astype(np.float32) for i in range(2))
    g = np.random.default_rng(73)
    bns = [(g.random(C, dtype=np.float32) + 0.5, g.standard_normal(C, dtype=np.float32) * 0.1,
            g.standard_normal(C, dtype=np.float32) * 0.1, g.random(C, dtype=np.float32) + 0.5) for _ in range(2)]
    offs = {} if which == "aligned" else {which: 4}
    n = B * C * H * W

    def run(deferred):
        vx, vw1, vw2 = V.place(x, offs.get("x", 0)), V.place(w1), V.place(w2)
        vp1, vp2 = [V.place(a) for a in bns[0]], [V.place(a) for a in bns[1]]
        vt, vo = V.place_out(n * 4, offs.get("t1", 0)), V.place_out(n * 4, offs.get("out", 0))

        def program():
            _rec("rn_conv2d_forward", vx.ptr, vt.ptr, vw1.ptr, 3, 1, 1, H, W, B, C, C, H, W)
            _rec("rn_batchnorm2d_forward", vt.ptr, vt.ptr, *(t.ptr for t in vp1), B, C, H * W)
            _rec("rn_relu_forward", vt.ptr, vt.ptr, n)
            _rec("rn_conv2d_forward", vt.ptr, vo.ptr, vw2.ptr, 3, 1, 1, H, W, B, C, C, H, W)
            _rec("rn_batchnorm2d_forward", vo.ptr, vo.ptr, *(t.ptr for t in vp2), B, C, H * W)
            _rec("rn_add_forward", vo.ptr, vx.ptr, vo.ptr, n)
            _rec("rn_relu_forward", vo.ptr, vo.ptr, n)
            return [vo, vt, vx]
        fused = _deferred(program, deferred)
        what = f"deferred basic block {offs} deferred={deferred}"
        V.check_guards(what, vw1, vw2, *vp1, *vp2)
        same(V.fetch(vx, np.float32, what).reshape(x.shape), x, what + ": the block input changed")
        return V.fetch(vt, np.float32, what), V.fetch(vo, np.float32, what), fused

    lit_t, lit_o, _ = run(False)
    got_t, got_o, fused = run(True)
    _near_literal(got_t, lit_t, f"basic block {offs}: t1")
    _near_literal(got_o, lit_o, f"basic block {offs}: out")
    # conv1 folds unless x or t1 is off a 16-byte boundary, conv2 unless t1 or out is
    assert fused == {"aligned": 2, "x": 1, "t1": 0, "out": 1}[which], f"{offs}: {fused} fused launches"


@pytest.mark.parametrize("which", ["aligned", "inp", "pool_out"])
def test_deferred_stem_on_views(which):
    """conv 7x7/2/3 -> bn -> relu -> maxpool 3x3/2/1 recorded: one fused stem launch when the image and the pooled
    tensor sit on 16-byte boundaries (rn_defer.hip), the convolution's fold plus a literal pool otherwise.  Stem
    tensor and pooled tensor against the literal route on the same views."""
    B, H, W = 2, 32, 32
    x, w = rnd((B, 3, H, W), 80), (rnd((64, 3, 7, 7), 81) / 12).astype(np.float32)
    g = np.random.default_rng(82)
    bn = (g.random(64, dtype=np.float32) + 0.5, g.standard_normal(64, dtype=np.float32) * 0.1,
          g.standard_normal(64, dtype=np.float32) * 0.1, g.random(64, dtype=np.float32) + 0.5)
    offs = {} if which == "aligned" else {which: 4}
    ny, npool = B * 64 * 16 * 16, B * 64 * 8 * 8

    def run(deferred):
        vx, vw, vp = V.place(x, offs.get("inp", 0)), V.place(w), [V.place(a) for a in bn]
        vy, vo = V.place_out(ny * 4), V.place_out(npool * 4, offs.get("pool_out", 0))

        def program():
            _rec("rn_conv2d_forward", vx.ptr, vy.ptr, vw.ptr, 7, 2, 3, 16, 16, B, 3, 64, H, W)
            _rec("rn_batchnorm2d_forward", vy.ptr, vy.ptr, *(t.ptr for t in vp), B, 64, 256)
            _rec("rn_relu_forward", vy.ptr, vy.ptr, ny)
            _rec("rn_maxpool2d_forward", vy.ptr, vo.ptr, 3, 2, 1, 8, 8, B, 64, 16, 16)
            return [vo, vy]
        _deferred(program, deferred)
        what = f"deferred stem {offs} deferred={deferred}"
        V.check_guards(what, vx, vw, *vp)
        return V.fetch(vy, np.float32, what), V.fetch(vo, np.float32, what)

    lit_y, lit_o = run(False)
    got_y, got_o = run(True)
    _near_literal(got_y, lit_y, f"deferred stem {offs}: stem tensor")
    _near_literal(got_o, lit_o, f"deferred stem {offs}: pooled tensor")
