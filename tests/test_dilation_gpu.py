"""Dilated convolution on the GPU: rn_conv2d_dilated_forward and rn_conv2d_dilated_nhwc_forward_dt.

Yardsticks from outside the code under test (tests/test_dilation_host.py holds them to each other on the CPU):
  A  torch on the CPU, F.conv2d(..., dilation=d, groups=g) in float64;
  B  the committed oracle on a zero-stuffed kernel (the reference's summation order: the zero products add
     exact zeros), for the routes that promise the reference's bits.
"""
import ctypes
import functools

import numpy as np
import pytest

import resnet_c_amd as R
import views as V
from resnet_c_amd import _lib as L
from resnet_c_amd import ops
from test_dilation_host import conv64, stuffed_oracle
from test_schedules_gpu import schedule

pytestmark = pytest.mark.gpu

F32, BF16 = L.RN_DTYPE_F32, L.RN_DTYPE_BF16

# (B, Cin, Cout, H, W, k, s, p, d): the smallest shapes at which each mistake shows
CASES = {
    "w_below_span":   (2, 32, 32, 7, 5, 3, 1, 2, 2),       # W < 2d + 1, two images: bleed into the next image / row
    "centre_row":     (1, 64, 64, 3, 9, 3, 1, 4, 4),       # only the centre kernel row is ever inside
    "stride2":        (2, 64, 32, 9, 8, 3, 2, 2, 2),       # stride with dilation
    "no_padding":     (1, 32, 64, 11, 10, 3, 1, 0, 2),     # the output shrinks
    "many_tiles":     (3, 128, 128, 14, 14, 3, 1, 2, 2),   # 588 rows: several M tiles, a ragged last one, 4 segments per tap
    "pad_not_d":      (2, 32, 32, 6, 7, 3, 1, 3, 5),
    "k5":             (1, 32, 32, 13, 13, 5, 1, 4, 2),
    "layer3":         (1, 256, 256, 28, 28, 3, 1, 2, 2),   # the model's shapes
    "layer4":         (1, 512, 512, 28, 28, 3, 1, 4, 4),
}
BF16_CASES = [n for n, c in CASES.items() if c[1] % 64 == 0]


def rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def operands(name):
    B, Cin, Cout, H, W, k, s, p, d = CASES[name]
    seed = 1000 + sum(CASES[name])
    x, w = rnd((B, Cin, H, W), seed), rnd((Cout, Cin, k, k), seed + 1) / np.float32(np.sqrt(Cin * k * k))
    x.setflags(write=False), w.setflags(write=False)
    return x, w


@functools.lru_cache(maxsize=None)
def reference(name, bf16=False):
    """yardstick A, computed once per case and shared"""
    x, w = operands(name)
    _, _, _, _, _, _, s, p, d = CASES[name]
    ref = conv64(ops.bf16_round(x), ops.bf16_round(w), s, p, d) if bf16 else conv64(x, w, s, p, d)
    ref.setflags(write=False)
    return ref


def tol_f32(ref, K):
    """the bound tests/test_ops_gpu.py and test_grouped_gpu.py use for these kernels"""
    return 2e-6 * np.sqrt(K) * float(np.abs(ref).max()) + 1e-6


def tol_bf16(ref):
    """as test_bf16_route_is_the_dense_panel"""
    return 2.0 ** -8 * float(np.abs(ref).max()) + 1e-6


def check(got, ref, tol, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    print(f"\n  dilation: {what}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (what, err, tol)


# ---- runners on views between guard bands ---------------------------------------------------------------------
def dilated_size(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def packed_for(w, Cin, G, dt):
    if G == 1:
        return V.packed_weight_dt(w, dt)
    Cout, _, k, _ = w.shape
    pn = int(L.lib().rn_conv2d_grouped_packed_weight_numel_dt(dt, Cin, Cout, k, G))
    vw0, vp = V.place(np.asarray(w, dtype=np.float32)), V.place_out(pn * V._es(dt))
    V.must("rn_conv2d_grouped_pack_weight_dt", dt, vw0.ptr, vp.ptr, Cin, Cout, k, G)
    return V.fetch(vp, V._np(dt), "rn_conv2d_grouped_pack_weight_dt")


def launch_nhwc_dt(x, w, s, p, d, G, scale, shift, residual, relu, dt_in, dt_out, offs=None, ho=None, wo=None):
    """ONE rn_conv2d_dilated_nhwc_forward_dt on views; ((status, text), output view, input views)"""
    offs = offs or {}
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    ho = dilated_size(H, k, s, p, d) if ho is None else ho
    wo = dilated_size(W, k, s, p, d) if wo is None else wo
    vi, vw = V.place(V._act(x, dt_in), offs.get("inp", 0)), V.place(packed_for(w, Cin, G, dt_in), offs.get("weight", 0))
    vsc, vsh = V._f32(scale, offs.get("scale", 0)), V._f32(shift, offs.get("shift", 0))
    vr = V.place(V._act(residual, dt_out), offs.get("residual", 0)) if residual is not None else None
    vo = V.place_result(B * max(ho, 1) * max(wo, 1), Cout, dt_out, offs.get("out", 0))
    ep = L.Epilogue(V._ptr(vsc), V._ptr(vsh), V._ptr(vr), int(relu))
    st = V.call("rn_conv2d_dilated_nhwc_forward_dt", dt_in, dt_out, vi.ptr, vo.ptr, vw.ptr, k, s, p, d, ho, wo, B, Cin,
                Cout, H, W, G, ctypes.byref(ep))
    return st, vo, [vi, vw, vsc, vsh, vr]


def run_nhwc_dt(x, w, s, p, d, G=1, scale=None, shift=None, residual=None, relu=False, dt_in=F32, dt_out=F32, offs=None):
    B, _, H, W = x.shape
    Cout, _, k, _ = w.shape
    what = f"rn_conv2d_dilated_nhwc_forward_dt {dt_in}->{dt_out} {x.shape} w={w.shape} s={s} p={p} d={d} G={G} offs={offs}"
    st, vo, ins = launch_nhwc_dt(x, w, s, p, d, G, scale, shift, residual, relu, dt_in, dt_out, offs)
    V._ok(what, st)
    V.check_guards(what, *ins)
    return V.fetch_result(vo, (B, Cout, dilated_size(H, k, s, p, d), dilated_size(W, k, s, p, d)), dt_out, what)


def run_forward(x, w, s, p, d, G, layout, offs=None):
    """rn_conv2d_dilated_forward (OIHW weight, tensors in the context layout) on views"""
    offs = offs or {}
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    ho, wo = dilated_size(H, k, s, p, d), dilated_size(W, k, s, p, d)
    what = f"rn_conv2d_dilated_forward {layout} {x.shape} w={w.shape} s={s} p={p} d={d} G={G} offs={offs}"
    vi, vw = V.place(V._dev(x, layout), offs.get("inp", 0)), V.place(np.asarray(w, dtype=np.float32), offs.get("weight", 0))
    vo = V.place_out(B * Cout * ho * wo * 4, offs.get("out", 0), V.contraction_guard(Cout * 4))
    V.must("rn_conv2d_dilated_forward", vi.ptr, vo.ptr, vw.ptr, k, s, p, d, ho, wo, B, Cin, Cout, H, W, G, layout=layout)
    V.check_guards(what, vi, vw)
    return V._host(V.fetch(vo, np.float32, what, written=True), (B, Cout, ho, wo), layout)


# ---- fp32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_matches_torch(name, layout):
    B, Cin, Cout, H, W, k, s, p, d = CASES[name]
    x, w = operands(name)
    ref = reference(name)
    check(ops.conv2d_dilated(x, w, s, p, d, 1, layout), ref, tol_f32(ref, Cin * k * k), f"{name} {layout} forward")
    if layout == "nhwc":
        check(ops.conv2d_dilated_nhwc(x, w, s, p, d), ref, tol_f32(ref, Cin * k * k), f"{name} packed nhwc")


@pytest.mark.parametrize("name,G", [("w_below_span", 1), ("stride2", 1), ("pad_not_d", 1), ("many_tiles", 1),
                                    ("w_below_span", 8), ("pad_not_d", 8), ("many_tiles", 8)])
def test_fp32_epilogue(name, G):
    """the epilogue combinations of test_grouped_epilogue, on the dense path and (Cin == Cout) the grouped fast path"""
    B, Cin, Cout, H, W, k, s, p, d = CASES[name]
    x = operands(name)[0]
    w = rnd((Cout, Cin // G, k, k), 7 + Cin) / np.float32(np.sqrt(k * k * Cin // G))
    conv = conv64(x, w, s, p, d, G)
    g = np.random.default_rng(33 + Cout)
    sc, sh = g.random(Cout, dtype=np.float32) + 0.5, g.standard_normal(Cout, dtype=np.float32)
    res = rnd(conv.shape, 34 + Cout)
    bc = lambda v: v[None, :, None, None]
    for scale, shift, residual, relu in ((sc, sh, res, True), (sc, sh, None, True), (None, sh, None, False),
                                         (sc, None, res, False), (None, None, None, True)):
        ref = conv * (bc(scale) if scale is not None else 1) + (bc(shift) if shift is not None else 0)
        if residual is not None:
            ref = ref + residual
        if relu:
            ref = np.maximum(ref, 0)
        got = ops.conv2d_dilated_nhwc(x, w, s, p, d, G, scale, shift, residual, relu)
        assert np.abs(got - ref).max() <= 2e-5 * float(np.abs(ref).max()) + 1e-6, (name, G, relu)
    a = ops.conv2d_dilated_nhwc(x, w, s, p, d, G, sc, sh, res, False)
    b = ops.conv2d_dilated_nhwc(x, w, s, p, d, G, sc, sh, None, False)
    assert np.abs((a - b) - res).max() <= 1e-5 * float(np.abs(a).max()) + 1e-6 and np.abs(a - b).max() > 1.0


# ---- bf16 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BF16_CASES)
def test_bf16_matches_torch_on_rounded_operands(name):
    B, Cin, Cout, H, W, k, s, p, d = CASES[name]
    x, w = operands(name)
    ref = reference(name, True)
    check(ops.conv2d_dilated_nhwc_bf16(x, w, s, p, d), ref, tol_bf16(ref), f"{name} bf16")
    check(ops.conv2d_dilated_nhwc_bf16(x, w, s, p, d, out_f32=True), ref, tol_bf16(ref), f"{name} bf16 -> f32")


def kernel_of_launch(run, cand):
    """run() under forced candidate `cand` with the debug stamps on: (result, kernel that ran, blocks)"""
    from resnet_c_amd.tensor import _DeviceBuffer
    ctx, lib = R.get_ctx(), L.lib()
    nblk = 1 << 12
    stamps = _DeviceBuffer(ctx, nblk * 16 * 8)
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
    return got, kernel, int(wrote[:, 0].sum())


@pytest.mark.parametrize("name", ["layer3", "layer4"])
def test_bf16_model_shapes_run_on_the_wide_tiles(name):
    """every wide-tile candidate is eligible for the model's dilated shapes and IS the kernel that runs (read from
    the debug stamps, as test_wide_tiles_and_strip); the last candidate, the strip kernel, is out of reach"""
    B, Cin, Cout, H, W, k, s, p, d = CASES[name]
    x, w = operands(name)
    ref = reference(name, True)
    ncand = L.lib().rn_conv_tile_candidates()
    wide_tiles = ((256, 256), (256, 128), (128, 256), (256, 64), (224, 256), (128, 128))
    assert ncand == 9 + len(wide_tiles)
    M, first = B * H * W, None
    run = lambda: run_nhwc_dt(x, w, s, p, d, dt_in=BF16, dt_out=BF16)
    for cand in range(9, ncand + 1):
        got, kernel, grid = kernel_of_launch(run, cand)
        if cand < ncand:
            bm, bn = wide_tiles[cand - 9]
            assert kernel == "wide" and grid == -(-M // bm) * -(-Cout // bn), (name, cand, kernel, grid)
        else:
            assert kernel != "strip", (name, cand, kernel)
        check(got, ref, tol_bf16(ref), f"{name} bf16 candidate {cand} ({kernel})")
        first = got if first is None else first
        assert np.array_equal(got, first), (name, cand)


def test_strip_shapes_stay_off_the_strip_kernel():
    """3x3 / stride 1 / 128 -> 128 and 64 -> 64 with d = p = 2 keep the plane's size, like the strip kernel's
    own layers; the forced strip candidate must not take them"""
    for C in (64, 128):
        x, w = rnd((3, C, 7, 9), 40 + C), rnd((C, C, 3, 3), 41 + C) / np.float32(np.sqrt(9 * C))
        ref = conv64(ops.bf16_round(x), ops.bf16_round(w), 1, 2, 2)
        ncand = L.lib().rn_conv_tile_candidates()
        got, kernel, _ = kernel_of_launch(lambda: run_nhwc_dt(x, w, 1, 2, 2, dt_in=BF16, dt_out=BF16), ncand)
        assert kernel != "strip"
        check(got, ref, tol_bf16(ref), f"strip shape C={C} d=2")


# ---- grouped fp32 fast path -------------------------------------------------------------------------------------
# (B, H, W, stride, pad, d)
GROUP_PLANES = [(2, 7, 9, 1, 2, 2), (1, 5, 6, 1, 4, 4), (2, 7, 9, 2, 2, 2)]


@pytest.mark.parametrize("cg", [(128, 32), (256, 32), (1024, 32), (2048, 32)])
def test_grouped_fast_path(cg):
    C, G = cg
    for B, H, Wd, s, p, d in GROUP_PLANES:
        x, w = rnd((B, C, H, Wd), C + G + H), rnd((C, C // G, 3, 3), C + G + H + 1)
        ref = conv64(x, w, s, p, d, G)
        tol = 2e-6 * np.sqrt(9 * C // G) * float(np.abs(ref).max()) + 1e-6     # tol_of of test_grouped_gpu.py
        for layout in ("nchw", "nhwc"):
            check(ops.conv2d_dilated(x, w, s, p, d, G, layout), ref, tol, f"grouped {cg} {(B, H, Wd, s, p, d)} {layout}")
        check(run_nhwc_dt(x, w, s, p, d, G), ref, tol, f"grouped {cg} {(B, H, Wd, s, p, d)} packed")


def test_grouped_bf16_is_the_dense_panel():
    C, G = 128, 32
    x, w = rnd((2, C, 6, 5), 80), rnd((C, C // G, 3, 3), 81) / 6
    ref = conv64(ops.bf16_round(x), ops.bf16_round(w), 1, 2, 2, G)
    check(ops.conv2d_dilated_nhwc_bf16(x, w, 1, 2, 2, G), ref, tol_bf16(ref), "grouped bf16 d=2")


# ---- direct routes: the reference's bits ------------------------------------------------------------------------
def test_direct_routes_are_bit_exact_with_the_stuffed_oracle():
    # Cin = 12: no whole channel segment
    x, w = rnd((2, 12, 7, 6), 1), rnd((8, 12, 3, 3), 2)
    want = stuffed_oracle(x, w, 1, 2, 2)
    for layout in ("nchw", "nhwc"):
        assert np.array_equal(ops.conv2d_dilated(x, w, 1, 2, 2, 1, layout), want), layout
    assert np.array_equal(ops.conv2d_dilated_nhwc(x, w, 1, 2, 2), want)
    # the stem's small-Cin packing has no dilated form: its panel is read by the direct kernel
    x, w = rnd((2, 3, 9, 8), 3), rnd((16, 3, 7, 7), 4)
    want = stuffed_oracle(x, w, 2, 6, 2)
    for layout in ("nchw", "nhwc"):
        assert np.array_equal(ops.conv2d_dilated(x, w, 2, 6, 2, 1, layout), want), layout
    assert np.array_equal(ops.conv2d_dilated_nhwc(x, w, 2, 6, 2), want)
    # one operand 4 bytes off a 16-byte boundary, where the undilated entry point takes the direct kernel
    name = "w_below_span"
    B, Cin, Cout, H, W, k, s, p, d = CASES[name]
    x, w = operands(name)
    want = stuffed_oracle(x, w, s, p, d)
    for offs in ({"inp": 4}, {"out": 4}, {"weight": 4}):
        assert np.array_equal(run_nhwc_dt(x, w, s, p, d, offs=offs), want), offs
    for layout, offs in (("nhwc", {"inp": 4}), ("nhwc", {"out": 4}), ("nchw", {"out": 4})):
        assert np.array_equal(run_forward(x, w, s, p, d, 1, layout, offs), want), (layout, offs)
    # grouped: a shape the super-group kernel does not take, and the fast shape 4 bytes off
    x, w = rnd((1, 24, 7, 6), 5), rnd((36, 2, 3, 3), 6)
    want = stuffed_oracle(x, w, 2, 2, 2, 12)
    for layout in ("nchw", "nhwc"):
        assert np.array_equal(ops.conv2d_dilated(x, w, 2, 2, 2, 12, layout), want), layout
    x, w = rnd((2, 128, 5, 6), 7), rnd((128, 4, 3, 3), 8)
    want = stuffed_oracle(x, w, 1, 2, 2, 32)
    assert np.array_equal(run_nhwc_dt(x, w, 1, 2, 2, 32, offs={"inp": 4}), want)


# ---- dilation = 1 is the existing entry point -----------------------------------------------------------------
def test_dilation_one_is_the_existing_launch():
    x, w = rnd((2, 64, 9, 11), 11), rnd((72, 64, 3, 3), 12) / np.float32(24)
    for layout in ("nchw", "nhwc"):
        assert np.array_equal(ops.conv2d_dilated(x, w, 1, 1, 1, 1, layout), ops.conv2d(x, w, 1, 1, layout)), layout
    xs, ws = rnd((2, 3, 20, 20), 13), rnd((64, 3, 7, 7), 14)          # the stem's packing
    for layout in ("nchw", "nhwc"):
        assert np.array_equal(ops.conv2d_dilated(xs, ws, 2, 3, 1, 1, layout), ops.conv2d(xs, ws, 2, 3, layout)), layout
    assert np.array_equal(ops.conv2d_dilated_nhwc(xs, ws, 2, 3, 1), ops.conv2d_nhwc_fused(xs, ws, 2, 3))
    xg, wg = rnd((2, 128, 7, 9), 15), rnd((128, 4, 3, 3), 16)
    for layout in ("nchw", "nhwc"):
        assert np.array_equal(ops.conv2d_dilated(xg, wg, 1, 1, 1, 32, layout), ops.conv2d_grouped(xg, wg, 1, 1, 32, layout))
    assert np.array_equal(ops.conv2d_dilated_nhwc(xg, wg, 2, 1, 1, 32), ops.conv2d_grouped_nhwc(xg, wg, 2, 1, 32))
    assert np.array_equal(ops.conv2d_dilated_nhwc_bf16(xg, wg, 1, 1, 1, 32), ops.conv2d_grouped_nhwc_bf16(xg, wg, 1, 1, 32))
    g = np.random.default_rng(17)
    sc, sh, res = g.random(72, dtype=np.float32) + 0.5, g.standard_normal(72, dtype=np.float32), rnd((2, 72, 9, 11), 18)
    ncand = L.lib().rn_conv_tile_candidates()
    for cand in range(1, ncand + 1):       # one case per tile candidate
        with schedule(tile=cand):
            if cand <= 8:
                assert np.array_equal(ops.conv2d_dilated_nhwc(x, w, 1, 1, 1, 1, sc, sh, res, True),
                                      ops.conv2d_nhwc_fused(x, w, 1, 1, sc, sh, res, True)), cand
            assert np.array_equal(ops.conv2d_dilated_nhwc_bf16(x, w, 1, 1, 1, 1, sc, sh, res, True),
                                  ops.conv2d_nhwc_bf16(x, w, 1, 1, sc, sh, res, True)), cand


def test_one_tap_has_no_dilation():
    x, w = rnd((2, 64, 7, 6), 21), rnd((40, 64, 1, 1), 22)
    for layout in ("nchw", "nhwc"):
        assert np.array_equal(ops.conv2d_dilated(x, w, 2, 0, 3, 1, layout), ops.conv2d_dilated(x, w, 2, 0, 1, 1, layout))
    assert np.array_equal(ops.conv2d_dilated_nhwc(x, w, 1, 0, 3), ops.conv2d_dilated_nhwc(x, w, 1, 0, 1))
    assert np.array_equal(ops.conv2d_dilated_nhwc_bf16(x, w, 1, 0, 3), ops.conv2d_dilated_nhwc_bf16(x, w, 1, 0, 1))
    assert np.array_equal(ops.conv2d_dilated_nhwc(x, w, 1, 0, 3), ops.conv2d_nhwc_fused(x, w, 1, 0))


# ---- schedules --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["many_tiles", "layer3"])
def test_every_schedule(name, dt):
    """every tile candidate, split K and every XCD grouping: within the element type's bound, and the same bits
    across the candidates and the XCD groupings (as the undilated layer: only split K changes the order)"""
    B, Cin, Cout, H, W, k, s, p, d = CASES[name]
    x, w = operands(name)
    bf = dt == BF16
    ref = reference(name, bf)
    tol = tol_bf16(ref) if bf else tol_f32(ref, Cin * k * k)
    run = lambda: run_nhwc_dt(x, w, s, p, d, dt_in=dt, dt_out=dt)
    first = None
    ncand = L.lib().rn_conv_tile_candidates()
    for cand in range(0, (ncand if bf else 8) + 1):
        with schedule(tile=cand):
            got = run()
        check(got, ref, tol, f"{name} {dt} candidate {cand}")
        first = got if first is None else first
        assert np.array_equal(got, first), f"{name} {dt}: candidate {cand} has other bits than the dispatcher's choice"
    for xcd in (1, 2, 4, 8):
        with schedule(tile=4, xcd=xcd):
            got = run()
        assert np.array_equal(got, first), f"{name} {dt}: xcd groups {xcd} change bits"
    for tile in (0, 4):
        with schedule(tile=tile, split_k=16):
            got = run()
        check(got, ref, tol, f"{name} {dt} split K, tile {tile}")


# ---- guard bands ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w_below_span", "centre_row"])
def test_views_between_guard_bands(name):
    """inputs between NaN bands, outputs poisoned between wide bands: a tap that left its image would read a NaN
    or the neighbouring image, a store outside the tensor would dirty a band (run_* check every band)"""
    B, Cin, Cout, H, W, k, s, p, d = CASES[name]
    x, w = operands(name)
    ref = reference(name)
    tol = tol_f32(ref, Cin * k * k)
    for offs in V.offset_configs(("inp", "weight", "out"), offsets=(16,)):
        check(run_nhwc_dt(x, w, s, p, d, offs=offs), ref, tol, f"{name} views {offs}")
        for layout in ("nchw", "nhwc"):
            check(run_forward(x, w, s, p, d, 1, layout, offs), ref, tol, f"{name} views {layout} {offs}")
    if Cin % 64 == 0:
        refb = reference(name, True)
        check(run_nhwc_dt(x, w, s, p, d, dt_in=BF16, dt_out=BF16), refb, tol_bf16(refb), f"{name} views bf16")
    if Cin == Cout:
        wg = rnd((Cout, Cin // 8, k, k), 3)
        refg = conv64(x, wg, s, p, d, 8)
        check(run_nhwc_dt(x, wg, s, p, d, 8), refg, tol_f32(refg, Cin // 8 * k * k), f"{name} views grouped")


# ---- refusals ---------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    name = "w_below_span"
    B, Cin, Cout, H, W, k, s, p, d = CASES[name]
    x, w = operands(name)
    ho, wo = dilated_size(H, k, s, p, d), dilated_size(W, k, s, p, d)
    assert L.RN_CONV_MAX_DILATION >= 64
    for dt in (F32, BF16) if Cin % 64 == 0 else (F32,):
        for G in (1, 8):
            wq = w if G == 1 else rnd((Cout, Cin // G, k, k), 9)
            for dd, hh in ((0, ho), (L.RN_CONV_MAX_DILATION + 1, ho), (d, ho + 1), (d, ho - 1), (1, ho)):
                (st, msg), vo, ins = launch_nhwc_dt(x, wq, s, p, dd, G, None, None, None, False, dt, dt, ho=hh, wo=wo)
                assert st == L.RN_ERR_INVALID and msg, (dt, G, dd, hh, st)
                V.assert_untouched(vo, f"refused d={dd} h_out={hh}")
    ctx, lib = R.get_ctx(), L.lib()
    dx, dw = R.FloatTensor.from_numpy(x, R.Device.GPU), R.FloatTensor.from_numpy(w, R.Device.GPU)
    out = R.FloatTensor((B, Cout, ho, wo), R.Device.GPU)
    for dd, hh, G in ((0, ho, 1), (L.RN_CONV_MAX_DILATION + 1, ho, 1), (d, ho + 1, 1), (d, ho, 3), (0, ho, 8)):
        assert lib.rn_conv2d_dilated_forward(ctx.handle, dx.data(), out.data(), dw.data(), k, s, p, dd, hh, wo, B, Cin,
                                             Cout, H, W, G) == L.RN_ERR_INVALID, (dd, hh, G)
    # the largest dilation the contract promises at k = 3: every tap but the centre one is outside a small image
    xs, ws = rnd((1, 32, 5, 4), 31), rnd((32, 32, 3, 3), 32)
    for dd in (64, L.RN_CONV_MAX_DILATION):
        ref = conv64(xs, ws, 1, dd, dd)
        check(ops.conv2d_dilated_nhwc(xs, ws, 1, dd, dd), ref, tol_f32(ref, 32 * 9), f"d = {dd}")


# =====================================================================================================================
# models: rn_model_set_dilation (torchvision's replace_stride_with_dilation)
# =====================================================================================================================
import os                                            # noqa: E402
import subprocess                                    # noqa: E402

import torch                                         # noqa: E402
import torch.nn.functional as F                      # noqa: E402

from oracle import netref as N                       # noqa: E402
from resnet_c_amd import preprocess                  # noqa: E402
from resnet_c_amd import weights as W                # noqa: E402
from test_dilation_host import dilated_features_f64  # noqa: E402

TOL = 1e-4  # fp32 whole-network bound, as test_model_gpu.py / test_grouped_gpu.py / test_input_size_gpu.py
MB = 3      # images per model test


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def state_of(arch):
    return W.generate_state(arch, seed=0)


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(arch, dtype="f32"):
        if (arch, dtype) not in made:
            made[(arch, dtype)] = R.NativeModel(arch, state=state_of(arch), dtype=dtype)
        return made[(arch, dtype)]
    yield get
    for m in made.values():
        m.close()


@functools.lru_cache(maxsize=None)
def images(size, n=MB):
    x = W.generate_input(n, seed=300 + size[0] + size[1], hw=size)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ref_features(arch, size, flags):
    f = dilated_features_f64(arch, state_of(arch), images(size), flags)
    f.setflags(write=False)
    return f


def ref_logits(arch, size, flags):
    return N.ref_logits(state_of(arch), ref_features(arch, size, flags))


def three_modes(m, x):
    got = {"ops": m.forward(x, fused=False), "fused": m.forward(x, fused=True)}
    m.set_pair_fusion(False)
    try:
        got["fused, pair fusion off"] = m.forward(x, fused=True)
    finally:
        m.set_pair_fusion(True)
    return got


@pytest.mark.parametrize("size", [(64, 64), (96, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("flags", [(0, 1, 1), (1, 1, 1)], ids=lambda f: "".join(map(str, f)))
@pytest.mark.parametrize("arch", ["resnet50", "resnext50_32x4d"])
def test_model_logits_vs_fp64(arch, flags, size, models):
    m, x, want = models(arch), images(size), ref_logits(arch, size, flags)
    m.set_input_size(*size)
    m.set_dilation(*flags)
    assert m.dilation == tuple(bool(f) for f in flags) and m.output_stride == 32 >> sum(flags)
    for what, g in three_modes(m, x).items():
        err = float(np.abs(g - want).max())
        print(f"\n  dilation: {arch} {flags} {size} {what}: max|gpu - fp64| = {err:.3e}")
        assert g.shape == (MB, 1000) and err <= TOL, (what, err)
        assert np.array_equal(g.argmax(1), want.argmax(1)), what


def test_degenerate_map(models):
    """32 x 32 with (0,1,1): layer4 runs d = 4 on a 4 x 4 map, all eight outer taps outside everywhere"""
    arch, size, flags = "resnet50", (32, 32), (0, 1, 1)
    m, x, want = models(arch), images(size), ref_logits(arch, size, flags)
    m.set_input_size(*size)
    m.set_dilation(*flags)
    for what, g in three_modes(m, x).items():
        err = float(np.abs(g - want).max())
        print(f"\n  dilation: degenerate map {what}: max|gpu - fp64| = {err:.3e}")
        assert err <= TOL, (what, err)
        assert np.array_equal(g.argmax(1), want.argmax(1)), what


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_nothing_changes_undilated(dtype, finch):
    """logits, arenas, sub-batch and the tuning table of a (0,0,0) model are those of a model that was never told
    about dilation; setting flags and clearing them on a live model returns the first bits"""
    x = np.concatenate([finch, W.generate_input(1, seed=7)])
    state = state_of("resnet50")
    plain = R.NativeModel("resnet50", state=state, dtype=dtype)
    told = R.NativeModel("resnet50", state=state, dtype=dtype, replace_stride_with_dilation=(False, False, False))
    try:
        want = plain.forward(x, fused=True)
        assert plain.dilation == told.dilation == (False, False, False) and plain.output_stride == told.output_stride == 32
        assert np.array_equal(bits(told.forward(x, fused=True)), bits(want))
        es = 4 if dtype == "f32" else 2
        hand = 2 * es * (230 * 230 * 4 + 3 * 112 * 112 * 64 + 2 * 56 * 56 * 128 + 2048)     # test_grouped_gpu.py's sum
        assert plain.activation_bytes() == told.activation_bytes() == hand
        assert plain.max_sub_batch() == told.max_sub_batch() == 512
        if dtype == "f32":
            assert np.array_equal(bits(told.forward(x, fused=False)), bits(plain.forward(x, fused=False)))
        # flags on a live model, then cleared: the first bits, the first arenas
        told.set_dilation(0, 1, 1)
        assert told.activation_bytes() == 0 and told.max_sub_batch() == 256
        other = told.forward(x, fused=True)
        assert told.activation_bytes() > hand
        told.set_dilation(0, 0, 0)
        assert np.array_equal(bits(told.forward(x, fused=True)), bits(want))
        assert told.activation_bytes() == hand and told.max_sub_batch() == 512
        # different flags are a different function: otherwise the comparisons above show nothing
        assert float(np.abs(other - want).max()) > 10 * TOL
        # the tuning table keeps its length and header
        xd = R.FloatTensor.from_numpy(x, R.Device.GPU)
        out = R.FloatTensor((2, 1000), R.Device.GPU)
        plain.tune(xd.data(), 2, out.data(), True)
        words = plain.export_tuning()
        assert words.size == 10 + 4 * (53 + 16)
        told.import_tuning(words)
        assert np.array_equal(told.export_tuning(), words)
        assert np.array_equal(bits(told.forward(x, fused=True)), bits(want))
    finally:
        plain.close()
        told.close()


def test_same_architecture_same_bits_other_flags_other_logits():
    """flags given at construction, set on a live model, or reached through other flags: one architecture, one
    set of bits; different flags differ by far more than the tolerance on these images"""
    size, state = (64, 64), state_of("resnet50")
    x = images(size)
    a = R.NativeModel("resnet50", state=state, input_size=size, replace_stride_with_dilation=(False, True, True))
    b = R.NativeModel("resnet50", state=state, input_size=size)
    try:
        want = a.forward(x, fused=True)
        seen = {(0, 0, 0): b.forward(x, fused=True)}
        for flags in ((1, 1, 1), (0, 0, 1), (0, 1, 1)):
            b.set_dilation(*flags)
            seen[flags] = b.forward(x, fused=True)
        assert np.array_equal(bits(seen[(0, 1, 1)]), bits(want))
        assert np.array_equal(bits(b.forward(x, fused=False)), bits(a.forward(x, fused=False)))
        keys = sorted(seen)
        for i, p in enumerate(keys):
            for q in keys[i + 1:]:
                assert float(np.abs(seen[p] - seen[q]).max()) > 10 * TOL, (p, q)
    finally:
        a.close()
        b.close()


def test_geometry(models):
    arch, flags = "resnet50", (0, 1, 1)
    m = models(arch)
    size = (64, 64)
    m.set_input_size(*size)
    m.set_dilation(*flags)
    assert m.output_stride == 8
    out = m.forward_outputs(images(size), logits=True, features=True)
    feats = ref_features(arch, size, flags)
    assert out["features"].shape == (MB, 2048)
    # the pooled map is the network without its classifier: the whole-network bound, relative to the largest feature
    assert np.abs(out["features"] - feats).max() <= TOL * float(np.abs(feats).max()) + 1e-6
    assert np.abs(out["logits"] - ref_logits(arch, size, flags)).max() <= TOL
    m.set_input_size(224, 224)
    assert m.max_sub_batch() == 256 == 1 << int(np.log2((1 << 29) / 1_605_632))      # layer4's output: 28 * 28 * 2048
    m.forward(W.generate_input(1, seed=2), fused=True)
    # per image: padded input, two ping-pong arenas and the downsample branch of 28 x 28 x 2048, conv1 / conv2
    # outputs of 56 x 56 x 128 (= 28 x 28 x 512), the pooled vector
    assert m.activation_bytes() == 4 * (230 * 230 * 4 + 3 * 28 * 28 * 2048 + 2 * 56 * 56 * 128 + 2048)
    m.set_dilation(0, 0, 0)
    assert m.max_sub_batch() == 512 and m.output_stride == 32


def _rb(a):
    return a.to(torch.float32).to(torch.bfloat16).to(torch.float64)


@torch.no_grad()
def features_bf16_emulated(arch, state, x, flags):
    """features_bf16_emulated of test_grouped_gpu.py with the dilated block table: the roundings of the driver's bf16
    storage (image, weight panels, every stored activation; the pair panel of a stage's first block carries both
    batch-norm scales), float64 sums"""
    t = lambda k: torch.from_numpy(np.asarray(state[k], dtype=np.float64))
    q = lambda k: _rb(t(k))
    groups = W.family_of(arch)[1]
    h = _rb(torch.from_numpy(np.asarray(x, dtype=np.float64)))
    sc, sh = N._fold(state, "bn1")
    h = F.relu(N._affine(F.conv2d(h, q("conv1.weight"), stride=2, padding=3), sc, sh))
    h = _rb(F.max_pool2d(h, 3, 2, 1))
    for pre, _cin, _mid, _cout, s, has_ds, d in W.iter_blocks_dilated(arch, flags):
        sc1, sh1 = N._fold(state, f"{pre}.bn1")
        sc2, sh2 = N._fold(state, f"{pre}.bn2")
        sc3, sh3 = N._fold(state, f"{pre}.bn3")
        y = _rb(F.relu(N._affine(F.conv2d(h, q(f"{pre}.conv1.weight")), sc1, sh1)))
        y = _rb(F.relu(N._affine(F.conv2d(y, q(f"{pre}.conv2.weight"), stride=s, padding=d, dilation=d, groups=groups),
                                 sc2, sh2)))
        if has_ds:
            scd, shd = N._fold(state, f"{pre}.downsample.1")
            w3 = _rb(t(f"{pre}.conv3.weight") * sc3[:, None, None, None])
            wd = _rb(t(f"{pre}.downsample.0.weight") * scd[:, None, None, None])
            z = F.conv2d(y, w3) + F.conv2d(h, wd, stride=s) + (sh3 + shd)[None, :, None, None]
        else:
            z = N._affine(F.conv2d(y, q(f"{pre}.conv3.weight")), sc3, sh3) + h
        h = _rb(F.relu(z))
    return _rb(h.mean(dim=(2, 3))).numpy()


def structured(finch, size):
    """structured() of test_input_size_gpu.py: four images with content, resampled to H x W by nearest neighbour"""
    x = N.structured_inputs(finch)[[0, 5, 8, 12]]
    ih = np.rint(np.linspace(0, 223, size[0])).astype(int)
    iw = np.rint(np.linspace(0, 223, size[1])).astype(int)
    return np.ascontiguousarray(x[:, :, ih][:, :, :, iw])


def test_bf16_within_the_emulations_distance(finch):
    """resnet50 (0,1,1) at 64 x 64 in bf16, fc re-centred to a logit spread of 1: within 2.3 times the distance of
    the CPU emulation of the driver's roundings from the float64 logits (the multiple of test_input_size_gpu.py),
    and that bound below a fifth of the spread.  The three numbers are in profiles/dilation/README.md."""
    arch, size, flags = "resnet50", (64, 64), (0, 1, 1)
    state, x = state_of(arch), structured(finch, size)
    st, want = N.recentre_fc(state, dilated_features_f64(arch, state, x, flags), spread=1.0)
    emu = N.logits_bf16_emulated(st, features_bf16_emulated(arch, st, x, flags))
    dist, spread = float(np.abs(emu - want).max()), N.logit_spread(want)
    bound = 2.3 * dist
    m = R.NativeModel(arch, state=st, dtype="bf16", input_size=size, replace_stride_with_dilation=flags)
    try:
        got = m.forward(x, fused=True)
    finally:
        m.close()
    err = float(np.abs(got - want).max())
    print(f"\n  dilation: bf16 {flags} {size}: emulation {dist:.4f}, bound {bound:.4f}, spread {spread:.3f}, gpu {err:.4f}")
    assert spread > 5 * bound, (bound, spread)      # otherwise the check says nothing
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rescheduling_changes_no_bit(dtype):
    """(0,1,1) at 64 x 64: batch position, streams, the depth-first front, tuning, a captured graph launched twice,
    the host pipeline and the byte route only reschedule the same arithmetic"""
    size, flags = (64, 64), (0, 1, 1)
    m = R.NativeModel("resnet50", state=state_of("resnet50"), dtype=dtype, input_size=size,
                      replace_stride_with_dilation=flags)
    try:
        x5 = W.generate_input(5, seed=41, hw=size)
        base5 = m.forward(x5, fused=True)
        for i in (0, 2, 4):
            assert np.array_equal(bits(m.forward(x5[i:i + 1], fused=True)), bits(base5[i:i + 1])), i
        B = 128
        x = W.generate_input(B, seed=42, hw=size)
        x[7] = x5[2]
        m.set_streams(1)
        want = m.forward(x, fused=True)
        assert np.array_equal(bits(want[7:8]), bits(base5[2:3]))
        m.set_streams(2)
        assert m.parts(B) == 2
        assert np.array_equal(bits(m.forward(x, fused=True)), bits(want))
        m.set_front_parts(4)
        assert np.array_equal(bits(m.forward(x, fused=True)), bits(want))
        m.set_front_parts(1)
        xin = R.FloatTensor.from_numpy(x5, R.Device.GPU)
        out = R.FloatTensor((5, 1000), R.Device.GPU)
        m.tune(xin.data(), 5, out.data(), True)
        m.ctx.sync()
        assert np.array_equal(bits(out.numpy()), bits(base5))
        assert np.array_equal(bits(m.forward(x5, fused=True)), bits(base5))
        xd = R.FloatTensor.from_numpy(x[:8], R.Device.GPU)
        o8 = R.FloatTensor((8, 1000), R.Device.GPU)
        g = R.Graph(m, xd.data(), 8, o8.data(), fused=True)
        L.check(L.lib().rn_memset(m.ctx.handle, o8.data(), 0, 8 * 4000), "memset", m.ctx.handle)
        g.launch(); g.launch(); m.ctx.sync()
        assert np.array_equal(bits(o8.numpy()), bits(want[:8]))
        g.close()
        pipe = R.Pipeline(m, 16, fused=True)
        got = list(pipe.run([x[:16], x[16:32]]))
        pipe.close()
        assert np.array_equal(bits(got[0]), bits(want[:16])) and np.array_equal(bits(got[1]), bits(want[16:32]))
        px = np.random.default_rng(9).integers(0, 256, (3,) + size + (3,), dtype=np.uint8)
        assert np.array_equal(bits(m.forward_u8(px, fused=True)), bits(m.forward(preprocess.normalize_u8(px), fused=True)))
    finally:
        m.close()


def test_decoded_images_on_a_dilated_model(models):
    """rn_model_forward_images_u8's contract is the 224 crop only: on a (0,0,1) model it is forward_u8 on the crops"""
    m = models("resnet50")
    m.set_input_size(224, 224)
    m.set_dilation(0, 0, 1)
    try:
        img = np.random.default_rng(5).integers(0, 256, (300, 280, 3), dtype=np.uint8)
        got = m.forward_images([img])
        assert got.shape == (1, 1000) and np.isfinite(got).all()
        m.set_dilation(0, 0, 0)
        assert float(np.abs(m.forward_images([img]) - got).max()) > 10 * TOL
    finally:
        m.set_dilation(0, 0, 0)


def test_model_refusals():
    size = (64, 64)
    r18 = R.NativeModel("resnet18", state=state_of("resnet18"))
    try:
        with pytest.raises(R.RnError) as e:
            r18.set_dilation(0, 0, 1)
        assert e.value.status == L.RN_ERR_UNSUPPORTED and "bottleneck" in str(e.value)
        assert r18.dilation == (False, False, False) and r18.output_stride == 32
    finally:
        r18.close()
    m = R.NativeModel("resnet50", state=state_of("resnet50"), input_size=size)
    try:
        assert L.lib().rn_model_set_dilation(m.handle, 0, 2, 0) == L.RN_ERR_INVALID
        assert L.lib().rn_model_set_dilation(m.handle, -1, 0, 0) == L.RN_ERR_INVALID
        x = images(size)[:2]
        first = m.forward(x, fused=True)
        xd = R.FloatTensor.from_numpy(x, R.Device.GPU)
        out = R.FloatTensor((2, 1000), R.Device.GPU)
        g = R.Graph(m, xd.data(), 2, out.data(), True)
        with pytest.raises(R.RnError) as e:
            m.set_dilation(0, 1, 1)
        assert e.value.status == L.RN_ERR_INVALID and m.dilation == (False, False, False)
        g.launch()
        m.ctx.sync()
        assert np.array_equal(bits(out.numpy()), bits(first))
        g.close()
        pipe = R.Pipeline(m, 2, fused=True)
        with pytest.raises(R.RnError):
            m.set_dilation(0, 1, 1)
        assert m.dilation == (False, False, False)
        pipe.close()
        assert np.array_equal(bits(m.forward(x, fused=True)), bits(first))
        # tuning tables carry the flags
        m.tune(xd.data(), 2, out.data(), True)
        t000 = m.export_tuning()
        m.set_dilation(0, 1, 1)
        with pytest.raises(R.RnError):
            m.export_tuning()              # the flags dropped the tiles
        with pytest.raises(R.RnError):
            m.import_tuning(t000)
        want = m.forward(x, fused=True)
        m.tune(xd.data(), 2, out.data(), True)
        assert np.array_equal(bits(out.numpy()), bits(want))       # tiles change no bit
        t011 = m.export_tuning()
        assert t011.size == t000.size + 1
        m.set_dilation(0, 0, 1)
        with pytest.raises(R.RnError):
            m.import_tuning(t011)          # (0,1,1) is not (0,0,1)
        m.set_dilation(0, 0, 0)
        with pytest.raises(R.RnError):
            m.import_tuning(t011)
        m.import_tuning(t000)
        m.set_dilation(0, 1, 1)
        m.import_tuning(t011)
        assert np.array_equal(bits(m.forward(x, fused=True)), bits(want))
    finally:
        m.close()


@pytest.mark.parametrize("arch,flags", [("resnet50", (0, 1, 1)), ("resnext50_32x4d", (1, 1, 1))])
def test_profile_flops(arch, flags, models):
    size = (96, 64)
    m = models(arch)
    m.set_input_size(*size)
    m.set_dilation(*flags)
    for fused in (True, False):
        m.set_profiling(True)
        try:
            m.forward(images(size)[:1], fused=fused)
            recs = m.profile()
        finally:
            m.set_profiling(False)
        assert int(round(sum(r["flops"] for r in recs))) == W.forward_flops(arch, size, replace_stride_with_dilation=flags)


def test_rn_infer_dilate(tmp_path, models):
    size, flags = (64, 64), (0, 1, 1)
    wdir = tmp_path / "weights_bin"
    os.mkdir(wdir)
    W.save_weights_bin(state_of("resnet50"), str(wdir))
    x = images(size)[:2]
    inp = tmp_path / "in_64x64.bin"
    np.ascontiguousarray(x).tofile(inp)
    m = models("resnet50")
    m.set_input_size(*size)
    m.set_dilation(*flags)
    want = m.forward(x, fused=True).argmax(1)
    exe = os.path.join(os.path.dirname(L.LIB_PATH), "rn_infer")
    base = [exe, "--weights", str(wdir), "--batch", "2", "--size", "64,64", "--input", str(inp)]
    r = subprocess.run(base + ["--arch", "50", "--dilate", "0,1,1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [int(l.split()[-1]) for l in r.stdout.splitlines() if l.startswith("max index is")] == want.tolist()
    r = subprocess.run(base + ["--arch", "18", "--dilate", "0,1,1"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "unsupported" in r.stderr and "bottleneck" in r.stderr, r.stderr
    r = subprocess.run(base + ["--arch", "50", "--dilate", "0,2,1"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--dilate" in r.stderr, r.stderr
