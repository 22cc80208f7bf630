"""Feature pyramid neck on the GPU: the top-down launch on views between guard bands, the neck alone against its
float64 reference, and the model route (rn_model_forward_fpn) against the same reference on the model's own stage maps.

Bounds are the project's: tol_f32(ref, K) with K = the products that reach an output (test_fpn_host.products; the host
test shows torch's own fp32 execution inside it) and tol_bf16(ref) against a reference rounded where the device stores
bf16.  Everything that only reschedules -- parts, streams, front slices, sub-batches, batch position, the byte route --
is held to the same bits.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_c_amd as R
import views as V
from resnet_c_amd import _lib as L
from resnet_c_amd import fpn as P
from resnet_c_amd import ops, preprocess
from resnet_c_amd import weights as W
from test_dilation_gpu import bits, state_of, tol_bf16, tol_f32
from test_fpn_host import GEOMETRIES, NECKS, neck_maps, neck_state, products

pytestmark = pytest.mark.gpu

DT = {"f32": L.RN_DTYPE_F32, "bf16": L.RN_DTYPE_BF16}
NP = {"f32": np.float32, "bf16": np.uint16}
NAME = "rn_upsample_nearest_add_forward_dt"


def launches(ctx=None):
    return int(L.lib().rn_ctx_launch_count((ctx or R.get_ctx()).handle))


def typed(a, dtype):
    """fp32 host values as the kernel's element type: fp32 as they are, bf16 as rounded bit patterns"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if dtype == "f32" else ops.to_bf16_bits(a).reshape(a.shape)


def run_op(top, lat, size, dtype, inplace=False):
    """one launch on views between guard bands: every guard intact, dst written everywhere; returns dst"""
    B, h, w, C = top.shape
    H, Wd = size
    es = np.dtype(NP[dtype]).itemsize
    vt = V.place(top)
    vl = V.place(lat) if lat is not None else None
    vd = vl if inplace else V.place_out(B * H * Wd * C * es)
    before = launches()
    V.must(NAME, DT[dtype], vt.ptr, B, h, w, C, vl.ptr if vl else None, vd.ptr, H, Wd)
    assert launches() == before + 1
    V.check_guards(f"{NAME} inputs", vt, None if inplace else vl)
    assert np.array_equal(V.fetch(vt, np.uint8, "top"), top.reshape(-1).view(np.uint8))     # the source's bytes stay
    return V.fetch(vd, NP[dtype], f"{NAME} dst", written=not inplace).reshape(B, H, Wd, C)


# =====================================================================================================================
# 1. the kernel
# =====================================================================================================================
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}to{g[1][0]}x{g[1][1]}")
def test_op_is_the_contract_bit_for_bit(geom, dtype):
    (h, w), (H, Wd) = geom
    unit = 4 if dtype == "f32" else 8          # one 16-byte chunk; 72: no multiple of a wave's 64 lanes either way
    for C in (unit, 64, 72):
        for B in (1, 3):
            rng = np.random.default_rng(C * 100 + B + h * 7 + H)
            top = typed(rng.standard_normal((B, h, w, C)), dtype)
            lat = typed(rng.standard_normal((B, H, Wd, C)), dtype)
            want = ops.upsample_nearest_add_ref(top, lat)
            V.assert_no_poison(want if dtype == "f32" else ops.from_bf16_bits(want), dtype == "bf16", "reference")
            if dtype == "f32":       # torch itself, not only its restatement
                up = F.interpolate(torch.from_numpy(top).permute(0, 3, 1, 2), size=(H, Wd), mode="nearest")
                assert np.array_equal(bits((torch.from_numpy(lat) + up.permute(0, 2, 3, 1)).numpy()), bits(want))
            got = run_op(top, lat, (H, Wd), dtype)
            assert np.array_equal(got, want) if dtype == "bf16" else np.array_equal(bits(got), bits(want)), (C, B)
            same = run_op(top, lat, (H, Wd), dtype, inplace=True)
            assert np.array_equal(same.view(np.uint8), got.view(np.uint8)), ("in place", C, B)
            plain = run_op(top, None, (H, Wd), dtype)
            assert np.array_equal(plain, ops.upsample_nearest_add_ref(top, size=(H, Wd))), ("lat NULL", C, B)


def test_op_more_than_one_block_and_long_pixels():
    """rows of more than one block's span, a pixel longer than a block's trip (C = 8192 fp32: 2048 chunks), more rows
    than the grid has in y"""
    for (B, h, w, C), (H, Wd) in (((1, 3, 70, 64), (5, 139)), ((1, 2, 2, 8192), (3, 3)), ((2, 1100, 1, 4), (2200, 2))):
        rng = np.random.default_rng(C + H)
        top = rng.standard_normal((B, h, w, C)).astype(np.float32)
        lat = rng.standard_normal((B, H, Wd, C)).astype(np.float32)
        assert np.array_equal(bits(run_op(top, lat, (H, Wd), "f32")), bits(ops.upsample_nearest_add_ref(top, lat)))


def test_op_python_wrappers():
    rng = np.random.default_rng(5)
    top = rng.standard_normal((2, 3, 2, 8)).astype(np.float32)
    lat = rng.standard_normal((2, 5, 3, 8)).astype(np.float32)
    assert np.array_equal(bits(ops.upsample_nearest_add(top, lat)), bits(ops.upsample_nearest_add_ref(top, lat)))
    assert np.array_equal(bits(ops.upsample_nearest_add(top, size=(7, 7))), bits(ops.upsample_nearest_add_ref(top, size=(7, 7))))
    tb, lb = ops.to_bf16_bits(top).reshape(top.shape), ops.to_bf16_bits(lat).reshape(lat.shape)
    assert np.array_equal(ops.upsample_nearest_add_bf16(tb, lb), ops.upsample_nearest_add_ref(tb, lb))


def test_op_special_values_fp32():
    """lat == NULL is a copy: NaN payloads and -0.0 arrive as they are; the add is IEEE's"""
    pat = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000001],
                   dtype=np.uint32)
    top = np.tile(pat, 2 * 2 * 3).reshape(2, 2, 3, 8).view(np.float32)
    got = run_op(top, None, (4, 5), "f32")
    assert np.array_equal(bits(got), bits(ops.upsample_nearest_add_ref(top, size=(4, 5))))
    assert np.array_equal(bits(got[0, 0, 0]), pat)
    inf = np.float32(np.inf)
    t = np.array([inf, inf, -inf, np.float32(-0.0), np.float32(-0.0), np.float32(1.0), inf, np.float32(3e38)],
                 dtype=np.float32).reshape(1, 1, 1, 8)
    a = np.array([np.float32(1.0), -inf, inf, np.float32(-0.0), np.float32(0.0), np.float32(-1.0), inf, np.float32(3e38)],
                 dtype=np.float32).reshape(1, 1, 1, 8)
    out = run_op(t, np.tile(a, (1, 2, 2, 1)), (2, 2), "f32")[0, 1, 1]
    assert out[0] == inf and np.isnan(out[1]) and np.isnan(out[2])
    assert bits(out[3:4])[0] == 0x80000000 and bits(out[4:5])[0] == 0 and bits(out[5:6])[0] == 0
    assert out[6] == inf and out[7] == inf


def test_op_bf16_half_ulp_ties():
    """sums that are exact in fp32 and lie halfway between two bf16 values: to the even neighbour, once"""
    ulp, half = 2.0 ** -7, 2.0 ** -8
    lat_v = np.array([1.0, 1.0 + ulp, -1.0, -1.0 - ulp, 2.0, 1.0, 256.0, 0.5], dtype=np.float32)
    top_v = np.array([half, half, -half, -half, 2 * half, 3 * half, 1.0, half / 2], dtype=np.float32)
    assert np.array_equal(ops.bf16_round(lat_v), lat_v) and np.array_equal(ops.bf16_round(top_v), top_v)
    top = ops.to_bf16_bits(top_v).reshape(1, 1, 1, 8)
    lat = np.tile(ops.to_bf16_bits(lat_v).reshape(1, 1, 1, 8), (1, 3, 2, 1))
    want = ops.upsample_nearest_add_ref(top, lat)
    exact = lat_v.astype(np.float64) + top_v.astype(np.float64)
    assert np.array_equal((lat_v + top_v).astype(np.float64), exact)                 # fp32 holds every sum exactly
    assert np.all(ops.bf16_round((lat_v + top_v)).astype(np.float64) != exact)       # and none of them is a bf16 value
    assert ops.from_bf16_bits(want[0, 0, 0]).tolist() == [1.0, 1.0 + 2 * ulp, -1.0, -1.0 - 2 * ulp, 2.0, 1.0 + 2 * ulp, 256.0,
                                                         0.5]
    assert np.array_equal(run_op(top, lat, (3, 2), "bf16"), want)


def test_op_refusals_launch_nothing():
    lib, ctx = L.lib(), R.get_ctx()
    B, h, w, C, H, Wd = 2, 2, 3, 8, 4, 6
    top = np.ones((B, h, w, C), np.float32)
    vt, vl, vd = V.place(top), V.place(np.ones((B, H, Wd, C), np.float32)), V.place_out(B * H * Wd * C * 4)
    f32 = L.RN_DTYPE_F32
    good = (f32, vt.ptr, B, h, w, C, vl.ptr, vd.ptr, H, Wd)

    def but(**kw):
        names = ("dtype", "top", "B", "h", "w", "C", "lat", "dst", "H", "W")
        return tuple(kw.get(n, v) for n, v in zip(names, good))

    big = V.place(np.ones((B * H * Wd * C,), np.float32))
    cases = [(but(top=None), "top_nhwc"), (but(dst=None), "dst_nhwc"), (but(h=0), ">= 1"), (but(W=0), ">= 1"),
             (but(C=6), "C must"), (but(C=0), "C must"), (but(dtype=L.RN_DTYPE_BF16, C=12), "C must"),
             (but(top=vt.ptr + 4), "top_nhwc"), (but(lat=vl.ptr + 8), "lat_nhwc"), (but(dst=vd.ptr + 4), "dst_nhwc"),
             (but(dtype=7), "dtype"), (but(top=big.ptr, dst=big.ptr + 16, lat=None), "overlaps top"),
             (but(lat=big.ptr, dst=big.ptr + 16 * C), "overlaps lat"), (but(B=1 << 31), "2^31"),
             (but(H=1 << 16, W=1 << 16), "2^31")]
    before = launches()
    for args, word in cases:
        st, msg = V.call(NAME, *args)
        assert st == L.RN_ERR_INVALID and word in msg and NAME in msg, (word, st, msg)
    assert lib.rn_upsample_nearest_add_forward_dt(None, *good) == L.RN_ERR_INVALID
    st, msg = V.call(NAME, *but(B=0))
    assert st == L.RN_OK
    assert launches() == before
    ctx.sync()
    V.assert_untouched(vd, "refused calls"), V.assert_untouched(vl, "refused calls"), V.assert_untouched(big, "refused calls")
    V.must(NAME, *good)                                   # and the call they all almost were
    assert launches() == before + 1


# =====================================================================================================================
# 2. the neck alone
# =====================================================================================================================
@pytest.fixture(scope="module")
def necks():
    made = {}

    def get(name, dtype):
        if (name, dtype) not in made:
            cin, a, extra = NECKS[name]
            made[(name, dtype)] = P.FeaturePyramidNetwork(cin, a, neck_state(name), extra=extra, dtype=dtype)
        return made[(name, dtype)]
    yield get
    for n in made.values():
        n.close()


def check_levels(got, ref, cin, a, dtype, what):
    for i in range(len(cin)):
        g, r = got[str(i)], ref[str(i)]
        assert g.shape == r.shape and g.dtype == np.float32, (what, i, g.shape, r.shape)
        tol = tol_f32(r, products(cin, a, i)) if dtype == "f32" else tol_bf16(r)
        err = float(np.abs(g - r).max())
        print(f"\n  fpn {what} {dtype}: level {i}: max error {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (what, i, err, tol)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(NECKS))
def test_neck_alone(necks, name, dtype):
    cin, a, extra = NECKS[name]
    neck = necks(name, dtype)
    maps = neck_maps(name)
    nhwc = [np.ascontiguousarray(m.transpose(0, 2, 3, 1)) for m in maps]
    ref = P.fpn_ref([m.astype(np.float64) for m in maps], neck_state(name), extra,
                    round_fn=ops.bf16_round if dtype == "bf16" else None)
    got = neck.forward(nhwc)
    assert list(got) == list(ref) == list(neck.names)
    check_levels(got, ref, cin, a, dtype, name)
    last = str(len(cin) - 1)
    if extra:
        assert got["pool"].shape == ref["pool"].shape
        assert np.array_equal(bits(got["pool"]), bits(got[last][:, :, ::2, ::2]))
    again = neck.forward(nhwc)
    assert all(np.array_equal(bits(again[k]), bits(got[k])) for k in got)
    wanted = ("0", "pool") if extra else ("1",)       # the others still run their laterals and top-down steps
    some = neck.forward(nhwc, levels=wanted)
    assert list(some) == list(wanted) and all(np.array_equal(bits(some[k]), bits(got[k])) for k in wanted)
    one = neck.forward([m[1:2] for m in nhwc])        # an image alone
    assert all(np.array_equal(bits(one[k][0]), bits(got[k][1])) for k in got)


def test_neck_refusals():
    lib, ctx = L.lib(), R.get_ctx()
    raw = ctypes.c_void_p()

    def create(cin, a=64, extra=1):
        arr = (ctypes.c_uint64 * len(cin))(*cin)
        st = lib.rn_fpn_create(ctx.handle, ctypes.byref(raw), len(cin), arr, a, extra)
        return st, (lib.rn_last_error(ctx.handle) or b"").decode()

    for cin, a, extra, word in (((64, 96), 64, 1, "multiple of 64"), ((64, 64, 64, 64, 64), 64, 1, "n_levels"), ((), 64, 1, "n_levels"),
                                ((64,), 96, 1, "out_channels"), ((64,), 2048, 1, "out_channels"), ((64,), 64, 2, "extra")):
        st, msg = create(cin or (64,), a, extra) if cin else (lib.rn_fpn_create(ctx.handle, ctypes.byref(raw), 0, None, a, extra),
                                                              (lib.rn_last_error(ctx.handle) or b"").decode())
        assert st == L.RN_ERR_INVALID and word in msg and not raw.value, (word, st, msg)
    st, msg = create((64, 128), 64, 1)
    assert st == L.RN_OK, msg
    try:
        state = P.generate_fpn_state((64, 128), 64)
        w = state["inner_blocks.1.0.weight"]

        def set_tensor(key, arr, numel=None):
            st = lib.rn_fpn_set_tensor(raw, key.encode(), arr.ctypes.data, arr.size if numel is None else numel)
            return st, (lib.rn_last_error(ctx.handle) or b"").decode()

        for key in ("inner_blocks.2.0.weight", "inner_blocks.1.0.gamma", "layer_blocks.0.1.weight", "classifier.0.weight"):
            st, msg = set_tensor(key, w)
            assert st == L.RN_ERR_INVALID and "unknown key" in msg and key in msg, (key, st, msg)
        st, msg = set_tensor("inner_blocks.1.0.weight", w, w.size - 1)
        assert st == L.RN_ERR_INVALID and "inner_blocks.1.0.weight" in msg and "elements" in msg
        assert set_tensor("inner_blocks.1.weight", w)[0] == L.RN_OK                  # the older spelling
        x = ops._up_raw(np.zeros((1, 2, 2, 128), np.float32))
        out = V.place_out(64 * 4 * 4)
        xs, outs = (ctypes.c_void_p * 2)(x.ptr, x.ptr), (ctypes.c_void_p * 3)(out.ptr, None, None)
        hw = (ctypes.c_uint64 * 2)(2, 2)
        before = launches()
        assert lib.rn_fpn_forward(raw, xs, 1, hw, hw, outs) == L.RN_ERR_INVALID      # before finalize
        assert "not finalized" in (lib.rn_last_error(ctx.handle) or b"").decode()
        assert lib.rn_fpn_finalize(raw) == L.RN_ERR_INVALID                          # not every tensor is set
        assert "is not set" in (lib.rn_last_error(ctx.handle) or b"").decode()
        assert launches() == before
        ctx.sync()
        V.assert_untouched(out, "refused neck calls")
    finally:
        lib.rn_fpn_destroy(raw)


# =====================================================================================================================
# 3. the model route
# =====================================================================================================================
SIZE, MB = (72, 40), 3          # stage maps 18x10, 9x5, 5x3, 3x2
WIDTH = {"resnet18": 64, "resnet50": 256}      # out_channels of the model tests' necks (256: torchvision's)


@functools.lru_cache(maxsize=None)
def images(size=SIZE, n=MB):
    x = W.generate_input(n, seed=300 + size[0] + size[1], hw=size)
    x.setflags(write=False)
    return x


def stage_channels(arch):
    return (64, 128, 256, 512) if arch == "resnet18" else (256, 512, 1024, 2048)


@functools.lru_cache(maxsize=None)
def model_neck_state(arch, first=0):
    return P.generate_fpn_state(stage_channels(arch)[first:], WIDTH[arch], seed=1)


@pytest.fixture(scope="module")
def nets():
    made, extra_necks = {}, []

    def get(arch="resnet50", dtype="f32"):
        if (arch, dtype) not in made:
            m = R.NativeModel(arch, state=state_of(arch), dtype=dtype, input_size=SIZE)
            made[(arch, dtype)] = (m, P.FeaturePyramidNetwork(stage_channels(arch), WIDTH[arch], model_neck_state(arch),
                                                              dtype=dtype))
        m, neck = made[(arch, dtype)]
        m.set_streams(0)
        return m, neck
    get.keep = extra_necks.append
    yield get
    for n in extra_necks:
        n.close()
    for m, neck in made.values():
        neck.close()
        m.close()


def check_against_ref(m, neck, x, dtype, stages=R.NativeModel.STAGES, state=None, what=""):
    """forward_fpn against fpn_ref on the stage maps the same model returns for the same images"""
    maps = m.forward_maps(x, stages)
    ref = P.fpn_ref([maps[s].astype(np.float64) for s in stages], state or model_neck_state(m.arch), "pool",
                    round_fn=ops.bf16_round if dtype == "bf16" else None)
    got = m.forward_fpn(x, neck, stages)
    assert list(got) == list(ref) == list(neck.names)
    check_levels(got, ref, neck.in_channels_list, neck.out_channels, dtype, f"{m.arch} {what}")
    last = str(len(stages) - 1)
    assert np.array_equal(bits(got["pool"]), bits(got[last][:, :, ::2, ::2]))
    return got


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_model_pyramid(nets, arch, dtype):
    m, neck = nets(arch, dtype)
    assert [m.stage_shapes[s][1:] for s in m.STAGES] == [(18, 10), (9, 5), (5, 3), (3, 2)]
    got = check_against_ref(m, neck, images(), dtype, what="72x40")
    assert [got[k].shape for k in got] == [(MB, WIDTH[arch], 18, 10), (MB, WIDTH[arch], 9, 5), (MB, WIDTH[arch], 5, 3),
                                          (MB, WIDTH[arch], 3, 2), (MB, WIDTH[arch], 2, 1)]
    again = m.forward_fpn(images(), neck)
    assert all(np.array_equal(bits(again[k]), bits(got[k])) for k in got)


def test_model_exact_2x_and_equal_sizes(nets):
    m, neck = nets()
    try:
        m.set_input_size(64, 64)
        assert [m.stage_shapes[s][1:] for s in m.STAGES] == [(16, 16), (8, 8), (4, 4), (2, 2)]
        check_against_ref(m, neck, images((64, 64)), "f32", what="64x64")
        m.set_input_size(*SIZE)
        m.set_dilation(False, True, True)
        assert [m.stage_shapes[s][1:] for s in m.STAGES] == [(18, 10), (9, 5), (9, 5), (9, 5)]
        check_against_ref(m, neck, images(), "f32", what="dilated (0,1,1)")
    finally:
        m.set_dilation(False, False, False)
        m.set_input_size(*SIZE)


def test_model_three_levels(nets):
    m, _ = nets()
    state = model_neck_state("resnet50", 1)
    neck3 = P.FeaturePyramidNetwork(stage_channels("resnet50")[1:], 256, state)
    nets.keep(neck3)
    stages = ("layer2", "layer3", "layer4")
    got = check_against_ref(m, neck3, images(), "f32", stages, state, what="layer2..4")
    assert list(got) == ["0", "1", "2", "pool"] and got["0"].shape == (MB, 256, 9, 5)
    some = m.forward_fpn(images(), neck3, stages, levels=("1", "pool"))
    assert list(some) == ["1", "pool"] and all(np.array_equal(bits(some[k]), bits(got[k])) for k in some)
    for bad in (("layer1", "layer2"), ("layer3", "layer2", "layer4"), ("layer2", "layer2", "layer4"), ("layer2", "layer3", "fc")):
        with pytest.raises(ValueError):
            m.forward_fpn(images(), neck3, bad)
    with pytest.raises(ValueError):
        m.forward_fpn(images(), neck3, stages, levels=("3",))


def test_model_other_outputs_keep_their_bits(nets):
    m, neck = nets()
    x = images()
    want = m.forward_outputs(x, logits=True, features=True, probs=True, topk=5)
    got = m.forward_fpn(x, neck, logits=True, features=True, probs=True, topk=5)
    assert list(got) == ["0", "1", "2", "3", "pool", "logits", "features", "probs", "topk_prob", "topk_idx"]
    for k in ("logits", "features", "probs", "topk_prob"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.array_equal(got["topk_idx"], want["topk_idx"])
    pyramid = m.forward_fpn(x, neck)
    assert all(np.array_equal(bits(pyramid[k]), bits(got[k])) for k in pyramid)
    # the request does not outlive its call: a plain forward issues the launches it always did, and its bits
    before = launches(m.ctx)
    a = m.forward(x)
    plain = launches(m.ctx) - before
    assert np.array_equal(bits(a), bits(want["logits"]))
    before = launches(m.ctx)
    m.forward_fpn(x, neck, levels=("0",))
    assert launches(m.ctx) - before > plain
    before = launches(m.ctx)
    assert np.array_equal(bits(m.forward(x)), bits(a))
    assert launches(m.ctx) - before == plain


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_rescheduling_changes_no_bit(nets, dtype):
    m, neck = nets("resnet50", dtype)
    x = images()
    base = m.forward_fpn(x, neck)
    for i in range(MB):                               # one call of three images against three calls of one
        one = m.forward_fpn(x[i:i + 1], neck)
        assert all(np.array_equal(bits(one[k][0]), bits(base[k][i])) for k in base), i
    moved = m.forward_fpn(x[[2, 0]], neck)
    assert all(np.array_equal(bits(moved[k]), bits(base[k][[2, 0]])) for k in base)
    px = np.random.default_rng(9).integers(0, 256, (MB,) + SIZE + (3,), dtype=np.uint8)
    a = m.forward_fpn_u8(px, neck)
    b = m.forward_fpn(preprocess.normalize_u8(px), neck)
    assert list(a) == list(b) and all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


def test_model_parts_on_two_streams(nets):
    """128 images as two parts of 64 on two streams, each in its own slice of the neck's scratch, then with the front
    (stem .. layer1, and with it the lateral behind layer1) in four slices of a part: the bits of one stream, and of
    the three-image call for the images they share"""
    m, neck = nets()
    x = W.generate_input(128, seed=300 + SIZE[0] + SIZE[1], hw=SIZE)
    assert np.array_equal(x[:MB], images())
    try:
        m.set_streams(1)
        one = m.forward_fpn(x, neck)
        m.set_streams(2)
        assert m.parts(128) == 2
        two = m.forward_fpn(x, neck)
        m.set_front_parts(4)
        sliced = m.forward_fpn(x, neck)
    finally:
        m.set_front_parts(1)
        m.set_streams(0)
    for k in one:
        assert np.array_equal(bits(two[k]), bits(one[k])), k
        assert np.array_equal(bits(sliced[k]), bits(one[k])), k
    few = m.forward_fpn(images(), neck)
    assert all(np.array_equal(bits(few[k]), bits(one[k][:MB])) for k in few)


def test_model_two_sub_batches(nets):
    """one image more than a launch batch holds: the second sub-batch reuses the neck's scratch behind the first"""
    m, neck = nets("resnet18")
    try:
        m.set_input_size(32, 32)
        cap = m.max_sub_batch()
        x = W.generate_input(cap + 1, seed=43, hw=(32, 32))
        whole = m.forward_fpn(x, neck, levels=("1", "3", "pool"))
        first, last = m.forward_fpn(x[:cap], neck, levels=("1", "3", "pool")), m.forward_fpn(x[cap:], neck, levels=("1", "3", "pool"))
        for k in whole:
            assert np.array_equal(bits(whole[k][:cap]), bits(first[k])) and np.array_equal(bits(whole[k][cap:]), bits(last[k])), k
    finally:
        m.set_input_size(*SIZE)


def test_profile_records(nets):
    m, neck = nets()
    x = images()
    m.forward_fpn(x, neck)
    m.set_profiling(True)
    try:
        m.forward_outputs(x, logits=True)
        plain = m.profile()
        m.forward_fpn(x, neck)
        recs = m.profile()
        m.forward_fpn(x, neck, levels=("1", "pool"))
        some = m.profile()
    finally:
        m.set_profiling(False)
    mine = [r for r in recs if r["layer"] == "fpn"]
    assert [r["op"] for r in mine] == (["fpn_inner0", "fpn_inner1", "fpn_inner2", "fpn_inner3", "fpn_topdown3", "fpn_topdown2",
                                       "fpn_topdown1", "fpn_layer0", "fpn_layer1", "fpn_layer2", "fpn_layer3", "fpn_pool",
                                       "fpn_export0", "fpn_export1", "fpn_export2", "fpn_export3", "fpn_export_pool"])
    assert all(r["ms"] > 0 for r in mine)
    by = {r["op"]: r for r in mine}
    assert by["fpn_inner0"]["flops"] == 2.0 * MB * 18 * 10 * 256 * 256 and by["fpn_layer3"]["flops"] == 2.0 * MB * 3 * 2 * 9 * 256 * 256
    assert by["fpn_topdown1"]["flops"] == 0 and by["fpn_topdown1"]["bytes"] == 4.0 * 256 * MB * (9 * 5 + 2 * 18 * 10)
    assert [r["op"] for r in some if r["layer"] == "fpn"] == ["fpn_inner0", "fpn_inner1", "fpn_inner2", "fpn_inner3", "fpn_topdown3",
                                                             "fpn_topdown2", "fpn_topdown1", "fpn_layer1", "fpn_layer3", "fpn_pool",
                                                             "fpn_export1", "fpn_export_pool"]
    rest = [(r["op"], r["layer"]) for r in recs if r["layer"] != "fpn"]
    assert rest == [(r["op"], r["layer"]) for r in plain]
    # the lateral of a stage sits right behind the stage: before the first record of the next stage's blocks
    layers = [r["layer"] for r in recs]
    ops_ = [r["op"] for r in recs]
    for i in range(3):
        first_next = next(j for j, name in enumerate(layers) if name.startswith(f"layer{i + 2}"))
        last_this = max(j for j, name in enumerate(layers) if name.startswith(f"layer{i + 1}"))
        assert last_this < ops_.index(f"fpn_inner{i}") < first_next, i
    assert ops_.index("fpn_inner3") == ops_.index("fpn_topdown3") - 1


def test_model_refusals(nets):
    m, neck = nets()
    m18, neck18 = nets("resnet18")
    mb, neckb = nets("resnet50", "bf16")
    lib = L.lib()
    x = ops._up_raw(images())
    out = V.place_out(MB * 256 * 18 * 10 * 4)
    fo = L.FpnOutputs()
    fo.level[0] = out.ptr
    off = L.FpnOutputs()
    off.level[0] = out.ptr + 2
    raw = ctypes.c_void_p()
    cin = (ctypes.c_uint64 * 4)(256, 512, 1024, 2048)
    assert lib.rn_fpn_create(m.ctx.handle, ctypes.byref(raw), 4, cin, 256, 1) == L.RN_OK   # never finalized
    asc = (ctypes.c_int * 4)(1, 2, 3, 4)

    def call(model, nk, stages, fo_ptr, mode=L.RN_FWD_FUSED):
        st = lib.rn_model_forward_fpn(model.handle, nk, x.ptr, MB, None, stages, fo_ptr, mode)
        return st, (lib.rn_last_error(model.ctx.handle) or b"").decode()

    try:
        before, before_b = launches(m.ctx), launches(mb.ctx)
        for nk, stages, fo_ptr, word in ((None, asc, ctypes.byref(fo), "neck is NULL"), (raw, asc, ctypes.byref(fo), "not finalized"),
                                         (neckb.handle, asc, ctypes.byref(fo), "dtype"),
                                         (neck.handle, (ctypes.c_int * 4)(1, 3, 2, 4), ctypes.byref(fo), "ascending"),
                                         (neck.handle, (ctypes.c_int * 4)(1, 2, 2, 4), ctypes.byref(fo), "ascending"),
                                         (neck.handle, (ctypes.c_int * 4)(0, 1, 2, 3), ctypes.byref(fo), "1..4"),
                                         (neck.handle, (ctypes.c_int * 4)(2, 3, 4, 5), ctypes.byref(fo), "1..4"),
                                         (neck.handle, None, ctypes.byref(fo), "stages is NULL"),
                                         (neck18.handle, asc, ctypes.byref(fo), "in_channels"),
                                         (neck.handle, asc, None, "fpn_out is NULL"),
                                         (neck.handle, asc, ctypes.byref(L.FpnOutputs()), "nothing wanted"),
                                         (neck.handle, asc, ctypes.byref(off), "4-byte aligned")):
            st, msg = call(m, nk, stages, fo_ptr)
            assert st == L.RN_ERR_INVALID and word in msg, (word, st, msg)
        assert lib.rn_model_forward_fpn(None, neck.handle, x.ptr, MB, None, asc, ctypes.byref(fo), L.RN_FWD_FUSED) == L.RN_ERR_INVALID
        st, msg = call(mb, neckb.handle, asc, ctypes.byref(fo), L.RN_FWD_REFERENCE_OPS)
        assert st == L.RN_ERR_UNSUPPORTED and "bf16" in msg, (st, msg)
        assert launches(m.ctx) == before and launches(mb.ctx) == before_b
        m.ctx.sync()
        V.assert_untouched(out, "refused pyramid calls")
        with pytest.raises(ValueError):
            m.forward_fpn(images(), neck, ("layer2", "layer3", "layer4"))         # three stages, a neck of four levels
        st, msg = call(m, neck.handle, asc, ctypes.byref(fo))                     # and the call they all almost were
        assert st == L.RN_OK, msg
        m.ctx.sync()
        want = m.forward_fpn(images(), neck, levels=("0",))["0"]
        assert np.array_equal(bits(V.fetch(out, np.float32, "level 0", written=True).reshape(want.shape)), bits(want))
    finally:
        lib.rn_fpn_destroy(raw)


def test_model_op_by_op_backbone(nets):
    """RN_FWD_REFERENCE_OPS: behind a stage's last block the arena holds the finished output (batch-norm, add and
    ReLU are launches of their own there) where the lateral reads it -- the pyramid against fpn_ref on that mode's maps"""
    m, neck = nets()
    maps = m.forward_maps(images(), fused=False)
    ref = P.fpn_ref([maps[s].astype(np.float64) for s in m.STAGES], model_neck_state(m.arch), "pool")
    got = m.forward_fpn(images(), neck, fused=False)
    assert list(got) == list(neck.names)
    check_levels(got, ref, neck.in_channels_list, neck.out_channels, "f32", "resnet50 op by op")
    assert np.array_equal(bits(got["pool"]), bits(got["3"][:, :, ::2, ::2]))
