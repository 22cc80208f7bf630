"""Stage feature maps on the GPU: rn_nhwc_to_nchw_dt and rn_model_forward_maps(_u8).

The op is checked bit for bit against numpy.transpose on poisoned views between guard bands (tests/views.py); the
model's maps against the float64 forward of tests/test_stage_maps_host.py (fp32) and against the CPU emulation of
the driver's bf16 roundings (bf16); everything that only reschedules the same arithmetic must not change a bit.
Map buffers are handed to the C entry point as 0xA5-filled views: a stage output sits behind a ReLU, so no
written element can equal the (negative) fill.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_c_amd as R
import views as V
from oracle import netref as N
from resnet_c_amd import _lib as L
from resnet_c_amd import ops, preprocess
from resnet_c_amd import weights as W
from test_dilation_gpu import TOL, _rb, bits, state_of, structured
from test_stage_maps_host import stage_maps_f64

pytestmark = pytest.mark.gpu

F32, BF16 = L.RN_DTYPE_F32, L.RN_DTYPE_BF16
STAGES = ("layer1", "layer2", "layer3", "layer4")
MB = 3


# =====================================================================================================================
# 1. the op, exact
# =====================================================================================================================
# (B, C, H, W): 7 x 7, 3 x 3, 1 x 1 and 2 x 2 maps (one span per block), 9 x 12 (two pixel chunks, the second ragged),
# 56 x 56 (many chunks), 70000 images (the grid slabs), and two shapes of the element-wise form (C % 4 != 0; for
# bf16 also C % 8 != 0)
OP_SHAPES = [(2, 64, 7, 7), (3, 256, 3, 3), (1, 64, 1, 1), (2, 128, 9, 12), (1, 2048, 2, 2), (2, 64, 56, 56),
             (70000, 8, 1, 1), (2, 3, 5, 7), (1, 20, 4, 4)]


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_is_numpys_transpose(shape, dt):
    B, C, H, Wd = shape
    g = np.random.default_rng(sum(shape) + dt)
    x = g.standard_normal((B, H, Wd, C), dtype=np.float32)
    if dt == BF16:
        src = ops.to_bf16_bits(x).reshape(x.shape)
        want = (src.astype(np.uint32) << np.uint32(16)).transpose(0, 3, 1, 2)      # the source bits, shifted
    else:
        src = x
        want = x.view(np.uint32).transpose(0, 3, 1, 2)
    want = np.ascontiguousarray(want)
    V.assert_no_poison(want.view(np.float32), False, f"{shape}")
    vi = V.place(src)
    for off in (0, 4, 12):
        what = f"rn_nhwc_to_nchw_dt dt={dt} {shape} dst +{off}"
        vo = V.place_out(want.nbytes, off)
        V.must("rn_nhwc_to_nchw_dt", dt, vi.ptr, vo.ptr, B, C, H, Wd)
        got = V.fetch(vo, np.uint32, what, written=True).reshape(want.shape)       # guards intact, every element written
        assert np.array_equal(got, want), what
    V.check_guards(f"rn_nhwc_to_nchw_dt dt={dt} {shape} src", vi)


def test_op_python_wrapper_and_refusals():
    g = np.random.default_rng(5)
    x = g.standard_normal((2, 5, 6, 16), dtype=np.float32)
    assert np.array_equal(ops.nhwc_to_nchw_dt(x), x.transpose(0, 3, 1, 2))
    assert np.array_equal(ops.nhwc_to_nchw_dt(x, bf16=True), ops.bf16_round(x).transpose(0, 3, 1, 2))
    vi, vo = V.place(x), V.place_out(x.nbytes)
    for args, word in (((7, vi.ptr, vo.ptr, 2, 16, 5, 6), "dtype"), ((F32, vi.ptr, vo.ptr + 2, 2, 16, 5, 6), "4-byte"),
                       ((BF16, vi.ptr + 1, vo.ptr, 2, 16, 5, 6), "element"), ((F32, None, vo.ptr, 2, 16, 5, 6), "null")):
        st, msg = V.call("rn_nhwc_to_nchw_dt", *args)
        assert st == L.RN_ERR_INVALID and word in msg, (args, st, msg)
    V.must("rn_nhwc_to_nchw_dt", F32, vi.ptr, vo.ptr, 0, 16, 5, 6)                 # an empty batch launches nothing
    V.assert_untouched(vo, "refused or empty")


# =====================================================================================================================
# the model
# =====================================================================================================================
@pytest.fixture(scope="module")
def models():
    made = {}

    def get(arch, dtype="f32"):
        if (arch, dtype) not in made:
            made[(arch, dtype)] = R.NativeModel(arch, state=state_of(arch), dtype=dtype)
        m = made[(arch, dtype)]
        m.set_streams(0), m.set_front_parts(1), m.set_chain(True), m.set_pair_fusion(True)
        return m
    yield get
    for m in made.values():
        m.close()


def setup(m, size, flags):
    m.set_input_size(*size)
    if m.arch not in ("resnet18", "resnet34"):
        m.set_dilation(*flags)


@functools.lru_cache(maxsize=None)
def images(size, n=MB):
    x = W.generate_input(n, seed=300 + size[0] + size[1], hw=size)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ref_maps(arch, size, flags):
    """computed once per case, shared, read-only"""
    maps = stage_maps_f64(arch, state_of(arch), images(size), flags)
    for a in maps:
        a.setflags(write=False)
    return dict(zip(STAGES, maps))


class MapsCall:
    """ONE rn_model_forward_maps(_u8) with every wanted map in a 0xA5-filled view between guard bands"""

    def __init__(self, m, x, stages=STAGES, fused=True, head=False, offset=0):
        x = np.ascontiguousarray(x)
        self.u8 = x.dtype == np.uint8
        self.m, self.B, self.stages = m, x.shape[0], tuple(stages)
        self.shapes = {s: (self.B,) + chw for s, chw in m.stage_shapes.items()}
        self.xin = ops._up_raw(x)
        self.views = {s: V.place_out(int(np.prod(self.shapes[s])) * 4, offset) for s in self.stages}
        self.maps = L.ModelMaps()
        for s in self.stages:
            self.maps.layer[STAGES.index(s)] = self.views[s].ptr
        self.head = V.place_out(self.B * m.classes * 4) if head else None
        self.outs = L.ModelOutputs(self.head.ptr if head else None, None, None, None, None, 0)
        self.mode = L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS

    def status(self, outs=True, maps=True, mode=None):
        fn = L.lib().rn_model_forward_maps_u8 if self.u8 else L.lib().rn_model_forward_maps
        st = fn(self.m.handle, self.xin.ptr, self.B, ctypes.byref(self.outs) if outs else None,
                ctypes.byref(self.maps) if maps else None, self.mode if mode is None else mode)
        msg = (L.lib().rn_last_error(self.m.ctx.handle) or b"").decode() if st != L.RN_OK else ""
        self.m.ctx.sync()
        return st, msg

    def run(self):
        st, msg = self.status()
        assert st == L.RN_OK, (st, msg)
        return self.fetch()

    def fetch(self):
        """guards intact, every element written"""
        return {s: V.fetch(self.views[s], np.float32, f"map of {s}", written=True).reshape(self.shapes[s])
                for s in self.stages}

    def logits(self):
        return V.fetch(self.head, np.float32, "logits", written=True).reshape(self.B, -1)

    def repoison(self):
        for v in self.views.values():
            L.check(L.lib().rn_memcpy_h2d(self.m.ctx.handle, v.buf.ptr, v.image.ctypes.data, v.image.size), "h2d")

    def assert_untouched(self, what):
        for s, v in self.views.items():
            V.assert_untouched(v, f"{what}: map of {s}")


def same_bits(a, b, what):
    assert a.keys() == b.keys(), what
    for s in a:
        assert np.array_equal(bits(a[s]), bits(b[s])), f"{what}: {s} differs"


# ---- 2. fp32 maps against float64 --------------------------------------------------------------------------------
FP32_CASES = [("resnet50", (64, 64), (0, 0, 0)), ("resnet50", (33, 47), (0, 0, 0)), ("resnet50", (64, 96), (0, 1, 1)),
              ("resnext50_32x4d", (64, 64), (0, 0, 0)), ("resnet18", (64, 64), (0, 0, 0))]


@pytest.mark.parametrize("arch,size,flags", FP32_CASES,
                         ids=[f"{a}-{s[0]}x{s[1]}-{''.join(map(str, f))}" for a, s, f in FP32_CASES])
def test_fp32_maps_vs_fp64(arch, size, flags, models):
    """max|gpu - ref| <= 1e-4 * max|ref| + 1e-6 per stage (the project's TOL form), in the three modes of
    three_modes; a torch fp32 CPU forward of these nets sits at 3.5e-7 .. 6.4e-7 of max|ref|, a misplaced
    element is O(1)"""
    m, x, want = models(arch), images(size), ref_maps(arch, size, flags)
    setup(m, size, flags)
    assert [m.stage_shapes[s] for s in STAGES] == [want[s].shape[1:] for s in STAGES]
    got = {"ops": MapsCall(m, x, fused=False).run(), "fused": MapsCall(m, x).run()}
    m.set_pair_fusion(False)
    try:
        got["fused, pair fusion off"] = MapsCall(m, x).run()
    finally:
        m.set_pair_fusion(True)
    for what, maps in got.items():
        for s in STAGES:
            top = float(np.abs(want[s]).max())
            err = float(np.abs(maps[s] - want[s]).max())
            print(f"\n  stage maps: {arch} {flags} {size} {what} {s}: max|gpu - fp64| = {err:.3e} = {err / top:.2e} of max|ref|")
            assert err <= TOL * top + 1e-6, (what, s, err, top)


# ---- 3. one forward, same head -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_forward_same_head(dtype, models):
    size, flags = (64, 64), (0, 1, 1)
    m, x = models("resnet50", dtype), images(size)
    setup(m, size, flags)
    for fused in (True, False) if dtype == "f32" else (True,):
        want = m.forward_outputs(x, logits=True, features=True, probs=True, topk=5, fused=fused)
        got = m.forward_maps(x, ("layer4", "layer2"), logits=True, features=True, probs=True, topk=5, fused=fused)
        assert list(got) == ["layer4", "layer2", "logits", "features", "probs", "topk_prob", "topk_idx"]
        for k in want:
            assert np.array_equal(bits(got[k]) if got[k].dtype == np.float32 else got[k],
                                  bits(want[k]) if want[k].dtype == np.float32 else want[k]), (k, fused)
        assert got["layer4"].shape == (MB,) + m.stage_shapes["layer4"] == (MB, 2048, 8, 8)
        mean = got["layer4"].astype(np.float64).mean(axis=(2, 3))
        # fp32: the whole-network bound.  bf16: `features` is the fp32 sum rounded to bf16, half an ulp = 2^-9 of
        # the value; 2^-8 of the largest leaves the fp32 summation its room
        bound = (TOL if dtype == "f32" else 2.0 ** -8) * float(np.abs(mean).max()) + 1e-6
        assert np.abs(mean - got["features"]).max() <= bound
        # nothing asked of the head: the logits go to the model's own buffer, the maps are the same
        alone = m.forward_maps(x, ("layer4", "layer2"), fused=fused)
        assert list(alone) == ["layer4", "layer2"]
        same_bits(alone, {k: got[k] for k in alone}, "maps without head outputs")
    for bad in (("layer5",), ("layer1", "layer1"), ("fc",)):
        with pytest.raises(ValueError):
            m.forward_maps(x, bad)


# ---- 4. rescheduling changes no bit ------------------------------------------------------------------------------
RB = 128


@pytest.fixture(scope="module", params=["f32", "bf16"])
def resched(request):
    """resnet50 (0,1,1) at 64 x 64, B = 128 on one stream: the bits everything else must reproduce"""
    size, flags = (64, 64), (0, 1, 1)
    m = R.NativeModel("resnet50", state=state_of("resnet50"), dtype=request.param, input_size=size,
                      replace_stride_with_dilation=flags)
    x = W.generate_input(RB, seed=42, hw=size)
    m.set_streams(1)
    base = MapsCall(m, x).run()
    yield m, x, base
    m.close()


def test_streams_front_parts_and_chain(resched):
    m, x, base = resched
    try:
        m.set_streams(2)
        assert m.parts(RB) == 2
        same_bits(MapsCall(m, x).run(), base, "two streams")
        m.set_front_parts(4)
        same_bits(MapsCall(m, x).run(), base, "two streams, front in four slices")
        m.set_streams(1)
        same_bits(MapsCall(m, x).run(), base, "one stream, front in four slices")
        m.set_front_parts(1)
        m.set_chain(False)
        same_bits(MapsCall(m, x).run(), base, "no chained launches")
    finally:
        m.set_streams(1), m.set_front_parts(1), m.set_chain(True)


def test_subsets_and_batch_position(resched):
    m, x, base = resched
    m.set_streams(2)
    try:
        same_bits(MapsCall(m, x, ("layer2",)).run(), {"layer2": base["layer2"]}, "layer2 alone")
        same_bits(MapsCall(m, x, ("layer4", "layer1")).run(), {s: base[s] for s in ("layer4", "layer1")}, "layer4, layer1")
        moved = MapsCall(m, x[[100, 3, 77]]).run()
        same_bits(moved, {s: base[s][[100, 3, 77]] for s in STAGES}, "an image at another batch position")
        # an offset, 4-byte-aligned destination: the same bits (test 1 holds the op to it; here through the model)
        same_bits(MapsCall(m, x[:5], offset=4).run(), {s: base[s][:5] for s in STAGES}, "maps 4 bytes off")
    finally:
        m.set_streams(1)


def test_byte_route(resched):
    m, _x, _base = resched
    px = np.random.default_rng(9).integers(0, 256, (RB, 64, 64, 3), dtype=np.uint8)
    m.set_streams(2)
    try:
        a = MapsCall(m, px).run()
        b = MapsCall(m, preprocess.normalize_u8(px)).run()
        same_bits(a, b, "forward_maps_u8 against forward_maps(normalize_u8)")
        c = m.forward_maps_u8(px[:4], ("layer3",))
        assert np.array_equal(bits(c["layer3"]), bits(a["layer3"][:4]))
    finally:
        m.set_streams(1)


def test_two_sub_batches(resched):
    m, _x, _base = resched
    m.set_input_size(32, 32)
    try:
        cap = m.max_sub_batch()
        x = W.generate_input(cap + 1, seed=43, hw=(32, 32))
        whole = MapsCall(m, x).run()
        first, last = MapsCall(m, x[:cap]).run(), MapsCall(m, x[cap:]).run()
        same_bits({s: whole[s][:cap] for s in STAGES}, first, "first sub-batch")
        same_bits({s: whole[s][cap:] for s in STAGES}, last, "second sub-batch")
    finally:
        m.set_input_size(64, 64)


def test_request_does_not_outlive_its_call(resched):
    m, x, base = resched
    m.set_streams(2)
    try:
        before = m.forward(x, fused=True)
        call = MapsCall(m, x, head=True)
        same_bits(call.run(), base, "maps")
        assert np.array_equal(bits(call.logits()), bits(before))
        call.repoison()
        launches = L.lib().rn_ctx_launch_count(m.ctx.handle)
        m.forward(x[:8], fused=True)
        per_forward = L.lib().rn_ctx_launch_count(m.ctx.handle) - launches
        assert np.array_equal(bits(m.forward(x, fused=True)), bits(before))
        call.assert_untouched("after a plain forward")
        # a maps forward of 8 images (one part, the model's own stream) adds exactly one launch per wanted stage
        launches = L.lib().rn_ctx_launch_count(m.ctx.handle)
        MapsCall(m, x[:8], ("layer1", "layer3")).run()
        assert L.lib().rn_ctx_launch_count(m.ctx.handle) - launches == per_forward + 2
        launches = L.lib().rn_ctx_launch_count(m.ctx.handle)
        m.forward(x[:8], fused=True)
        assert L.lib().rn_ctx_launch_count(m.ctx.handle) - launches == per_forward
        xd = R.FloatTensor.from_numpy(x[:8], R.Device.GPU)
        out = R.FloatTensor((8, 1000), R.Device.GPU)
        m.tune(xd.data(), 8, out.data(), True)
        m.ctx.sync()
        assert np.array_equal(bits(out.numpy()), bits(before[:8]))
        call.assert_untouched("after a tuning pass")
        # an error on the way leaves no request behind either
        st, _ = call.status(mode=7)
        assert st == L.RN_ERR_INVALID
        m.forward(x, fused=True)
        call.assert_untouched("after a refused maps call and a plain forward")
    finally:
        m.set_streams(1)


# ---- 5. bf16 maps ------------------------------------------------------------------------------------------------
@torch.no_grad()
def stage_maps_bf16_emulated(arch, state, x, flags):
    """the loop of features_bf16_emulated (tests/test_dilation_gpu.py) with h kept at the end of every stage"""
    t = lambda k: torch.from_numpy(np.asarray(state[k], dtype=np.float64))
    q = lambda k: _rb(t(k))
    groups = W.family_of(arch)[1]
    h = _rb(torch.from_numpy(np.asarray(x, dtype=np.float64)))
    sc, sh = N._fold(state, "bn1")
    h = F.relu(N._affine(F.conv2d(h, q("conv1.weight"), stride=2, padding=3), sc, sh))
    h = _rb(F.max_pool2d(h, 3, 2, 1))
    maps = {}
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
        maps[pre.split(".")[0]] = h.numpy()
    return maps


@pytest.mark.parametrize("flags", [(0, 0, 0), (0, 1, 1)], ids=lambda f: "".join(map(str, f)))
def test_bf16_maps_within_the_emulations_distance(flags, finch, models):
    """resnet50 at 64 x 64 in bf16 on structured images: per stage the RMS and the max distance from the float64 maps
    are at most 2.3 times (the project's multiple, test_input_size_gpu.py) those of the CPU emulation of the driver's
    roundings, and those bounds are below a fifth of the maps' std and max.  Every value is a widened bf16.
    The numbers are in profiles/stage_maps/README.md."""
    arch, size = "resnet50", (64, 64)
    state, x = state_of(arch), structured(finch, size)
    want = dict(zip(STAGES, stage_maps_f64(arch, state, x, flags)))
    emu = stage_maps_bf16_emulated(arch, state, x, flags)
    m = models(arch, "bf16")
    setup(m, size, flags)
    got = MapsCall(m, x).run()
    for s in STAGES:
        assert not (bits(got[s]) & np.uint32(0xFFFF)).any(), s
        d_emu, d_gpu = emu[s] - want[s], got[s].astype(np.float64) - want[s]
        rms_bound, max_bound = 2.3 * float(np.sqrt((d_emu ** 2).mean())), 2.3 * float(np.abs(d_emu).max())
        rms, mx = float(np.sqrt((d_gpu ** 2).mean())), float(np.abs(d_gpu).max())
        std, top = float(want[s].std()), float(np.abs(want[s]).max())
        print(f"\n  stage maps: bf16 {flags} {s}: rms gpu {rms:.4f} emulation {rms_bound / 2.3:.4f} bound {rms_bound:.4f} "
              f"std {std:.3f}; max gpu {mx:.4f} emulation {max_bound / 2.3:.4f} bound {max_bound:.4f} max|ref| {top:.2f}")
        assert std > 5 * rms_bound and top > 5 * max_bound, (s, std, rms_bound, top, max_bound)   # the check means something
        assert rms <= rms_bound, (s, rms, rms_bound)
        assert mx <= max_bound, (s, mx, max_bound)


# ---- 6. refusals launch nothing ------------------------------------------------------------------------------------
def test_refusals_launch_nothing(models):
    size = (64, 64)
    m, x = models("resnet50"), images(size)
    setup(m, size, (0, 0, 0))
    lib = L.lib()

    def refused(call, want, word="", **kw):
        before = lib.rn_ctx_launch_count(m.ctx.handle)
        st, msg = call.status(**kw)
        assert st == want and word in msg, (kw, st, msg)
        assert lib.rn_ctx_launch_count(m.ctx.handle) == before
        call.assert_untouched(f"refused {kw}")
        if call.head:
            V.assert_untouched(call.head, f"refused {kw}: logits")

    call = MapsCall(m, x, head=True)
    refused(call, L.RN_ERR_INVALID, "maps is NULL", maps=False)
    refused(call, L.RN_ERR_INVALID, mode=2)
    refused(call, L.RN_ERR_INVALID, mode=-1)
    nothing = MapsCall(m, x, stages=())
    refused(nothing, L.RN_ERR_INVALID, "nothing to write")                  # all four NULL, an empty rn_model_outputs
    refused(nothing, L.RN_ERR_INVALID, "nothing to write", outs=False)      # all four NULL, no rn_model_outputs
    odd = MapsCall(m, x, head=True)
    odd.maps.layer[2] = odd.views["layer3"].ptr + 2
    refused(odd, L.RN_ERR_INVALID, "layer3")
    assert "4-byte" in odd.status()[1]
    topk = MapsCall(m, x)
    topk.outs.k = 5                                                         # top-k without its two buffers
    refused(topk, L.RN_ERR_INVALID)
    # a model that is not finalized
    h = ctypes.c_void_p()
    L.check(lib.rn_model_create(m.ctx.handle, ctypes.byref(h), 50), "rn_model_create")
    try:
        before = lib.rn_ctx_launch_count(m.ctx.handle)
        assert lib.rn_model_forward_maps(h, call.xin.ptr, MB, None, ctypes.byref(call.maps), L.RN_FWD_FUSED) == L.RN_ERR_INVALID
        assert lib.rn_ctx_launch_count(m.ctx.handle) == before
        call.assert_untouched("model not finalized")
    finally:
        lib.rn_model_destroy(h)
    # bf16 storage exists in the fused mode only
    mb = models("resnet50", "bf16")
    setup(mb, size, (0, 0, 0))
    cb = MapsCall(mb, x, fused=False)
    st, _ = cb.status()
    assert st == L.RN_ERR_UNSUPPORTED
    cb.assert_untouched("bf16 with the reference ops")
    # and the refused model still runs
    assert call.status()[0] == L.RN_OK
    call.fetch()


# ---- 7. rn_infer --maps ----------------------------------------------------------------------------------------------
def test_rn_infer_maps(tmp_path, models):
    size, flags = (64, 64), (0, 1, 1)
    wdir = tmp_path / "weights_bin"
    os.mkdir(wdir)
    W.save_weights_bin(state_of("resnet50"), str(wdir))
    x = images(size)[:2]
    inp = tmp_path / "in_64x64.bin"
    np.ascontiguousarray(x).tofile(inp)
    m = models("resnet50")
    setup(m, size, flags)
    want = m.forward_maps(x, logits=True)
    exe = os.path.join(os.path.dirname(L.LIB_PATH), "rn_infer")
    base = [exe, "--weights", str(wdir), "--batch", "2", "--size", "64,64", "--input", str(inp), "--arch", "50",
            "--dilate", "0,1,1"]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    r = subprocess.run(base + ["--maps", str(tmp_path / "m")], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    assert r.stdout == plain.stdout                                        # the lines printed are unchanged
    assert [int(l.split()[-1]) for l in r.stdout.splitlines() if l.startswith("max index is")] == want["logits"].argmax(1).tolist()
    for s in STAGES:
        got = np.fromfile(tmp_path / f"m.{s}.bin", dtype=np.float32)
        assert got.size == want[s].size == 2 * int(np.prod(m.stage_shapes[s])), s
        assert np.array_equal(bits(got), bits(want[s]).reshape(-1)), s


# ---- 8. profile ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_profile_records(dtype, models):
    size, flags = (64, 96), (0, 1, 1)
    m, x = models("resnet50", dtype), images(size)
    setup(m, size, flags)
    m.forward_outputs(x, logits=True)
    m.set_profiling(True)
    try:
        m.forward_outputs(x, logits=True)
        plain = m.profile()
        MapsCall(m, x, ("layer2", "layer4")).run()
        recs = m.profile()
    finally:
        m.set_profiling(False)
    mine = [r for r in recs if r["op"] == "stage_map"]
    assert [r["layer"] for r in mine] == ["layer2", "layer4"]
    es = 4 if dtype == "f32" else 2
    for r in mine:
        assert r["bytes"] == MB * int(np.prod(m.stage_shapes[r["layer"]])) * (es + 4) and r["flops"] == 0 and r["ms"] > 0
    # every other record is the plain forward's, in its order
    key = lambda r: (r["op"], r["layer"], r["flops"], r["bytes"])
    assert [key(r) for r in recs if r["op"] != "stage_map"] == [key(r) for r in plain]
    # the export sits right behind the last block of its stage
    names = [r["layer"] for r in recs]
    at = names.index("layer2")
    assert names[at - 1].startswith("layer2.3") and names[at + 1].startswith("layer3.0"), names[at - 1:at + 2]
