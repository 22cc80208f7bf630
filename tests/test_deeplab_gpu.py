"""DeepLabV3 head on the GPU: rn_concat_channels_forward_dt, the DeepLab kind of rn_seg_head_* and
rn_model_forward_segment(_u8) with it.

The concat is a copy and is held bit for bit to ops.concat_channels_ref on views between guard bands (tests/views.py),
NaN payloads included.  The head is held to the float64 torch reference segmentation.deeplab_head_ref (itself held to
torchvision's module by tests/test_deeplab_host.py, which also owns the cases and seeds) with the bounds the single
convolutions have in tests/test_dilation_gpu.py; the model hook to the same reference on the layer4 map the same model
hands out.  Everything that only reschedules the same arithmetic -- the centre-tap plan, streams, sub-batches, the
other head on the same model -- must not change a bit.

Launch counts.  A DeepLab forward is n + 8 entry points.  rn_ctx_launch_count counts kernels, and a contraction with
fp32 output and 32 or more K tiles (K >= 1024 in fp32) folds its sum in chunks and, on a grid smaller than one round
of the chip, adds the chunks in a second kernel (include/rn_hip.h; test_segmentation_gpu.py meets the same: "a
contraction may count more than one launch").  expected_launches() counts those contractions from the shapes, so the
assertion stays an equality: n + 8 for every bf16 head, n + 8 plus the chunked 3x3 branches for the fp32 ones.
"""
import ctypes
import functools

import numpy as np
import pytest

import resnet_c_amd as R
import views as V
from resnet_c_amd import _lib as L
from resnet_c_amd import ops, preprocess
from resnet_c_amd import segmentation as S
from resnet_c_amd import weights as W
from test_deeplab_host import CASES, CONCAT_CASES, HEAD_SEED, concat_sources, head_map, head_ref, head_state
from test_dilation_gpu import bits, state_of, tol_bf16, tol_f32

pytestmark = pytest.mark.gpu

DT = {"f32": L.RN_DTYPE_F32, "bf16": L.RN_DTYPE_BF16}


def launches(ctx=None):
    return int(L.lib().rn_ctx_launch_count((ctx or R.get_ctx()).handle))


# =====================================================================================================================
# 1. the concat, bit for bit
# =====================================================================================================================
def concat_call(dtype, srcs, per, dst_ptr, B, pixels):
    """the C arguments of one rn_concat_channels_forward_dt on device pointers"""
    ptrs = (ctypes.c_void_p * len(srcs))(*[p for p, _ in srcs])
    chans = (ctypes.c_uint64 * len(srcs))(*[c for _, c in srcs])
    return (DT[dtype], len(srcs), ptrs, chans, per[0] if per else None, per[1] if per else 0, dst_ptr, B, pixels)


def run_concat(case, dtype, special):
    bf16 = dtype == "bf16"
    srcs, per = concat_sources(case, bf16, special)
    want = ops.concat_channels_ref(srcs, per)
    B, pixels, total = want.shape
    what = f"rn_concat_channels_forward_dt {dtype} {case} special={special}"
    vs = [V.place(s) for s in srcs]
    vp = V.place(per) if per is not None else None
    vo = V.place_out(want.nbytes)
    before = launches()
    V.must("rn_concat_channels_forward_dt",
           *concat_call(dtype, [(v.ptr, s.shape[2]) for v, s in zip(vs, srcs)], (vp.ptr, per.shape[1]) if vp else None,
                        vo.ptr, B, pixels))
    assert launches() - before == 1, what
    V.check_guards(what, vp, *vs)
    got = V.fetch(vo, want.dtype, what, written=True, row=total).reshape(want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, np.unravel_index(bad[0], want.shape))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(CONCAT_CASES))
def test_concat_is_numpy_concatenate_bit_for_bit(case, dtype):
    run_concat(case, dtype, special=False)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_concat_copies_nan_payloads_and_signed_zeros(dtype):
    for case in ("aspp", "broadcast"):
        run_concat(case, dtype, special=True)


def test_concat_python_wrappers():
    for bf16, fn in ((False, ops.concat_channels), (True, ops.concat_channels_bf16)):
        srcs, per = concat_sources("aspp", bf16, special=True)
        got = fn([s.view(np.float32) for s in srcs] if not bf16 else srcs, per.view(np.float32) if not bf16 else per)
        want = ops.concat_channels_ref(srcs, per)
        assert np.array_equal(got.view(want.dtype), want)
        srcs, _ = concat_sources("eight", bf16)
        got = fn([s.view(np.float32) for s in srcs] if not bf16 else srcs)
        assert np.array_equal(got.view(want.dtype), ops.concat_channels_ref(srcs))


# =====================================================================================================================
# 2. refusals
# =====================================================================================================================
def test_concat_refusals_launch_nothing():
    srcs, per = concat_sources("aspp", False)
    B, pixels = srcs[0].shape[:2]
    vs, vp = [V.place(s) for s in srcs], V.place(per)
    total = sum(s.shape[2] for s in srcs) + per.shape[1]
    vo = V.place_out(B * pixels * total * 4 + 16)
    good = [(v.ptr, s.shape[2]) for v, s in zip(vs, srcs)]
    ok = concat_call("f32", good, (vp.ptr, per.shape[1]), vo.ptr, B, pixels)

    def args(**kw):
        names = ("dtype", "n_src", "srcs", "channels", "per_image", "per_image_channels", "dst", "B", "pixels")
        a = dict(zip(names, ok))
        a.update(kw)
        return tuple(a[n] for n in names)

    def with_src0(ptr, ch):
        return concat_call("f32", [(ptr, ch)] + good[1:], (vp.ptr, per.shape[1]), vo.ptr, B, pixels)

    nine = concat_call("f32", [good[0]] * 9, None, vo.ptr, B, pixels)
    cases = [(args(srcs=None), "NULL"), (args(dst=None), "NULL"), (args(channels=None), "NULL"),
             (with_src0(None, 64), "NULL"), (args(per_image=None), "per_image"), (args(per_image_channels=0), "per_image"),
             (args(n_src=0), "n_src"), (nine, "n_src"), (with_src0(good[0][0], 0), "channel count"),
             (with_src0(good[0][0], 6), "16 bytes"), (args(per_image_channels=6), "16 bytes"),
             (with_src0(good[0][0] + 4, 64), "16-byte"), (args(dst=vo.ptr + 4), "16-byte"),
             (args(per_image=vp.ptr + 4), "16-byte"), (args(dst=good[1][0]), "overlaps"), (args(dst=vp.ptr), "overlaps"),
             (args(dtype=7), "dtype")]
    before = launches()
    for a, word in cases:
        st, msg = V.call("rn_concat_channels_forward_dt", *a)
        assert st == L.RN_ERR_INVALID and word in msg, (word, st, msg)
    assert L.lib().rn_concat_channels_forward_dt(None, *ok) == L.RN_ERR_INVALID        # no context
    V.must("rn_concat_channels_forward_dt", *args(B=0))                               # an empty batch launches nothing
    V.must("rn_concat_channels_forward_dt", *args(pixels=0))
    assert launches() == before
    V.assert_untouched(vo, "refused or empty concat: dst")
    for v in vs + [vp]:
        V.assert_untouched(v, "refused or empty concat: a source")
    V.must("rn_concat_channels_forward_dt", *ok)                                      # and the call they all almost were
    got = V.fetch(vo, np.uint32, "concat", written=False)[:B * pixels * total]
    assert np.array_equal(got.reshape(B, pixels, total), ops.concat_channels_ref(srcs, per))


# =====================================================================================================================
# 3. the head alone
# =====================================================================================================================
def expected_launches(case, dtype):
    """kernels of one forward (module docstring): n + 8, plus one for every contraction with fp32 output and >= 32 K
    tiles of 128 bytes; the centre-tap plan is taken by bf16 heads only at these widths and changes no count there"""
    cin, a, _classes, _bhw, _size, rates = CASES[case]
    n = len(rates)
    if dtype == "bf16":
        return n + 8                                             # bf16 outputs; the classifier's K = a is 1..4 tiles
    ks = [cin] + [9 * cin] * n + [cin, (n + 2) * a, 9 * a, a]    # K of the n + 4 convolutions and the classifier
    return n + 8 + sum(1 for k in ks if k // 32 >= 32)


def make_head(case, dtype, ctx=None):
    cin, a, classes, _bhw, _size, rates = CASES[case]
    return S.DeepLabHead(cin, classes, head_state(case), aspp_channels=a, rates=rates, dtype=dtype, ctx=ctx)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", ["H1", "H2"])
def test_head_alone(case, dtype):
    """scores within tol_f32(ref, 9 * in_channels) (fp32) or tol_bf16(ref) (bf16: the reference rounds the map, the
    weights and every stored tensor where the device does) of the float64 head; labels = numpy.argmax of the scores of
    the same call, the same from a labels-only call; a repeated call gives the same bits; the launch count"""
    cin, _a, _classes, bhw, size, _rates = CASES[case]
    x, ref = head_map(case), head_ref(case, dtype == "bf16")
    head = make_head(case, dtype)
    try:
        before = launches()
        scores, labels = head.forward(x, size, scores=True, labels=True)
        assert launches() - before == expected_launches(case, dtype)
        assert scores.shape == ref.shape and labels.shape == (bhw[0],) + size
        tol = tol_f32(ref, 9 * cin) if dtype == "f32" else tol_bf16(ref)
        err = float(np.abs(scores - ref).max())
        print(f"\n  DeepLabHead {case} {dtype}: max|gpu - fp64| = {err:.3e}, bound {tol:.3e}, max|ref| = {np.abs(ref).max():.3f}")
        assert err <= tol
        assert np.array_equal(labels, scores.argmax(axis=1))
        assert len(np.unique(labels)) >= 3
        none, only = head.forward(x, size, scores=False, labels=True)
        assert none is None and np.array_equal(only, labels)
        again, _ = head.forward(x, size, scores=True, labels=False)
        assert np.array_equal(bits(again), bits(scores))
    finally:
        head.close()


# =====================================================================================================================
# 4. the centre tap changes no bit
# =====================================================================================================================
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", ["H1", "H2"])
def test_center_tap_changes_no_bit(case, dtype):
    """H2: all three branches centre-only; H1: its rate-6 branch on the 6 x 5 map.  (An fp32 head of these widths keeps
    the 3x3 route either way -- include/rn_hip.h says why -- and must then give the same bits all the more.)"""
    _cin, _a, _classes, _bhw, size, _rates = CASES[case]
    x = head_map(case)
    head = make_head(case, dtype)
    try:
        on, on_labels = head.forward(x, size, scores=True, labels=True)
        head.center_tap(False)
        before = launches()
        off, off_labels = head.forward(x, size, scores=True, labels=True)
        assert launches() - before == expected_launches(case, dtype)
        head.center_tap(True)
        again, _ = head.forward(x, size, scores=True, labels=False)
    finally:
        head.close()
    assert np.array_equal(bits(on), bits(off)) and np.array_equal(on_labels, off_labels)
    assert np.array_equal(bits(again), bits(on))


def test_center_tap_fp32_head_that_takes_the_plan():
    """in_channels = 64 is the fp32 width at which neither route chunks its K sum: the plan runs, the bits stay"""
    cin, a, classes, rates, size = 64, 64, 5, (4, 9), (12, 12)
    st = S.generate_deeplab_head_state(cin, classes, a, rates, seed=HEAD_SEED)
    x = np.random.default_rng(64).standard_normal((2, 4, 3, cin), dtype=np.float32)
    head = S.DeepLabHead(cin, classes, st, aspp_channels=a, rates=rates)
    try:
        on, _ = head.forward(x, size)
        head.center_tap(False)
        off, _ = head.forward(x, size)
    finally:
        head.close()
    ref = S.deeplab_head_ref(x.transpose(0, 3, 1, 2).astype(np.float64), st, size, rates)
    assert float(np.abs(on - ref).max()) <= tol_f32(ref, 9 * cin)
    assert np.array_equal(bits(on), bits(off))


@pytest.mark.parametrize("dtype,cin", [("bf16", 128), ("f32", 64)])
def test_center_tap_at_op_level(dtype, cin):
    """dilation 6 on a 6 x 5 map, in -> 64 channels: the dilated 3x3 equals the 1x1 on the centre panel, as bits, at
    the widths where the head takes the plan: 128 channels in bf16 (every width does), 64 in fp32.  fp32 at 128
    channels is where the plan is NOT taken: measured there, 3170 of 3840 outputs differ in the last bits (at most
    4.2e-7; 3497 at 512 channels, 3647 at 2048), because the fp32 3x3 folds its K sum at tile 18 of 36, in the middle
    of the centre tap's tiles 16..19, and the 1x1 does not fold (profiles/deeplab/center_tap_bits.txt).  The head is
    restricted instead of this check loosened ("DeepLabV3 head")."""
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, cin, 6, 5), dtype=np.float32)
    w = (rng.standard_normal((64, cin, 3, 3), dtype=np.float32) / np.sqrt(9 * cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, 64).astype(np.float32)
    shift = rng.uniform(-0.1, 0.1, 64).astype(np.float32)
    centre = np.ascontiguousarray(w[:, :, 1:2, 1:2])
    if dtype == "bf16":
        full = ops.conv2d_dilated_nhwc_bf16(x, w, pad=6, dilation=6, scale=scale, shift=shift, relu_=True)
        one = ops.conv2d_nhwc_bf16(x, centre, scale=scale, shift=shift, relu_=True)
    else:
        full = ops.conv2d_dilated_nhwc(x, w, pad=6, dilation=6, scale=scale, shift=shift, relu_=True)
        one = ops.conv2d_nhwc_fused(x, centre, scale=scale, shift=shift, relu_=True)
    assert full.shape == one.shape == (2, 64, 6, 5) and (full > 0).any()
    assert np.array_equal(bits(full), bits(one))


# =====================================================================================================================
# 5. head refusals
# =====================================================================================================================
def test_head_refusals():
    ctx, lib = R.get_ctx(), L.lib()
    h = ctypes.c_void_p()

    def create(cin, a, classes, rates):
        r = (ctypes.c_uint64 * max(len(rates), 1))(*rates)
        return lib.rn_seg_head_create_deeplab(ctx.handle, ctypes.byref(h), cin, a, classes, len(rates), r)

    for bad in ((100, 64, 21, (2,)), (128, 0, 21, (2,)), (128, 96, 21, (2,)), (128, 2048, 21, (2,)), (128, 64, 0, (2,)),
                (128, 64, 257, (2,)), (128, 64, 21, ()), (128, 64, 21, (1, 2, 3, 4, 5)), (128, 64, 21, (2, 0)),
                (128, 64, 21, (L.RN_CONV_MAX_DILATION + 1,))):
        assert create(*bad) == L.RN_ERR_INVALID and not h.value, bad
    assert lib.rn_seg_head_create_deeplab(ctx.handle, ctypes.byref(h), 128, 64, 21, 1, None) == L.RN_ERR_INVALID
    fcn = ctypes.c_void_p()
    assert lib.rn_seg_head_create(ctx.handle, ctypes.byref(fcn), 128, 32, 5) == L.RN_OK
    assert create(128, 64, 5, (2, L.RN_CONV_MAX_DILATION)) == L.RN_OK
    try:
        w = np.zeros(64, np.float32)
        assert lib.rn_seg_head_set_tensor(h, b"classifier.0.weight", w.ctypes.data, 64) == L.RN_ERR_INVALID   # an FCN key
        assert b"classifier.0.weight" in lib.rn_last_error(ctx.handle)
        assert lib.rn_seg_head_set_tensor(h, b"classifier.0.convs.4.0.weight", w.ctypes.data, 64) == L.RN_ERR_INVALID
        assert lib.rn_seg_head_set_tensor(fcn, b"classifier.0.project.0.weight", w.ctypes.data, 64) == L.RN_ERR_INVALID
        assert b"classifier.0.project.0.weight" in lib.rn_last_error(ctx.handle)
        assert lib.rn_seg_head_set_tensor(h, b"classifier.4.bias", w.ctypes.data, 7) == L.RN_ERR_INVALID       # 5 classes
        assert b"classifier.4.bias" in lib.rn_last_error(ctx.handle)
        assert lib.rn_seg_head_set_tensor(h, b"classifier.0.convs.3.2.weight", w.ctypes.data, 64) == L.RN_OK    # the pooled branch's bn
        assert lib.rn_seg_head_set_tensor(h, b"classifier.0.convs.3.1.weight", w.ctypes.data, 64) == L.RN_ERR_INVALID   # [64,128,1,1]
        assert lib.rn_seg_head_set_center_tap(fcn, 0) == L.RN_ERR_INVALID
        assert lib.rn_seg_head_set_center_tap(h, 2) == L.RN_ERR_INVALID and lib.rn_seg_head_set_center_tap(h, 0) == L.RN_OK
        assert lib.rn_seg_head_finalize(h) == L.RN_ERR_INVALID                        # tensors missing
        assert b"classifier.0.convs.0.0.weight" in lib.rn_last_error(ctx.handle)
        v = V.place(np.zeros((1, 2, 2, 128), np.float32))
        vo = V.place_out(4 * 4)
        before = launches()
        assert lib.rn_seg_head_forward(h, v.ptr, 1, 2, 2, 4, 4, None, vo.ptr) == L.RN_ERR_INVALID   # not finalized
        assert launches() == before
        V.assert_untouched(vo, "head not finalized")
    finally:
        lib.rn_seg_head_destroy(h)
        lib.rn_seg_head_destroy(fcn)


# =====================================================================================================================
# 6.-9. the model
# =====================================================================================================================
SIZE, FLAGS, MB = (64, 64), (0, 1, 1), 3
_CIN, ASPP, CLASSES, _BHW, _SIZE, RATES = CASES["model"]   # rates 2 and 4 reach inside the 8 x 8 map, rate 12 is centre-only
OPS = ["aspp_conv0", "aspp_conv1", "aspp_conv2", "aspp_conv3", "aspp_pool", "aspp_pool_conv", "aspp_concat",
       "aspp_project", "seg_conv1", "seg_conv2", "seg_upsample"]


@functools.lru_cache(maxsize=None)
def images(n=MB):
    x = W.generate_input(n, seed=300 + SIZE[0] + SIZE[1], hw=SIZE)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def nets():
    made = {}

    def get(dtype="f32"):
        if dtype not in made:
            m = R.NativeModel("resnet50", state=state_of("resnet50"), dtype=dtype, input_size=SIZE,
                              replace_stride_with_dilation=FLAGS)
            made[dtype] = (m, make_head("model", dtype, ctx=m.ctx))
        m, head = made[dtype]
        m.set_streams(0)
        head.center_tap(True)
        return m, head
    yield get
    for m, head in made.values():
        head.close()
        m.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_head_isolated(nets, dtype):
    """the head against deeplab_head_ref on the layer4 map the same model returns for the same images"""
    m, head = nets(dtype)
    x = images()
    assert m.stage_shapes["layer4"] == (2048, 8, 8)
    maps = m.forward_maps(x, ("layer4",))["layer4"]
    ref = S.deeplab_head_ref(maps.astype(np.float64), head_state("model"), SIZE, RATES,
                             round_fn=ops.bf16_round if dtype == "bf16" else None)
    got = m.forward_segment(x, head, labels=True, scores=True)
    assert list(got) == ["labels", "scores"]
    assert got["scores"].shape == ref.shape == (MB, CLASSES) + SIZE and got["labels"].shape == (MB,) + SIZE
    tol = tol_f32(ref, 9 * m.features) if dtype == "f32" else tol_bf16(ref)
    err = float(np.abs(got["scores"] - ref).max())
    print(f"\n  forward_segment DeepLab {dtype}: max|gpu - fp64 head on the gpu's map| = {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    assert np.array_equal(got["labels"], got["scores"].argmax(axis=1))
    assert len(np.unique(got["labels"])) >= 3
    only = m.forward_segment(x, head)
    assert list(only) == ["labels"] and np.array_equal(only["labels"], got["labels"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_rescheduling_changes_no_bit(nets, dtype):
    m, head = nets(dtype)
    x = images()
    base = m.forward_segment(x, head, labels=True, scores=True)
    head.center_tap(False)
    off = m.forward_segment(x, head, labels=True, scores=True)
    head.center_tap(True)
    assert np.array_equal(bits(off["scores"]), bits(base["scores"])) and np.array_equal(off["labels"], base["labels"])
    try:
        m.set_streams(2)
        two = m.forward_segment(x, head, labels=True, scores=True)
        assert np.array_equal(bits(two["scores"]), bits(base["scores"])) and np.array_equal(two["labels"], base["labels"])
    finally:
        m.set_streams(0)
    for i in range(MB):      # one call of three images against three calls of one
        one = m.forward_segment(x[i:i + 1], head, labels=True, scores=True)
        assert np.array_equal(bits(one["scores"][0]), bits(base["scores"][i])), i
        assert np.array_equal(one["labels"][0], base["labels"][i]), i
    px = np.random.default_rng(9).integers(0, 256, (MB,) + SIZE + (3,), dtype=np.uint8)
    a = m.forward_segment_u8(px, head, labels=True, scores=True)
    b = m.forward_segment(preprocess.normalize_u8(px), head, labels=True, scores=True)
    assert np.array_equal(bits(a["scores"]), bits(b["scores"])) and np.array_equal(a["labels"], b["labels"])


def test_model_other_outputs_keep_their_bits(nets):
    m, head = nets()
    x = images()
    want = m.forward_outputs(x, logits=True, features=True)
    got = m.forward_segment(x, head, labels=True, scores=False, logits=True, features=True)
    assert list(got) == ["labels", "logits", "features"]
    for k in ("logits", "features"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    # the request does not outlive its call, and the head adds exactly the launches it issues alone
    before = launches(m.ctx)
    a = m.forward(x)
    plain = launches(m.ctx) - before
    before = launches(m.ctx)
    head.forward(np.zeros((MB, 8, 8, 2048), np.float32), SIZE, scores=False, labels=True)
    alone = launches(m.ctx) - before
    assert alone == expected_launches("model", "f32")
    before = launches(m.ctx)
    m.forward_segment(x, head)
    assert launches(m.ctx) - before == plain + alone
    before = launches(m.ctx)
    assert np.array_equal(bits(m.forward(x)), bits(a))
    assert launches(m.ctx) - before == plain


def test_model_parts_on_two_streams(nets):
    """128 images as two parts of 64 on two streams, each in its own slice of the head's scratch (per pixel and, for
    the pooled vectors, per image): the bits of one stream, and of the three-image call for the images they share"""
    m, head = nets()
    x = W.generate_input(128, seed=300 + SIZE[0] + SIZE[1], hw=SIZE)
    assert np.array_equal(x[:MB], images())
    try:
        m.set_streams(1)
        one = m.forward_segment(x, head, labels=True, scores=True)
        m.set_streams(2)
        assert m.parts(128) == 2
        two = m.forward_segment(x, head, labels=True, scores=True)
    finally:
        m.set_streams(0)
    assert np.array_equal(bits(two["scores"]), bits(one["scores"])) and np.array_equal(two["labels"], one["labels"])
    few = m.forward_segment(images(), head, labels=True, scores=True)
    assert np.array_equal(bits(few["scores"]), bits(one["scores"][:MB])) and np.array_equal(few["labels"], one["labels"][:MB])
    assert np.array_equal(one["labels"], one["scores"].argmax(axis=1))


def test_model_refusals(nets):
    m, head = nets()
    _mb, headb = nets("bf16")
    lib = L.lib()
    x = ops._up_raw(images())
    vl = V.place_out(MB * SIZE[0] * SIZE[1])
    seg = L.SegOutputs(vl.ptr, None)
    narrow = make_head("H2", "f32", ctx=m.ctx)          # in_channels 512
    raw = ctypes.c_void_p()
    rates = (ctypes.c_uint64 * 3)(*RATES)
    assert lib.rn_seg_head_create_deeplab(m.ctx.handle, ctypes.byref(raw), 2048, ASPP, CLASSES, 3, rates) == L.RN_OK

    def call(hd, seg_ptr):
        st = lib.rn_model_forward_segment(m.handle, hd, x.ptr, MB, None, seg_ptr, L.RN_FWD_FUSED)
        return st, (lib.rn_last_error(m.ctx.handle) or b"").decode()

    try:
        before = launches(m.ctx)
        for hd, seg_ptr, word in ((narrow.handle, ctypes.byref(seg), "in_channels"), (headb.handle, ctypes.byref(seg), "dtype"),
                                  (raw, ctypes.byref(seg), "not finalized"), (head.handle, None, "seg is NULL"),
                                  (head.handle, ctypes.byref(L.SegOutputs(None, None)), "names nothing")):
            st, msg = call(hd, seg_ptr)
            assert st == L.RN_ERR_INVALID and word in msg, (word, st, msg)
        assert launches(m.ctx) == before
        m.ctx.sync()
        V.assert_untouched(vl, "refused segment calls")
        st, msg = call(head.handle, ctypes.byref(seg))                    # and the call they all almost were
        assert st == L.RN_OK, msg
        m.ctx.sync()
        want = m.forward_segment(images(), head)["labels"]
        assert np.array_equal(V.fetch(vl, np.uint8, "labels", written=True).reshape(want.shape), want)
    finally:
        lib.rn_seg_head_destroy(raw)
        narrow.close()


def profile_of(m, head, x):
    m.forward_segment(x, head)
    m.set_profiling(True)
    try:
        m.forward_outputs(x, logits=True)
        plain = m.profile()
        m.forward_segment(x, head)
        recs = m.profile()
    finally:
        m.set_profiling(False)
    return plain, recs


def test_profile_records(nets):
    """the eleven records (nine names, aspp_conv1..3 being one) in order; every branch reports the FLOPs of the route
    that runs: in the bf16 model aspp_conv3 (rate 12 on 8 x 8) is the centre tap, a ninth of aspp_conv1, and the full
    3x3 again with the plan switched off; the fp32 head at 2048 channels keeps the 3x3 (include/rn_hip.h) and says so"""
    x = images()
    P, full = MB * 64, 2.0 * MB * 64 * 9 * 2048 * ASPP
    for dtype in ("bf16", "f32"):
        m, head = nets(dtype)
        plain, recs = profile_of(m, head, x)
        mine = [r for r in recs if r["layer"] == "segmentation"]
        assert [r["op"] for r in mine] == OPS
        assert all(r["ms"] > 0 for r in mine)
        f = {r["op"]: r["flops"] for r in mine}
        assert f["aspp_conv0"] == full / 9 and f["aspp_conv1"] == f["aspp_conv2"] == full
        assert f["aspp_conv3"] == (full / 9 if dtype == "bf16" else full)
        assert f["aspp_pool"] == f["aspp_concat"] == f["seg_upsample"] == 0
        assert f["aspp_pool_conv"] == 2.0 * MB * 2048 * ASPP and f["aspp_project"] == 2.0 * P * 5 * ASPP * ASPP
        assert f["seg_conv1"] == 2.0 * P * 9 * ASPP * ASPP and f["seg_conv2"] == 2.0 * P * ASPP * 24
        rest = [(r["op"], r["layer"]) for r in recs if r["layer"] != "segmentation"]
        assert rest == [(r["op"], r["layer"]) for r in plain]
        head.center_tap(False)
        _, recs = profile_of(m, head, x)
        head.center_tap(True)
        off = {r["op"]: r["flops"] for r in recs if r["layer"] == "segmentation"}
        assert off["aspp_conv3"] == full and off["aspp_conv1"] == full


def test_fcn_head_on_the_same_model_keeps_its_bits(nets):
    """two heads share one model: the FCN head before and after a DeepLab forward"""
    m, head = nets()
    x = images()
    fcn = S.FCNHead(m.features, CLASSES, S.generate_fcn_head_state(m.features, CLASSES, seed=0), ctx=m.ctx)
    try:
        first = m.forward_segment(x, fcn, labels=True, scores=True)
        deep = m.forward_segment(x, head, labels=True, scores=True)
        second = m.forward_segment(x, fcn, labels=True, scores=True)
        again = m.forward_segment(x, head, labels=True, scores=True)
    finally:
        fcn.close()
    assert np.array_equal(bits(first["scores"]), bits(second["scores"])) and np.array_equal(first["labels"], second["labels"])
    assert np.array_equal(bits(deep["scores"]), bits(again["scores"])) and np.array_equal(deep["labels"], again["labels"])
    assert not np.array_equal(first["labels"], deep["labels"])
