"""Segmentation on the GPU: rn_upsample_bilinear_forward, rn_seg_head_* and rn_model_forward_segment(_u8).

The op is held bit for bit to segmentation.upsample_bilinear_ref (the contract of include/rn_hip.h in numpy, itself
held to torch by tests/test_segmentation_host.py) on views between guard bands (tests/views.py): sources between NaN
guards with +1e30 in the padding channels, outputs filled with 0xA5 that must come back written everywhere.  The
head is held to the float64 torch reference fcn_head_ref on the same map; the model hook to fcn_head_ref on the
layer4 map the same model hands out (which isolates the head) and, once, to the float64 network end to end.
Everything that only reschedules the same arithmetic must not change a bit.
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
from test_dilation_gpu import TOL, bits, state_of, tol_bf16, tol_f32
from test_segmentation_host import OP_SHAPES, op_reference, op_source
from test_stage_maps_host import stage_maps_f64

pytestmark = pytest.mark.gpu

OFFSETS = ((0, 0), (4, 1), (12, 3))  # (scores, labels) destination offsets in bytes from a 16-byte boundary


def launches():
    return int(L.lib().rn_ctx_launch_count(R.get_ctx().handle))


def run_op(x, classes, size, want_scores, want_labels, s_off=0, l_off=0):
    """ONE rn_upsample_bilinear_forward on views: guards intact, every requested element written"""
    B, h, w, cs = x.shape
    H, Wd = size
    what = f"rn_upsample_bilinear_forward {x.shape} classes={classes} -> {size} scores={want_scores}+{s_off} labels={want_labels}+{l_off}"
    vi = V.place(x)
    vs = V.place_out(B * classes * H * Wd * 4, s_off) if want_scores else None
    vl = V.place_out(B * H * Wd, l_off) if want_labels else None
    before = launches()
    V.must("rn_upsample_bilinear_forward", vi.ptr, B, h, w, classes, cs, H, Wd, vs.ptr if vs else None,
           vl.ptr if vl else None)
    assert launches() - before == 1, what                         # one launch, whatever is requested
    V.check_guards(what, vi)
    scores = V.fetch(vs, np.float32, what, written=True).reshape(B, classes, H, Wd) if vs else None
    # a label byte may legitimately equal the 0xA5 fill (class 165): the written-everywhere check needs fewer classes
    labels = V.fetch(vl, np.uint8, what, written=classes <= V.OUT_BYTE).reshape(B, H, Wd) if vl else None
    return scores, labels


# =====================================================================================================================
# 1. the op, bit for bit
# =====================================================================================================================
@pytest.mark.parametrize("shape", OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_is_the_contract_bit_for_bit(shape):
    B, h, w, classes, cs, H, Wd = shape
    x = op_source(shape)
    want_s, want_l = op_reference(shape)
    V.assert_no_poison(want_s, False, f"{shape}")
    if classes == 256:
        assert (want_l == 255).any()
    if classes == 1:
        assert not want_l.any()
    for s_off, l_off in OFFSETS:
        for ws, wl in ((True, False), (False, True), (True, True)):
            got_s, got_l = run_op(x, classes, (H, Wd), ws, wl, s_off, l_off)
            what = f"{shape} scores={ws}+{s_off} labels={wl}+{l_off}"
            if ws:
                bad = np.flatnonzero(bits(got_s) != bits(want_s))
                assert bad.size == 0, (what, bad.size, np.unravel_index(bad[0], want_s.shape))
            if wl:
                bad = np.flatnonzero(got_l != want_l)
                assert bad.size == 0, (what, bad.size, np.unravel_index(bad[0], want_l.shape))


def test_op_python_wrapper():
    shape = OP_SHAPES[2]
    B, h, w, classes, cs, H, Wd = shape
    want_s, want_l = op_reference(shape)
    s, lb = ops.upsample_bilinear(op_source(shape), (H, Wd), classes, scores=True, labels=True)
    assert np.array_equal(bits(s), bits(want_s)) and np.array_equal(lb, want_l)
    s, lb = ops.upsample_bilinear(op_source(shape), (H, Wd), classes, scores=False, labels=True)
    assert s is None and np.array_equal(lb, want_l)


# =====================================================================================================================
# 2. ties
# =====================================================================================================================
def test_ties_take_the_lowest_index():
    """integer-valued scores, channels 3 and 7 identical and largest everywhere: every interpolated value of the
    two is the same float, the label is 3"""
    x = np.random.default_rng(17).integers(-4, 4, (2, 5, 4, 12)).astype(np.float32)
    x[..., 3] = 9.0
    x[..., 7] = 9.0
    for size in ((19, 22), (5, 4), (3, 2)):
        _, want = S.upsample_bilinear_ref(x, size, 10)
        assert (want == 3).all()
        for ws in (False, True):
            _, got = run_op(x, 10, size, ws, True, 0, 1)
            assert (got == 3).all(), (size, ws)


# =====================================================================================================================
# 3. refusals
# =====================================================================================================================
def test_op_refusals_launch_nothing():
    x = op_source(OP_SHAPES[0])
    B, h, w, classes, cs, H, Wd = OP_SHAPES[0]
    vi = V.place(x)
    vs, vl = V.place_out(B * classes * H * Wd * 4 + 16), V.place_out(B * H * Wd)
    ok = (vi.ptr, B, h, w, classes, cs, H, Wd, vs.ptr, vl.ptr)

    def args(**kw):
        names = ("src", "B", "h", "w", "classes", "cs", "H", "W", "scores", "labels")
        a = dict(zip(names, ok))
        a.update(kw)
        return tuple(a[n] for n in names)

    cases = [(args(src=None), "src_nhwc"), (args(scores=None, labels=None), "outputs"), (args(classes=0), "classes"),
             (args(classes=257, cs=260), "classes"), (args(cs=20), "src_channels"), (args(cs=22), "src_channels"),
             (args(classes=21, cs=260), "src_channels"), (args(src=vi.ptr + 4), "src_nhwc"),
             (args(scores=vs.ptr + 2), "scores_nchw"), (args(H=0), "H"), (args(w=0), "w")]
    before = launches()
    for a, word in cases:
        st, msg = V.call("rn_upsample_bilinear_forward", *a)
        assert st == L.RN_ERR_INVALID and word in msg, (a, st, msg)
    assert L.lib().rn_upsample_bilinear_forward(None, *ok) == L.RN_ERR_INVALID        # no context
    V.must("rn_upsample_bilinear_forward", *args(B=0))                               # an empty batch launches nothing
    assert launches() == before
    V.assert_untouched(vs, "refused or empty: scores")
    V.assert_untouched(vl, "refused or empty: labels")
    V.check_guards("refusals", vi)


# =====================================================================================================================
# 4. the head alone
# =====================================================================================================================
HEAD_CASES = [(128, 21, (2, 6, 5), (24, 20)), (512, 7, (1, 4, 4), (32, 32))]


@functools.lru_cache(maxsize=None)
def head_case(cin, classes, bhw, size, dtype):
    """(map NHWC fp32, head state, float64 reference scores): computed once, shared, read-only"""
    B, h, w = bhw
    x = np.random.default_rng(cin + classes).standard_normal((B, h, w, cin), dtype=np.float32)
    st = S.generate_fcn_head_state(cin, classes, seed=1)
    ref = S.fcn_head_ref(x.transpose(0, 3, 1, 2).astype(np.float64), st, size,
                         round_fn=ops.bf16_round if dtype == "bf16" else None)
    x.setflags(write=False), ref.setflags(write=False)
    return x, st, ref


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cin,classes,bhw,size", HEAD_CASES, ids=["128x21", "512x7"])
def test_head_alone(cin, classes, bhw, size, dtype):
    """scores within tol_f32(ref, 9 * in_channels) (fp32) or tol_bf16(ref) (bf16: the reference rounds the map, both
    weights and the mid tensor where the device does) of the float64 head; labels = numpy.argmax of the scores of
    the same call, and the same from a labels-only call"""
    x, st, ref = head_case(cin, classes, bhw, size, dtype)
    head = S.FCNHead(cin, classes, st, dtype=dtype)
    try:
        scores, labels = head.forward(x, size, scores=True, labels=True)
        assert scores.shape == ref.shape and labels.shape == (bhw[0],) + size
        tol = tol_f32(ref, 9 * cin) if dtype == "f32" else tol_bf16(ref)
        err = float(np.abs(scores - ref).max())
        print(f"\n  FCNHead({cin}, {classes}) {dtype}: max|gpu - fp64| = {err:.3e}, bound {tol:.3e}, max|ref| = {np.abs(ref).max():.3f}")
        assert err <= tol
        assert np.array_equal(labels, scores.argmax(axis=1))
        assert len(np.unique(labels)) >= 3
        none, only = head.forward(x, size, scores=False, labels=True)
        assert none is None and np.array_equal(only, labels)
        again, _ = head.forward(x, size, scores=True, labels=False)
        assert np.array_equal(bits(again), bits(scores))
    finally:
        head.close()


def test_head_refusals():
    ctx, lib = R.get_ctx(), L.lib()
    h = ctypes.c_void_p()
    for bad in ((100, 64, 21), (128, 0, 21), (128, 64, 0), (128, 64, 257)):
        assert lib.rn_seg_head_create(ctx.handle, ctypes.byref(h), *bad) == L.RN_ERR_INVALID and not h.value, bad
    assert lib.rn_seg_head_create(ctx.handle, ctypes.byref(h), 128, 32 * 2, 5) == L.RN_OK
    try:
        w = np.zeros(7, np.float32)
        assert lib.rn_seg_head_set_tensor(h, b"classifier.9.weight", w.ctypes.data, 7) == L.RN_ERR_INVALID
        assert lib.rn_seg_head_set_tensor(h, b"classifier.4.bias", w.ctypes.data, 7) == L.RN_ERR_INVALID   # 5 classes
        assert lib.rn_seg_head_finalize(h) == L.RN_ERR_INVALID                        # tensors missing
        assert b"classifier.0.weight" in lib.rn_last_error(ctx.handle)
        v = V.place(np.zeros((1, 2, 2, 128), np.float32))
        vo = V.place_out(4 * 4)
        assert lib.rn_seg_head_forward(h, v.ptr, 1, 2, 2, 4, 4, None, vo.ptr) == L.RN_ERR_INVALID   # not finalized
        V.assert_untouched(vo, "head not finalized")
    finally:
        lib.rn_seg_head_destroy(h)


# =====================================================================================================================
# 4b. the head's bookkeeping: padding in its general form (scratch growth and a tensor set twice: every kind of object
#     shares that code, test_stage_objects_gpu.py)
# =====================================================================================================================
PAD_SEED = 2   # the float64 reference labels of this seed hold all three classes, fp32 and bf16 (17, 14 and 32 pixels)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_head_padding_in_general(dtype):
    """FCNHead(64, 3, mid_channels=20): mid 20 -> 64 and classes 3 -> 4, neither count a multiple of 4.  The bounds of
    test_head_alone; the added channels must add exact zeros and the added class must never be a label"""
    cin, classes, mid, size = 64, 3, 20, (7, 9)
    x = np.random.default_rng(20).standard_normal((1, 3, 5, cin), dtype=np.float32)
    st = S.generate_fcn_head_state(cin, classes, seed=PAD_SEED, mid_channels=mid)
    ref = S.fcn_head_ref(x.transpose(0, 3, 1, 2).astype(np.float64), st, size,
                         round_fn=ops.bf16_round if dtype == "bf16" else None)
    assert len(np.unique(ref.argmax(axis=1))) >= 2
    head = S.FCNHead(cin, classes, st, dtype=dtype, mid_channels=mid)
    try:
        assert head.mid_channels == mid
        scores, labels = head.forward(x, size, scores=True, labels=True)
    finally:
        head.close()
    tol = tol_f32(ref, 9 * cin) if dtype == "f32" else tol_bf16(ref)
    err = float(np.abs(scores - ref).max())
    print(f"\n  FCNHead({cin}, {classes}, mid {mid}) {dtype}: max|gpu - fp64| = {err:.3e}, bound {tol:.3e}")
    assert scores.shape == ref.shape and err <= tol
    assert np.array_equal(labels, scores.argmax(axis=1))
    assert len(np.unique(labels)) >= 2


def small_head(kind, dtype="f32", rates=(1, 2)):
    """(constructor of a 64-channel, 5-class head of either kind, its state, its shapes, the C create call and its
    arguments behind in_channels)"""
    if kind == "fcn":
        st = S.generate_fcn_head_state(64, 5, seed=3)
        return (lambda: S.FCNHead(64, 5, st, dtype=dtype)), st, S.head_shapes(64, 5), "rn_seg_head_create", (16, 5)
    st = S.generate_deeplab_head_state(64, 5, 64, rates, seed=3)
    rates_c = (ctypes.c_uint64 * len(rates))(*rates)
    return ((lambda: S.DeepLabHead(64, 5, st, aspp_channels=64, rates=rates, dtype=dtype)), st,
            S.deeplab_head_shapes(64, 5, 64, rates), "rn_seg_head_create_deeplab", (64, 5, len(rates), rates_c))


# =====================================================================================================================
# 5. the model
# =====================================================================================================================
SIZE, FLAGS, CLASSES, MB = (64, 64), (0, 1, 1), 21, 3
HEAD_SEED = 0   # the float64 reference labels of this seed hold four classes on >= 5 % of the pixels each


@functools.lru_cache(maxsize=None)
def images(n=MB):
    x = W.generate_input(n, seed=300 + SIZE[0] + SIZE[1], hw=SIZE)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def head_state(cin=2048):
    return S.generate_fcn_head_state(cin, CLASSES, seed=HEAD_SEED)


@pytest.fixture(scope="module")
def nets():
    made = {}

    def get(arch="resnet50", dtype="f32"):
        if (arch, dtype) not in made:
            basic = arch == "resnet18"
            m = R.NativeModel(arch, state=state_of(arch), dtype=dtype, input_size=SIZE,
                              replace_stride_with_dilation=None if basic else FLAGS)
            made[(arch, dtype)] = (m, S.FCNHead(m.features, CLASSES, head_state(m.features), dtype=dtype))
        m, head = made[(arch, dtype)]
        m.set_streams(0)
        return m, head
    yield get
    for m, head in made.values():
        head.close()
        m.close()


def check_isolated(m, head, x, dtype):
    """the head against fcn_head_ref on the layer4 map the same model returns for the same images"""
    maps = m.forward_maps(x, ("layer4",))["layer4"]
    ref = S.fcn_head_ref(maps.astype(np.float64), head_state(m.features), SIZE,
                         round_fn=ops.bf16_round if dtype == "bf16" else None)
    got = m.forward_segment(x, head, labels=True, scores=True)
    assert list(got) == ["labels", "scores"]
    assert got["scores"].shape == ref.shape == (x.shape[0], CLASSES) + SIZE and got["labels"].shape == (x.shape[0],) + SIZE
    tol = tol_f32(ref, 9 * m.features) if dtype == "f32" else tol_bf16(ref)
    err = float(np.abs(got["scores"] - ref).max())
    print(f"\n  forward_segment {m.arch} {dtype}: max|gpu - fp64 head on the gpu's map| = {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    assert np.array_equal(got["labels"], got["scores"].argmax(axis=1))
    only = m.forward_segment(x, head)
    assert list(only) == ["labels"] and np.array_equal(only["labels"], got["labels"])
    return got


def test_model_head_isolated_fp32(nets):
    m, head = nets()
    assert m.stage_shapes["layer4"] == (2048, 8, 8)
    check_isolated(m, head, images(), "f32")


def test_model_head_isolated_bf16(nets):
    m, head = nets("resnet50", "bf16")
    check_isolated(m, head, images(), "bf16")


def test_model_resnet18_undilated(nets):
    m, head = nets("resnet18")
    assert m.stage_shapes["layer4"] == (512, 2, 2) and head.mid_channels == 128
    check_isolated(m, head, images(), "f32")


def test_model_end_to_end_fp32(nets):
    """scores within TOL * max|ref| + 1e-6 of the float64 network + float64 head; labels equal the reference's
    wherever its top-two gap exceeds twice that, at most 1 % of the pixels left out; the reference labels hold at
    least three classes on at least 5 % of the pixels each (checked before anything runs on the GPU)"""
    x = images()
    ref = S.fcn_head_ref(stage_maps_f64("resnet50", state_of("resnet50"), x, FLAGS)[3], head_state(), SIZE)
    tol = TOL * float(np.abs(ref).max()) + 1e-6
    ref_labels = ref.argmax(axis=1)
    share = np.bincount(ref_labels.reshape(-1), minlength=CLASSES) / ref_labels.size
    assert (share >= 0.05).sum() >= 3, share
    top2 = np.sort(ref, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * tol
    assert 1.0 - clear.mean() <= 0.01
    m, head = nets()
    got = m.forward_segment(x, head, labels=True, scores=True)
    err = float(np.abs(got["scores"] - ref).max())
    print(f"\n  forward_segment end to end: max|gpu - fp64| = {err:.3e}, bound {tol:.3e}; {100 * (1 - clear.mean()):.2f} % of "
          f"the pixels inside twice the bound; classes on >= 5 %: {np.flatnonzero(share >= 0.05).tolist()}")
    assert err <= tol
    assert np.array_equal(got["labels"], got["scores"].argmax(axis=1))
    assert np.array_equal(got["labels"][clear], ref_labels[clear])


def test_model_other_outputs_keep_their_bits(nets):
    m, head = nets()
    x = images()
    want = m.forward_outputs(x, logits=True, features=True)
    got = m.forward_segment(x, head, labels=True, scores=False, logits=True, features=True)
    assert list(got) == ["labels", "logits", "features"]
    for k in ("logits", "features"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    # the request does not outlive its call: a plain forward issues the launches it always did
    before = int(L.lib().rn_ctx_launch_count(m.ctx.handle))
    a = m.forward(x)
    plain = int(L.lib().rn_ctx_launch_count(m.ctx.handle)) - before
    # what the head launches on a map of layer4's shape when it runs alone (three entry points; a contraction may
    # count more than one launch)
    before = int(L.lib().rn_ctx_launch_count(m.ctx.handle))
    head.forward(np.zeros((MB, 8, 8, 2048), np.float32), SIZE, scores=False, labels=True)
    alone = int(L.lib().rn_ctx_launch_count(m.ctx.handle)) - before
    assert alone >= 3
    before = int(L.lib().rn_ctx_launch_count(m.ctx.handle))
    m.forward_segment(x, head)
    assert int(L.lib().rn_ctx_launch_count(m.ctx.handle)) - before == plain + alone
    before = int(L.lib().rn_ctx_launch_count(m.ctx.handle))
    assert np.array_equal(bits(m.forward(x)), bits(a))
    assert int(L.lib().rn_ctx_launch_count(m.ctx.handle)) - before == plain


def test_model_rescheduling_changes_no_bit(nets):
    m, head = nets()
    x = images()
    base = m.forward_segment(x, head, labels=True, scores=True)
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


def test_model_parts_on_two_streams(nets):
    """128 images as two parts of 64 on two streams, each in its own slice of the head's scratch: the bits of one
    stream, and of the three-image call for the images they share"""
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
    m18, head18 = nets("resnet18")
    _mb, headb = nets("resnet50", "bf16")
    lib = L.lib()
    x = ops._up_raw(images())
    vl = V.place_out(MB * SIZE[0] * SIZE[1])
    seg = L.SegOutputs(vl.ptr, None)
    raw = ctypes.c_void_p()
    assert lib.rn_seg_head_create(m.ctx.handle, ctypes.byref(raw), 2048, 512, CLASSES) == L.RN_OK   # never finalized

    def call(model, hd, seg_ptr):
        st = lib.rn_model_forward_segment(model.handle, hd, x.ptr, MB, None, seg_ptr, L.RN_FWD_FUSED)
        return st, (lib.rn_last_error(model.ctx.handle) or b"").decode()

    try:
        before = int(lib.rn_ctx_launch_count(m.ctx.handle))
        for hd, seg_ptr, word in ((head18.handle, ctypes.byref(seg), "in_channels"), (headb.handle, ctypes.byref(seg), "dtype"),
                                  (raw, ctypes.byref(seg), "not finalized"), (head.handle, None, "seg is NULL"),
                                  (head.handle, ctypes.byref(L.SegOutputs(None, None)), "names nothing"),
                                  (None, ctypes.byref(seg), "head is NULL")):
            st, msg = call(m, hd, seg_ptr)
            assert st == L.RN_ERR_INVALID and word in msg, (word, st, msg)
        st, msg = call(m18, head.handle, ctypes.byref(seg))
        assert st == L.RN_ERR_INVALID and "in_channels" in msg
        assert int(lib.rn_ctx_launch_count(m.ctx.handle)) == before
        m.ctx.sync()
        V.assert_untouched(vl, "refused segment calls")
        st, msg = call(m, head.handle, ctypes.byref(seg))                 # and the call they all almost were
        assert st == L.RN_OK, msg
        m.ctx.sync()
        want = m.forward_segment(images(), head)["labels"]
        assert np.array_equal(V.fetch(vl, np.uint8, "labels", written=True).reshape(want.shape), want)
    finally:
        lib.rn_seg_head_destroy(raw)


# =====================================================================================================================
# 6. rn_infer --segment, the profile records
# =====================================================================================================================
def test_rn_infer_segment(tmp_path, nets):
    import os
    import subprocess
    wdir, hdir = tmp_path / "weights_bin", tmp_path / "head_bin"
    os.mkdir(wdir), os.mkdir(hdir)
    W.save_weights_bin(state_of("resnet50"), str(wdir))
    for key, arr in head_state().items():
        np.ascontiguousarray(arr, dtype=np.float32).tofile(hdir / key)
    x = images()[:2]
    inp, out = tmp_path / "in_64x64.bin", tmp_path / "labels.u8"
    np.ascontiguousarray(x).tofile(inp)
    m, head = nets()
    want = m.forward_segment(x, head, labels=True, logits=True)
    exe = os.path.join(os.path.dirname(L.LIB_PATH), "rn_infer")
    base = [exe, "--weights", str(wdir), "--batch", "2", "--size", "64,64", "--input", str(inp), "--arch", "50",
            "--dilate", "0,1,1"]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    r = subprocess.run(base + ["--segment", str(hdir), "--labels", str(out)], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    assert r.stdout == plain.stdout                                        # the lines printed are unchanged
    assert [int(l.split()[-1]) for l in r.stdout.splitlines() if l.startswith("max index is")] == want["logits"].argmax(1).tolist()
    got = np.fromfile(out, dtype=np.uint8)
    assert got.size == 2 * SIZE[0] * SIZE[1] and np.array_equal(got.reshape(want["labels"].shape), want["labels"])
    alone = subprocess.run(base + ["--segment", str(hdir)], capture_output=True, text=True, timeout=120)
    assert alone.returncode != 0 and "--labels" in alone.stderr


def test_profile_records(nets):
    m, head = nets()
    x = images()
    m.forward_segment(x, head)
    m.set_profiling(True)
    try:
        m.forward_outputs(x, logits=True)
        plain = m.profile()
        m.forward_segment(x, head)
        recs = m.profile()
    finally:
        m.set_profiling(False)
    mine = [r for r in recs if r["layer"] == "segmentation"]
    assert [r["op"] for r in mine] == ["seg_conv1", "seg_conv2", "seg_upsample"]
    assert all(r["ms"] > 0 for r in mine) and mine[0]["flops"] == 2.0 * MB * 64 * 9 * 2048 * 512 and mine[2]["flops"] == 0
    rest = [(r["op"], r["layer"]) for r in recs if r["layer"] != "segmentation"]
    assert rest == [(r["op"], r["layer"]) for r in plain]
