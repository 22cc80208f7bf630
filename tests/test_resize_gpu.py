"""Decoded images of any size on the device: rn_image_u8_resize_crop must write the bytes of
preprocess.resize_crop_u8 (PIL's antialiased bilinear resize, short side 256, centre crop 224), and
the routes built on it -- NativeModel.forward_images, Pipeline(input="images"), rn_infer --rgb -- the
logits of the byte route on those crops.  Every comparison is np.array_equal."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import ops
from resnet_c_amd import preprocess as P
from resnet_c_amd.tensor import _DeviceBuffer

import views as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JPEG = os.path.join(ROOT, "tests", "golden", "ILSVRC2012_val_00004749.jpeg")
SIZES = [(375, 500), (500, 375), (256, 256), (224, 224), (100, 130), (1080, 1920), (333, 257), (256, 341), (64, 48),
         (2000, 300)]
U64P = ctypes.POINTER(ctypes.c_uint64)


def random_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def mixed():
    """One image of every size in the list.  Only 333 x 257 has a byte count that is no multiple of 4,
    so three small odd-sized images stand between them: packed back to back, the images of the list
    start on every byte residue mod 4."""
    extra = [(33, 35), (45, 47), (51, 9)]
    order = [extra[0]] + SIZES[:3] + [extra[1]] + SIZES[3:6] + [extra[2]] + SIZES[6:]
    imgs = [random_image(h, w, 31 * h + w) for h, w in order]
    _, offsets, _, _ = ops.pack_images(imgs)
    assert {int(o) % 4 for o in offsets} == {0, 1, 2, 3} and any(int(o) % 2 for o in offsets)
    return imgs


@pytest.fixture(scope="module")
def batch130():
    """130 images of mixed sizes (every size of the list several times, not grouped) and their crops: two
    parts of 65 images, the smallest batch the driver runs on two streams (parts of at least 64)."""
    small = [s for s in SIZES if s != (1080, 1920)]
    imgs = [random_image(*small[i % len(small)], seed=1000 + i) for i in range(128)]
    imgs.insert(17, random_image(1080, 1920, 5))
    imgs.insert(100, random_image(1080, 1920, 6))
    crops = np.stack([P.resize_crop_u8(a) for a in imgs])
    return imgs, crops


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_op_equals_resize_crop_u8_one_image_per_call(hw):
    px = random_image(*hw, seed=hw[0] + 3 * hw[1])
    got = ops.image_u8_resize_crop([px])
    want = P.resize_crop_u8(px)
    assert got.shape == (1, 224, 224, 3) and got.dtype == np.uint8
    assert np.array_equal(got[0], want), (hw, int((got[0] != want).sum()))


@pytest.mark.parametrize("resize,crop", [(256, 224), (232, 224), (256, 256)])
def test_op_equals_resize_crop_u8_in_one_mixed_batch(mixed, resize, crop):
    got = ops.image_u8_resize_crop(mixed, resize, crop)
    assert got.shape == (len(mixed), crop, crop, 3)
    for i, px in enumerate(mixed):
        want = P.resize_crop_u8(px, resize, crop)
        assert np.array_equal(got[i], want), (px.shape, resize, crop, int((got[i] != want).sum()))


def test_op_with_other_crops_and_band_shapes():
    """crop 64 (one column of accumulators), 300 (four), 512 (six) and 700 (twelve: a band of two rows)."""
    imgs = [random_image(800, 1200, 1), random_image(701, 700, 2), random_image(90, 70, 3)]
    for resize, crop in ((64, 64), (320, 300), (512, 512), (700, 700)):
        got = ops.image_u8_resize_crop(imgs, resize, crop)
        for i, px in enumerate(imgs):
            assert np.array_equal(got[i], P.resize_crop_u8(px, resize, crop)), (px.shape, resize, crop)


def test_op_at_a_large_reduction():
    """Scale 20: a band reads more source rows than the block's LDS holds and takes several rounds."""
    px = random_image(5200, 5120, 9)
    assert np.array_equal(ops.image_u8_resize_crop([px])[0], P.resize_crop_u8(px))


def run_on_views(imgs, resize, crop, src_off, dst_off):
    packed, offsets, heights, widths = ops.pack_images(imgs)
    vi = V.place(packed, src_off)
    vo = V.place_out(len(imgs) * crop * crop * 3, dst_off)
    V.must("rn_image_u8_resize_crop", vi.ptr, offsets.ctypes.data_as(U64P), heights.ctypes.data_as(U64P),
           widths.ctypes.data_as(U64P), len(imgs), vo.ptr, resize, crop)
    V.check_guards("rn_image_u8_resize_crop", vi)
    return V.fetch(vo, np.uint8, f"rn_image_u8_resize_crop dst+{dst_off}").reshape(len(imgs), crop, crop, 3)


@pytest.mark.parametrize("dst_off", [0, 1, 2, 3, 7])
def test_op_writes_between_guard_bands(mixed, dst_off):
    imgs = [a for a in mixed if a.shape[0] != 1080]            # (the largest image adds nothing here)
    got = run_on_views(imgs, 256, 224, src_off=(dst_off * 5) % 4, dst_off=dst_off)
    for i, px in enumerate(imgs):
        assert np.array_equal(got[i], P.resize_crop_u8(px)), (px.shape, dst_off)


def test_op_refusals_launch_nothing():
    ctx, lib = R.get_ctx(), L.lib()
    px = random_image(64, 48, 1)
    src = ops._up_raw(px)
    view = V.place_out(224 * 224 * 3)
    h = ctx.handle

    def call(ptr, offs, hs, ws, B, dst, resize, crop, ctxh=h):
        a = [np.array(v, dtype=np.uint64) if v is not None else None for v in (offs, hs, ws)]
        p = [v.ctypes.data_as(U64P) if v is not None else None for v in a]
        return lib.rn_image_u8_resize_crop(ctxh, ptr, p[0], p[1], p[2], B, dst, resize, crop)

    before = lib.rn_ctx_launch_count(h)
    bad = [
        call(None, [0], [64], [48], 1, view.ptr, 256, 224),
        call(src.ptr, None, [64], [48], 1, view.ptr, 256, 224),
        call(src.ptr, [0], None, [48], 1, view.ptr, 256, 224),
        call(src.ptr, [0], [64], None, 1, view.ptr, 256, 224),
        call(src.ptr, [0], [64], [48], 1, None, 256, 224),
        call(src.ptr, [0], [0], [48], 1, view.ptr, 256, 224),          # zero dimensions
        call(src.ptr, [0], [64], [0], 1, view.ptr, 256, 224),
        call(src.ptr, [0, 0], [64, 0], [48, 48], 2, view.ptr, 256, 224),
        call(src.ptr, [0], [64], [48], 1, view.ptr, 224, 256),         # crop > resize
        call(src.ptr, [0], [64], [48], 1, view.ptr, 256, 0),           # crop == 0
        call(src.ptr, [0], [16385], [48], 1, view.ptr, 256, 224),      # sides over 16384
        call(src.ptr, [0], [64], [16385], 1, view.ptr, 256, 224),
        call(src.ptr, [0], [64], [48], 1, view.ptr, 16385, 224),
        call(src.ptr, [0], [64], [48], 1, view.ptr, 4096, 2049),       # crop over 2048
        call(src.ptr, [0], [16384], [16384], 1, view.ptr, 224, 224),   # scale over 64
    ]
    assert bad == [L.RN_ERR_INVALID] * len(bad), bad
    assert call(src.ptr, [0], [64], [48], 1, view.ptr, 256, 224, ctxh=None) == L.RN_ERR_INVALID
    assert lib.rn_ctx_launch_count(h) == before
    ctx.sync()
    V.assert_untouched(view, "refused calls")
    assert call(None, None, None, None, 0, None, 256, 224) == L.RN_OK       # nothing to do
    assert lib.rn_ctx_launch_count(h) == before
    assert call(src.ptr, [0], [64], [48], 1, view.ptr, 256, 224) == L.RN_OK
    assert lib.rn_ctx_launch_count(h) == before + 1
    ctx.sync()
    assert np.array_equal(V.fetch(view, np.uint8, "after").reshape(224, 224, 3), P.resize_crop_u8(px))


# ---- model driver ---------------------------------------------------------------------------------

def check_model(arch, dtype, modes, imgs, crops):
    m = R.NativeModel(arch, state=R.weights.generate_state(arch, seed=0), dtype=dtype)
    try:
        m.set_streams(2)
        for fused in modes:
            got, want = m.forward_images(imgs, fused=fused), m.forward_u8(crops, fused=fused)
            assert got.shape == (len(imgs), 1000) and np.isfinite(got).all()
            assert np.array_equal(got, want), (arch, dtype, fused)
    finally:
        m.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_resnet50_forward_images_equals_forward_u8_on_the_crops(dtype, state50, batch130):
    imgs, crops = batch130
    m = R.NativeModel("resnet50", state=state50, dtype=dtype)
    try:
        m.set_streams(2)             # a count the caller set: parts of 64 images and more, fp32 too
        assert len(imgs) >= 70 and m.parts(len(imgs)) == 2
        for fused in ((True, False) if dtype == "f32" else (True,)):
            got, want = m.forward_images(imgs, fused=fused), m.forward_u8(crops, fused=fused)
            assert np.array_equal(got, want) and np.isfinite(got).all(), (dtype, fused)
        m.set_streams(0)
        assert np.array_equal(m.forward_images(imgs[:3]), m.forward_u8(crops[:3]))
    finally:
        m.close()


def test_resnext50_forward_images(batch130):
    imgs, crops = batch130
    check_model("resnext50_32x4d", "f32", (True,), imgs, crops)


def test_resnet18_forward_images(batch130):
    imgs, crops = batch130
    check_model("resnet18", "f32", (True,), imgs[:20], crops[:20])


def test_forward_images_profiles_the_resize_launch(state50, batch130):
    imgs, _ = batch130
    m = R.NativeModel("resnet50", state=state50)
    try:
        m.set_profiling(True)
        m.forward_images(imgs[:8])
        rec = m.profile()
        assert rec[0]["op"] == "image_u8_resize_crop" and rec[0]["layer"] == "input" and rec[0]["ms"] > 0
        assert rec[1]["op"].startswith("image_u8_to_nhwc") and rec[1]["layer"] == "input"
        m.set_profiling(False)
    finally:
        m.close()


def test_forward_images_refuses_bad_arguments(state50):
    m = R.NativeModel("resnet50", state=state50)
    try:
        lib, buf = L.lib(), _DeviceBuffer(m.ctx, 64 * 48 * 3)
        out = R.FloatTensor((1, 1000), R.Device.GPU)
        one = lambda v: np.array([v], dtype=np.uint64).ctypes.data_as(U64P)
        before = lib.rn_ctx_launch_count(m.ctx.handle)
        f = lib.rn_model_forward_images_u8
        assert f(m.handle, None, one(0), one(64), one(48), 1, out.data(), L.RN_FWD_FUSED) == L.RN_ERR_INVALID
        assert f(m.handle, buf.ptr, None, one(64), one(48), 1, out.data(), L.RN_FWD_FUSED) == L.RN_ERR_INVALID
        assert f(m.handle, buf.ptr, one(0), one(0), one(48), 1, out.data(), L.RN_FWD_FUSED) == L.RN_ERR_INVALID
        assert f(m.handle, buf.ptr, one(0), one(64), one(20000), 1, out.data(), L.RN_FWD_FUSED) == L.RN_ERR_INVALID
        assert f(m.handle, buf.ptr, one(0), one(64), one(48), 0, out.data(), L.RN_FWD_FUSED) == L.RN_ERR_INVALID
        assert f(m.handle, buf.ptr, one(0), one(64), one(48), 1, None, L.RN_FWD_FUSED) == L.RN_ERR_INVALID
        assert f(None, buf.ptr, one(0), one(64), one(48), 1, out.data(), L.RN_FWD_FUSED) == L.RN_ERR_INVALID
        assert lib.rn_ctx_launch_count(m.ctx.handle) == before
    finally:
        m.close()


def test_golden_jpeg_through_forward_images(state50):
    pytest.importorskip("PIL")
    m = R.NativeModel("resnet50", state=state50)
    try:
        got = m.forward_images([P.decode_image_u8(JPEG)])
        want = m.forward_u8(P.preprocess_image_u8(JPEG)[None])
        assert np.array_equal(got, want) and int(got.argmax(1)[0]) == 112
    finally:
        m.close()


# ---- host pipeline --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pipeline_images_equals_the_u8_pipeline_on_the_crops(dtype, state50, batch130):
    imgs, crops = batch130
    m = R.NativeModel("resnet50", state=state50, dtype=dtype)
    room = 64 << 20
    pi = R.Pipeline(m, 32, input="images", max_batch_bytes=room)
    pu = R.Pipeline(m, 32, input="u8")
    try:
        cuts = [(0, 32), (32, 64), (64, 74)]          # a ragged last batch of 10
        want = []
        for lo, hi in cuts:
            pu.submit_u8(crops[lo:hi])
            want.append(pu.collect_top1())
        got = []
        for lo, hi in cuts:                           # two in flight
            if pi.in_flight() == 2:
                got.append(pi.collect_top1())
            pi.submit_images(imgs[lo:hi])
        while pi.in_flight():
            got.append(pi.collect_top1())
        for (lo, hi), (gl, gi), (wl, wi) in zip(cuts, got, want):
            assert gl.shape == (hi - lo, 1000) and np.array_equal(gl, wl) and np.array_equal(gi, wi)
            assert np.array_equal(gi.astype(np.int64), gl.argmax(1))
        # a pipeline takes the input it was created for
        for bad in (lambda: pi.submit_u8(crops[:2]), lambda: pi.submit(P.normalize_u8(crops[:2])),
                    lambda: pu.submit_images(imgs[:2])):
            with pytest.raises(L.RnError) as e:
                bad()
            assert e.value.status == L.RN_ERR_INVALID and "input" in str(e.value)
        # a batch over max_batch_bytes
        with pytest.raises(L.RnError) as e:
            pi.submit_images([random_image(1080, 1920, 1)] * 12)    # 74.6 MB
        assert e.value.status == L.RN_ERR_INVALID and "max_batch_bytes" in str(e.value)
        with pytest.raises(L.RnError):
            pi.submit_images(imgs[:33])               # more images than the pipeline holds
        assert pi.in_flight() == 0
        pi.submit_images(imgs[:5])                    # and it still works
        assert np.array_equal(pi.collect(), m.forward_u8(crops[:5]))
    finally:
        pi.close()
        pu.close()
        m.close()


# ---- rn_infer -------------------------------------------------------------------------------------

def test_rn_infer_rgb_prints_what_u8_prints_on_the_crop(state50, tmp_path):
    wdir = tmp_path / "weights_bin"
    R.weights.save_weights_bin(state50, str(wdir))
    exe = os.path.join(os.path.dirname(R._lib.LIB_PATH), "rn_infer")

    def run(*args):
        return subprocess.run([exe, "--arch", "50", "--weights", str(wdir)] + [str(a) for a in args],
                              capture_output=True, text=True, timeout=300)

    px = random_image(375, 500, 4242)
    px.tofile(tmp_path / "img.rgb")
    P.resize_crop_u8(px)[None].tofile(tmp_path / "img.u8")
    a, b = run("--rgb", tmp_path / "img.rgb", "--hw", "375,500"), run("--u8", tmp_path / "img.u8")
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    la, lb = re.findall(r"max index is \d+", a.stdout), re.findall(r"max index is \d+", b.stdout)
    assert la == lb and len(la) == 1
    for extra in (["--dtype", "bf16"], ["--mode", "ops"]):
        a, b = run("--rgb", tmp_path / "img.rgb", "--hw", "375,500", *extra), run("--u8", tmp_path / "img.u8", *extra)
        assert a.returncode == 0 and re.findall(r"max index is \d+", a.stdout) == re.findall(r"max index is \d+", b.stdout)
    bad = run("--rgb", tmp_path / "img.rgb", "--hw", "375,499")
    assert bad.returncode != 0 and "--rgb" in bad.stderr and "max index" not in bad.stdout
    bad = run("--rgb", tmp_path / "img.rgb")
    assert bad.returncode != 0 and "--hw" in bad.stderr
