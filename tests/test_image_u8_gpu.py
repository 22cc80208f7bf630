"""Byte input on the device: 8-bit RGB [B,H,W,3] normalised by the first launch
(rn_image_u8_to_nhwc_pad_dt) must give, bit for bit, what the float route gives on the
host-normalised image (preprocess.normalize_u8): first tensor, logits, top-1, through the op, the
model driver, the host pipeline, the shards and rn_infer.  Every comparison is np.array_equal; only
the committed golden logits carry the project's 1e-4."""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JPEG = os.path.join(ROOT, "tests", "golden", "ILSVRC2012_val_00004749.jpeg")


def random_bytes(B, H, W, seed):
    """Seeded bytes; where the image has room for it, every value 0..255 in every channel of every image."""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    if H * W >= 256:
        flat = px.reshape(B, H * W, 3)
        for b in range(B):
            for c in range(3):
                flat[b, rng.choice(H * W, 256, replace=False), c] = np.arange(256, dtype=np.uint8)
        for c in range(3):
            assert len(np.unique(px[0, :, :, c])) == 256
    return px


@pytest.fixture(scope="module")
def finch_px():
    return P.preprocess_image_u8(JPEG)[None]


def float_route_tensor(x, cpad, border, bf16):
    """rn_nchw_to_nhwc_pad_dt on the fp32 NCHW image: the raw bits of the tensor it writes."""
    ctx, lib = R.get_ctx(), L.lib()
    B, C, H, W = x.shape
    es, ht = (2, np.uint16) if bf16 else (4, np.uint32)
    n = B * (H + 2 * border) * (W + 2 * border) * cpad
    src = R.FloatTensor.from_numpy(np.ascontiguousarray(x), R.Device.GPU)
    dst = _DeviceBuffer(ctx, max(n * es, 16))
    L.check(lib.rn_memset(ctx.handle, dst.ptr, 0x5A, max(n * es, 16)), "memset", ctx.handle)
    L.check(lib.rn_nchw_to_nhwc_pad_dt(ctx.handle, L.RN_DTYPE_BF16 if bf16 else L.RN_DTYPE_F32, src.data(), dst.ptr,
                                       B, C, H, W, cpad, border), "rn_nchw_to_nhwc_pad_dt", ctx.handle)
    ctx.sync()
    got = np.empty(n, dtype=ht)
    L.check(lib.rn_memcpy_d2h(ctx.handle, got.ctypes.data, dst.ptr, got.nbytes), "d2h", ctx.handle)
    return got.reshape(B, H + 2 * border, W + 2 * border, cpad)


def byte_route_tensor(px, cpad, border, bf16, mean=None, std=None):
    """rn_image_u8_to_nhwc_pad_dt into a destination pre-filled with 0xA5 bytes, as raw bits."""
    got = ops.image_u8_to_nhwc_pad(px, cpad, border, bf16, mean, std, prefill=0xA5)
    return got if bf16 else got.view(np.uint32)


def check_op(px, cpad, border, bf16, mean=None, std=None):
    x = P.normalize_u8(px) if mean is None else P.normalize_u8(px, mean, std)
    want = float_route_tensor(x, cpad, border, bf16)
    got = byte_route_tensor(px, cpad, border, bf16, mean, std)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), (px.shape, cpad, border, bf16, int((got != want).sum()))
    # what the launch must have written itself: border and pad channels are zero, not the pre-fill
    B, H, W, _ = px.shape
    if border:
        assert not got[:, :border].any() and not got[:, -border:].any()
        assert not got[:, :, :border].any() and not got[:, :, -border:].any()
    if cpad == 4:
        assert not got[..., 3].any()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("cpad", [3, 4])
@pytest.mark.parametrize("border", [0, 3])
@pytest.mark.parametrize("B", [1, 3, 256])
def test_op_equals_the_float_route_at_the_network_shape(B, border, cpad, bf16):
    check_op(random_bytes(B, 224, 224, 100 + B + 10 * border + cpad), cpad, border, bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("cpad", [3, 4])
@pytest.mark.parametrize("border", [0, 3])
def test_op_on_the_finch_crop(finch_px, finch, border, cpad, bf16):
    assert np.array_equal(P.normalize_u8(finch_px), finch)
    check_op(finch_px, cpad, border, bf16)


# odd shapes and borders: 5x7, 33x17, 1x1, 7x1 cannot take the 16-byte form (H*W*3 is no multiple of 4,
# or the padded image no whole number of stores), 16x20 / 8x12 / 4x4 / 2x2 do where the border allows
# it (0 or >= 3), borders 1 and 2 never do
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("cpad", [3, 4])
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 33, 17), (3, 1, 1), (2, 7, 1), (2, 16, 20), (3, 8, 12), (5, 4, 4),
                                   (2, 2, 2), (1, 36, 28), (2, 1, 4), (2, 4, 1)])
def test_op_on_other_shapes_and_borders(shape, cpad, bf16):
    B, H, W = shape
    for border in (0, 1, 2, 3, 4, 5):
        check_op(random_bytes(B, H, W, 7 * H + W + border), cpad, border, bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_op_with_another_mean_and_std(bf16):
    mean, std = (0.5, 0.25, 0.125), (0.5, 2.0, 0.3)
    check_op(random_bytes(2, 224, 224, 5), 4, 3, bf16, mean, std)
    check_op(random_bytes(2, 33, 17, 6), 3, 3, bf16, mean, std)


def test_op_on_an_unaligned_image_pointer():
    """An image that does not start on a 4-byte boundary cannot take the dword loads: the element kernel."""
    ctx, lib = R.get_ctx(), L.lib()
    px = random_bytes(2, 16, 20, 77)
    raw = np.concatenate([np.zeros(1, np.uint8), px.reshape(-1)])
    src = ops._up_raw(raw)
    n = 2 * 22 * 26 * 4
    dst = _DeviceBuffer(ctx, n * 4)
    m3, s3 = (ctypes.c_float * 3)(*P.MEAN), (ctypes.c_float * 3)(*P.STD)
    L.check(lib.rn_image_u8_to_nhwc_pad_dt(ctx.handle, L.RN_DTYPE_F32, src.ptr + 1, dst.ptr, 2, 16, 20, 4, 3, m3, s3),
            "u8", ctx.handle)
    got = ops._down_raw(dst, np.uint32, n).reshape(2, 22, 26, 4)
    assert np.array_equal(got, float_route_tensor(P.normalize_u8(px), 4, 3, False))


def test_op_refuses_bad_arguments():
    ctx, lib = R.get_ctx(), L.lib()
    src, dst = _DeviceBuffer(ctx, 64), _DeviceBuffer(ctx, 4096)
    m3, s3 = (ctypes.c_float * 3)(*P.MEAN), (ctypes.c_float * 3)(*P.STD)
    h, f32 = ctx.handle, L.RN_DTYPE_F32
    assert lib.rn_image_u8_to_nhwc_pad_dt(h, f32, src.ptr, dst.ptr, 1, 4, 4, 4, 0, m3, s3) == L.RN_OK
    assert lib.rn_image_u8_to_nhwc_pad_dt(h, f32, None, dst.ptr, 1, 4, 4, 4, 0, m3, s3) == L.RN_ERR_INVALID
    assert lib.rn_image_u8_to_nhwc_pad_dt(h, f32, src.ptr, None, 1, 4, 4, 4, 0, m3, s3) == L.RN_ERR_INVALID
    assert lib.rn_image_u8_to_nhwc_pad_dt(h, f32, src.ptr, dst.ptr, 1, 4, 4, 4, 0, None, s3) == L.RN_ERR_INVALID
    assert lib.rn_image_u8_to_nhwc_pad_dt(h, f32, src.ptr, dst.ptr, 1, 4, 4, 4, 0, m3, None) == L.RN_ERR_INVALID
    for cpad in (0, 1, 2, 5):
        assert lib.rn_image_u8_to_nhwc_pad_dt(h, f32, src.ptr, dst.ptr, 1, 4, 4, cpad, 0, m3, s3) == L.RN_ERR_INVALID
    assert lib.rn_image_u8_to_nhwc_pad_dt(h, 7, src.ptr, dst.ptr, 1, 4, 4, 4, 0, m3, s3) == L.RN_ERR_INVALID
    assert lib.rn_image_u8_to_nhwc_pad_dt(None, f32, src.ptr, dst.ptr, 1, 4, 4, 4, 0, m3, s3) == L.RN_ERR_INVALID
    assert lib.rn_image_u8_to_nhwc_pad_dt(h, f32, None, None, 0, 4, 4, 4, 0, m3, s3) == L.RN_OK   # nothing to do
    ctx.sync()


# ---- model driver ---------------------------------------------------------------------------------

ARCHS = ["resnet18", "resnet34", "resnet50", "resnet101", "resnet152"]


@pytest.fixture(scope="module")
def batch_px():
    return random_bytes(128, 224, 224, 2024)


@pytest.fixture(scope="module")
def batch_x(batch_px):
    return P.normalize_u8(batch_px)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ARCHS)
def test_model_forward_u8_equals_forward_on_the_normalised_image(arch, dtype, batch_px, batch_x):
    """B = 1; an odd B through a depth-first front of two slices; B = 128 as two parts on two streams.
    fp32 fused and op by op, bf16 fused (bf16 storage exists only with the fused epilogues)."""
    m = R.NativeModel(arch, state=R.weights.generate_state(arch, seed=0), dtype=dtype)
    try:
        for fused in ((True, False) if dtype == "f32" else (True,)):
            m.set_front_parts(1)
            m.set_streams(0)
            assert np.array_equal(m.forward_u8(batch_px[5:6], fused=fused), m.forward(batch_x[5:6], fused=fused))
            m.set_front_parts(2)
            assert np.array_equal(m.forward_u8(batch_px[:33], fused=fused), m.forward(batch_x[:33], fused=fused))
            m.set_front_parts(1)
            m.set_streams(2)
            assert m.parts(128) == 2
            got, want = m.forward_u8(batch_px, fused=fused), m.forward(batch_x, fused=fused)
            assert np.array_equal(got, want) and np.isfinite(got).all()
    finally:
        m.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_model_forward_u8_one_stream_and_stem_from_nchw_setting(dtype, state50, batch_px, batch_x):
    m = R.NativeModel("resnet50", state=state50, dtype=dtype)
    try:
        base = m.forward(batch_x, fused=True)
        m.set_streams(1)
        assert m.parts(128) == 1
        assert np.array_equal(m.forward_u8(batch_px, fused=True), base)
        m.set_streams(0)
        # fusion 2 fetches the stem's patches from the caller's NCHW image; there is none on the byte
        # route, which runs the padded-image form: the logits of the float route at fusion 1
        m.set_stem_pool_fusion(2)
        got = m.forward_u8(batch_px[:37], fused=True)
        m.set_stem_pool_fusion(1)
        assert np.array_equal(got, m.forward(batch_x[:37], fused=True))
        m.set_stem_pool_fusion(0)
        assert np.array_equal(m.forward_u8(batch_px[:9], fused=True), m.forward(batch_x[:9], fused=True))
        m.set_stem_pool_fusion(1)
        if dtype == "f32":   # the stem that pads to four channels and no border
            m.set_stem_exact(False)
            assert np.array_equal(m.forward_u8(batch_px[:9], fused=True), m.forward(batch_x[:9], fused=True))
            assert np.array_equal(m.forward_u8(batch_px[:9], fused=False), m.forward(batch_x[:9], fused=False))
            m.set_stem_exact(True)
    finally:
        m.close()


def test_model_forward_u8_profiles_the_input_launch(state50, batch_px):
    m = R.NativeModel("resnet50", state=state50)
    try:
        m.set_profiling(True)
        m.forward_u8(batch_px[:8], fused=True)
        rec = m.profile()
        assert rec[0]["layer"] == "input" and rec[0]["op"].startswith("image_u8") and rec[0]["ms"] > 0
        assert rec[0]["bytes"] == 8 * (150528 + 4 * 230 * 230 * 3)
        m.set_profiling(False)
    finally:
        m.close()


def test_model_forward_u8_refuses_bad_arguments(state50):
    m = R.NativeModel("resnet50", state=state50)
    try:
        lib, buf = L.lib(), _DeviceBuffer(m.ctx, 150528)
        out = R.FloatTensor((1, 1000), R.Device.GPU)
        assert lib.rn_model_forward_u8(m.handle, None, 1, out.data(), L.RN_FWD_FUSED) == L.RN_ERR_INVALID
        assert lib.rn_model_forward_u8(m.handle, buf.ptr, 0, out.data(), L.RN_FWD_FUSED) == L.RN_ERR_INVALID
        assert lib.rn_model_forward_u8(m.handle, buf.ptr, 1, None, L.RN_FWD_FUSED) == L.RN_ERR_INVALID
        assert lib.rn_model_forward_u8(None, buf.ptr, 1, out.data(), L.RN_FWD_FUSED) == L.RN_ERR_INVALID
    finally:
        m.close()


def test_resnet50_on_the_finch_crop_matches_the_golden_logits(state50, finch_px, golden_dir):
    golden = np.load(os.path.join(golden_dir, "resnet50_finch_logits.npy"))
    m = R.NativeModel("resnet50", state=state50)
    try:
        for fused in (True, False):
            got = m.forward_u8(finch_px, fused=fused)
            err = float(np.abs(got - golden).max())
            print(f"finch crop, fused={fused}: max|byte route - golden| = {err:.3e}")
            assert err <= 1e-4
            assert int(got.argmax(1)[0]) == int(golden.argmax(1)[0]) == 112
    finally:
        m.close()


# ---- host pipeline --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pipeline_u8_equals_the_float_pipeline(dtype, state50, batch_px, batch_x):
    """Batches of 64 (four 16-image pieces: the helper threads copy), a ragged last one of 37 and a
    single image, from a pageable array, then whole batches written into the staging buffer."""
    m = R.NativeModel("resnet50", state=state50, dtype=dtype)
    pf = R.Pipeline(m, 64, input="f32")
    pu = R.Pipeline(m, 64, input="u8")
    try:
        cuts = [(0, 64), (64, 128), (3, 40), (127, 128)]
        want = []
        for lo, hi in cuts:
            pf.submit(batch_x[lo:hi])
            want.append(pf.collect_top1())
        got = []
        for lo, hi in cuts:          # two in flight
            if pu.in_flight() == 2:
                got.append(pu.collect_top1())
            pu.submit_u8(batch_px[lo:hi])
        while pu.in_flight():
            got.append(pu.collect_top1())
        for (lo, hi), (gl, gi), (wl, wi) in zip(cuts, got, want):
            assert gl.shape == (hi - lo, 1000) and np.array_equal(gl, wl) and np.array_equal(gi, wi)
            assert np.array_equal(gi.astype(np.int64), gl.argmax(1))
        for lo in (0, 64):           # producer writes into pinned staging
            buf = pu.input_buffer()
            assert buf.shape == (64, 224, 224, 3) and buf.dtype == np.uint8
            buf[...] = batch_px[lo:lo + 64]
            pu.submit_u8(None)
        for i in range(2):
            gl, gi = pu.collect_top1()
            assert np.array_equal(gl, want[i][0]) and np.array_equal(gi, want[i][1])
        # a pipeline takes the format it was created for
        for bad in (lambda: pu.submit(batch_x[:2]), lambda: pf.submit_u8(batch_px[:2]),
                    lambda: L.check(L.lib().rn_pipeline_input_buffer(pu.handle, ctypes.byref(ctypes.c_void_p())),
                                    "rn_pipeline_input_buffer", m.ctx.handle),
                    lambda: L.check(L.lib().rn_pipeline_input_buffer_u8(pf.handle, ctypes.byref(ctypes.c_void_p())),
                                    "rn_pipeline_input_buffer_u8", m.ctx.handle)):
            with pytest.raises(L.RnError) as e:
                bad()
            assert e.value.status == L.RN_ERR_INVALID and "input" in str(e.value)
        assert pu.in_flight() == 0 and pf.in_flight() == 0
        pu.submit_u8(batch_px[:5])   # and both still work
        assert np.array_equal(pu.collect(), m.forward(batch_x[:5]))
    finally:
        pu.close()
        pf.close()
        m.close()


# ---- shards ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("devices", [[0], [0, 0]], ids=["one", "twice"])
def test_shards_u8_equal_the_float_shards(devices, dtype, state50, batch_px, batch_x):
    g = R.ShardedModel(devices, "resnet50", state=state50, dtype=dtype)
    try:
        for B in (128, 37, 1):      # one call: 128 goes through the pipeline in chunks, 37 splits unevenly
            wl, wi = g.forward(batch_x[:B])
            gl, gi = g.forward_u8(batch_px[:B])
            assert np.array_equal(gl, wl) and np.array_equal(gi, wi)
        B = 48
        batches = [(0, 48), (48, 96), (80, 128)]
        g.stream_open(B, input="f32")
        want = []
        for lo, hi in batches:
            g.submit(batch_x[lo:hi])
            want.append(g.collect())
        with pytest.raises(L.RnError) as e:       # a float stream refuses bytes
            g.submit_u8(batch_px[:B])
        assert e.value.status == L.RN_ERR_INVALID and "fp32" in str(e.value)
        g.stream_close()
        g.stream_open(B, input="u8")
        with pytest.raises(L.RnError) as e:       # and a byte stream floats
            g.submit(batch_x[:B])
        assert e.value.status == L.RN_ERR_INVALID and "8-bit" in str(e.value)
        with pytest.raises(L.RnError):
            ptr = ctypes.c_void_p()
            g._check(L.lib().rn_shard_stream_buffer(g.handle, 0, ctypes.byref(ptr), None, None), "rn_shard_stream_buffer")
        got = []
        for lo, hi in batches:                    # pageable source, two in flight
            if g.in_flight() == 2:
                got.append(g.collect())
            g.submit_u8(batch_px[lo:hi])
        while g.in_flight():
            got.append(g.collect())
        for (gl, gi), (wl, wi) in zip(got, want):
            assert np.array_equal(gl, wl) and np.array_equal(gi, wi)
        for i, (lo, hi) in enumerate(batches[:2]):  # the decoder's way: bytes straight into pinned staging
            covered = 0
            for r in range(len(devices)):
                buf, slo, shi = g.stream_buffer(r)
                assert buf.dtype == np.uint8 and buf.shape == (shi - slo, 224, 224, 3)
                buf[...] = batch_px[lo + slo:lo + shi]
                covered += shi - slo
            assert covered == B
            g.submit_u8(None)
        for i in range(2):
            gl, gi = g.collect()
            assert np.array_equal(gl, want[i][0]) and np.array_equal(gi, want[i][1])
        g.stream_close()
    finally:
        g.close()


# ---- rn_infer -------------------------------------------------------------------------------------

def test_rn_infer_u8_prints_what_the_float_file_prints(state50, finch, finch_px, batch_px, batch_x, tmp_path):
    wdir = tmp_path / "weights_bin"
    R.weights.save_weights_bin(state50, str(wdir))
    exe = os.path.join(os.path.dirname(R._lib.LIB_PATH), "rn_infer")

    def lines(*args):
        r = subprocess.run([exe, "--arch", "50", "--weights", str(wdir)] + [str(a) for a in args],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return re.findall(r"max index is (\d+)", r.stdout)

    finch.tofile(tmp_path / "finch.bin")
    finch_px.tofile(tmp_path / "finch.u8")
    assert lines("--u8", tmp_path / "finch.u8") == lines("--input", tmp_path / "finch.bin") == ["112"]
    assert lines("--u8", tmp_path / "finch.u8", "--mode", "ops") == ["112"]
    batch_x[:12].tofile(tmp_path / "b12.bin")
    batch_px[:12].tofile(tmp_path / "b12.u8")
    for extra in ([], ["--dtype", "bf16"], ["--devices", "0,0,0"], ["--devices", "0,0", "--dtype", "bf16"]):
        want = lines("--input", tmp_path / "b12.bin", "--batch", 12, *extra)
        assert len(want) == 12
        assert lines("--u8", tmp_path / "b12.u8", "--batch", 12, *extra) == want
    for extra in ([], ["--devices", "0"]):          # a file of another size is refused with a message
        bad = subprocess.run([exe, "--arch", "50", "--weights", str(wdir), "--u8", str(tmp_path / "b12.u8"), "--batch",
                              "11"] + extra, capture_output=True, text=True, timeout=300)
        assert bad.returncode != 0 and "8-bit RGB" in bad.stderr and "max index" not in bad.stdout
