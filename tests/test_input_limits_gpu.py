"""The byte route's two input launches AT the limits include/rn_hip.h states, on the GPU: the inputs
test_input_limits_host.py built and vetted, each through ONE call on views between guard bands (the output starts as
0xA5 bytes, so an element the launch never wrote shows), launch counts asserted, against the numpy contract with
np.array_equal and nothing else.  The host file pins contract == PIL == C tables on the same cases and asserts, per
case, the path it reaches; this file needs device == contract only.  profiles/input_limits/README.md maps the cases
to the paths."""
import ctypes

import numpy as np
import pytest

import views as V
import resnet_c_amd as R
import test_input_limits_host as H
from resnet_c_amd import _lib as L
from resnet_c_amd import preprocess as P
from resnet_c_amd.tensor import _DeviceBuffer

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)


def launches():
    return int(L.lib().rn_ctx_launch_count(R.get_ctx().handle))


def u64(v):
    return np.ascontiguousarray(v, dtype=np.uint64)


def resize_on_views(packed, offsets, heights, widths, resize, crop, src_off=0, dst_off=0):
    """one rn_image_u8_resize_crop call: the packed images at `src_off` between NaN-byte guards, the output at
    `dst_off` in a buffer of 0xA5 bytes; both guards checked; -> [B, crop, crop, 3]"""
    offsets, heights, widths = u64(offsets), u64(heights), u64(widths)
    B = len(offsets)
    what = f"rn_image_u8_resize_crop B={B} ({resize}, {crop}) src+{src_off} dst+{dst_off}"
    vi = V.place(packed, src_off)
    vo = V.place_out(B * crop * crop * 3, dst_off)
    n0 = launches()
    V.must("rn_image_u8_resize_crop", vi.ptr, offsets.ctypes.data_as(U64P), heights.ctypes.data_as(U64P),
           widths.ctypes.data_as(U64P), B, vo.ptr, resize, crop)
    assert launches() - n0 == 1, "one counted call, however many pieces of 65535 images it is cut into"
    V.check_guards(what, vi)
    return V.fetch(vo, np.uint8, what).reshape(B, crop, crop, 3)


def differing(got, want):
    return f"{int((got != want).sum())} of {want.size} bytes differ, the first at {np.argwhere(got != want)[:4].tolist()}"


# =====================================================================================================================
# A. rn_image_u8_resize_crop
# =====================================================================================================================
@pytest.mark.parametrize("name", list(H.RESIZE_CASES))
def test_resize_crop_at_its_limits(name):
    h, w, resize, crop = H.RESIZE_CASES[name]
    px, want = H.resize_image(name), H.resize_want(name)
    i = list(H.RESIZE_CASES).index(name)
    got = resize_on_views(px.reshape(-1), [0], [h], [w], resize, crop, src_off=i % 4, dst_off=(3 * i + 1) % 4)
    assert np.array_equal(got[0], want), f"{name}: {differing(got[0], want)}"
    ncol, rows, rows_cap, step_r, step_x, lds = H.launch_form(crop)
    H.record(f"input limits resize {name} {h} x {w} ({resize}, {crop}): resize_crop_kernel<{ncol}> bands of {rows}, rows_cap "
             f"{rows_cap} ({lds} bytes of LDS), walk ({step_r}, {step_x}); {want.size} bytes equal, {len(np.unique(want))} values")


def test_resize_crop_second_launch():
    """B = 65537: images 65535 and 65536 go through a second launch with b_base = 65535"""
    packed, offsets, heights, widths, want = H.batch_case()
    got = resize_on_views(packed, offsets, heights, widths, *H.BATCH_SETTING)
    wrong = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    assert wrong.size == 0, f"{wrong.size} images differ, the first {wrong[:8].tolist()}"
    H.record(f"input limits resize B = {len(want)}: two launches, every image the bytes of its period's image")


def test_resize_crop_behind_4_gib():
    """Image 1 lies at byte 2^32 + 3 of the source buffer: the descriptor's high offset word.  The 4 GiB buffer comes
    straight from rn_malloc and only its head (image 0 at offset 1) and image 1 are uploaded: guard bands around a
    source of that size are not possible, the output keeps them."""
    ctx, lib = R.get_ctx(), L.lib()
    imgs, low, want = H.offset_case()
    src = _DeviceBuffer(ctx, H.OFFSET_BYTES)
    one = np.ascontiguousarray(imgs[1]).reshape(-1)
    L.check(lib.rn_memcpy_h2d(ctx.handle, src.ptr, low.ctypes.data, low.size), "h2d", ctx.handle)
    L.check(lib.rn_memcpy_h2d(ctx.handle, src.ptr + H.OFFSET_AT[1], one.ctypes.data, one.size), "h2d", ctx.handle)
    resize, crop = H.OFFSET_SETTING
    vo = V.place_out(2 * crop * crop * 3, 1)
    n0 = launches()
    V.must("rn_image_u8_resize_crop", src.ptr, u64(H.OFFSET_AT).ctypes.data_as(U64P), u64([33, 33]).ctypes.data_as(U64P),
           u64([35, 35]).ctypes.data_as(U64P), 2, vo.ptr, resize, crop)
    assert launches() - n0 == 1
    got = V.fetch(vo, np.uint8, "rn_image_u8_resize_crop behind 4 GiB").reshape(2, crop, crop, 3)
    assert np.array_equal(got[0], want[0]), differing(got[0], want[0])
    assert np.array_equal(got[1], want[1]), differing(got[1], want[1])
    H.record("input limits resize offset 2^32 + 3: both crops equal")


def test_resize_crop_refuses_scale_65_and_launches_nothing():
    ctx, lib = R.get_ctx(), L.lib()
    src = _DeviceBuffer(ctx, 64)
    view = V.place_out(64 * 64 * 3)
    n0 = launches()
    for h, w, resize, crop in H.REFUSED:
        st = lib.rn_image_u8_resize_crop(ctx.handle, src.ptr, u64([0]).ctypes.data_as(U64P), u64([h]).ctypes.data_as(U64P),
                                         u64([w]).ctypes.data_as(U64P), 1, view.ptr, resize, crop)
        assert st == L.RN_ERR_INVALID, (h, w, resize, crop, st)
    assert launches() == n0
    ctx.sync()
    V.assert_untouched(view, "refused calls")


# =====================================================================================================================
# B. rn_image_u8_to_nhwc_pad_dt
# =====================================================================================================================
@pytest.mark.parametrize("name,bf16,cpad", H.norm_params())
def test_normaliser_at_its_limits(name, bf16, cpad):
    """The expected tensor is numpy alone (H.norm_want), on purpose: not rn_nchw_to_nhwc_pad_dt, the device kernel
    test_image_u8_gpu.py compares with."""
    B, Hh, W, border = H.NORM_CASES[name]
    px, want = H.norm_pixels(name), H.norm_want(name, bf16, cpad)
    what = f"rn_image_u8_to_nhwc_pad_dt {name} {'bf16' if bf16 else 'f32'} Cpad {cpad}"
    vi, vo = V.place(px), V.place_out(want.nbytes)
    kernel = H.target(bf16, B, Hh, W, cpad, border, vi.ptr, vo.ptr)
    assert kernel == ("element" if (name, (bf16, cpad)) in H.NORM_ELEMENT else "x16"), "with these pointers"
    m3, s3 = (ctypes.c_float * 3)(*P.MEAN), (ctypes.c_float * 3)(*P.STD)
    n0 = launches()
    V.must("rn_image_u8_to_nhwc_pad_dt", L.RN_DTYPE_BF16 if bf16 else L.RN_DTYPE_F32, vi.ptr, vo.ptr, B, Hh, W, cpad, border, m3, s3)
    assert launches() - n0 == 1
    V.check_guards(what, vi)
    got = V.fetch(vo, want.dtype, what).reshape(want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} elements differ, the first at (b, hp, wp, c) {bad[:4].tolist()}")
    n16, steps, _ = H.x16_form(bf16, B, Hh, W, cpad, border)
    H.record(f"input limits normaliser {name} {B} x {Hh} x {W} border {border} {'bf16' if bf16 else 'f32'} Cpad {cpad}: {kernel}"
             + (f", {n16} stores an image, steps {steps}, divisor {W + 2 * border}" if kernel == "x16" else "") + f"; {want.size} elements equal")
