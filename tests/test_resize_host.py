"""The device resize's contract on the host: preprocess.resize_crop_u8 is PIL's antialiased bilinear
resize and centre crop byte for byte, and the C host code (rn_resize_crop_geometry,
rn_resize_coefficients: what the device's tables are made of) equals the Python restatement.  Every
comparison is exact equality."""
import ctypes
import os

import numpy as np
import pytest

from resnet_c_amd import _lib as L
from resnet_c_amd import preprocess as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JPEG = os.path.join(ROOT, "tests", "golden", "ILSVRC2012_val_00004749.jpeg")
SIZES = [(375, 500), (500, 375), (256, 256), (224, 224), (100, 130), (1080, 1920), (333, 257), (256, 341), (64, 48),
         (2000, 300)]
SETTINGS = [(256, 224), (232, 224), (256, 256)]


def random_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def pil_resize_crop(px, resize=256, crop=224):
    """preprocess_image_u8 from an array instead of a file."""
    Image = pytest.importorskip("PIL.Image")
    im = Image.fromarray(px)
    w, h = im.size
    if w <= h:
        nw, nh = resize, int(resize * h / w)
    else:
        nw, nh = int(resize * w / h), resize
    im = im.resize((nw, nh), Image.BILINEAR)
    left = int(round((nw - crop) / 2.0))
    top = int(round((nh - crop) / 2.0))
    return np.asarray(im.crop((left, top, left + crop, top + crop)), dtype=np.uint8)


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_crop_u8_is_pil_byte_for_byte(hw):
    px = random_image(*hw, seed=hw[0] * 7 + hw[1])
    for resize, crop in SETTINGS:
        got, want = P.resize_crop_u8(px, resize, crop), pil_resize_crop(px, resize, crop)
        assert got.shape == want.shape == (crop, crop, 3) and got.dtype == np.uint8
        assert np.array_equal(got, want), (hw, resize, crop, int((got != want).sum()))


def test_resize_crop_u8_on_the_golden_jpeg():
    pytest.importorskip("PIL")
    px = P.decode_image_u8(JPEG)
    assert px.shape == (375, 500, 3) or px.shape[2] == 3
    assert np.array_equal(P.resize_crop_u8(px), pil_resize_crop(px))
    assert np.array_equal(P.preprocess_image_u8(JPEG), P.resize_crop_u8(P.decode_image_u8(JPEG)))


def c_geometry(h, w, resize, crop):
    out = [ctypes.c_uint64() for _ in range(4)]
    st = L.lib().rn_resize_crop_geometry(h, w, resize, crop, *[ctypes.byref(o) for o in out])
    return st, tuple(o.value for o in out)


def c_coefficients(in_size, out_size, first, count):
    lib = L.lib()
    ks = ctypes.c_uint64()
    assert lib.rn_resize_coefficients(in_size, out_size, first, count, None, None, 0, ctypes.byref(ks)) in (
        L.RN_OK, L.RN_ERR_INVALID)
    bounds = np.full((count, 2), -7, dtype=np.int32)
    kk = np.full((count, ks.value), -7, dtype=np.int32)
    st = lib.rn_resize_coefficients(in_size, out_size, first, count, bounds.ctypes.data, kk.ctypes.data, kk.size,
                                    ctypes.byref(ks))
    assert st == L.RN_OK
    return bounds, kk, ks.value


def check_axis(in_size, out_size, first, count):
    wb, wk, wks = P.resize_coefficients(in_size, out_size, first, count)
    gb, gk, gks = c_coefficients(in_size, out_size, first, count)
    assert gks == wks and np.array_equal(gb, wb) and np.array_equal(gk, wk), (in_size, out_size, first, count)
    # each row sums to 2^22 within one rounding step per tap
    assert (np.abs(gk.sum(axis=1, dtype=np.int64) - (1 << 22)) <= gks).all(), (in_size, out_size)
    assert (gk >= 0).all() and (gb[:, 0] >= 0).all() and (gb[:, 0] + gb[:, 1] <= in_size).all()
    assert (gb[:, 1] >= 1).all() and (gb[:, 1] <= gks).all()


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_c_geometry_and_tables_equal_python(hw):
    h, w = hw
    for resize, crop in SETTINGS:
        nh, nw, top, left = P.resize_crop_geometry(h, w, resize, crop)
        st, got = c_geometry(h, w, resize, crop)
        assert st == L.RN_OK and got == (nh, nw, top, left)
        check_axis(w, nw, left, crop)
        check_axis(h, nh, top, crop)


def test_c_geometry_rounds_halves_to_even_and_refuses():
    seen_half = 0
    for h in range(224, 420):
        for w in (224, 256, 301, 375):
            st, got = c_geometry(h, w, 256, 224)
            assert st == L.RN_OK and got == P.resize_crop_geometry(h, w, 256, 224), (h, w)
            seen_half += (got[0] - 224) % 2
    assert seen_half > 10       # .5 cases do occur
    assert c_geometry(0, 10, 256, 224)[0] == L.RN_ERR_INVALID
    assert c_geometry(10, 0, 256, 224)[0] == L.RN_ERR_INVALID
    assert c_geometry(10, 10, 224, 256)[0] == L.RN_ERR_INVALID
    assert c_geometry(10, 10, 256, 0)[0] == L.RN_ERR_INVALID
    assert c_geometry(16385, 10, 256, 224)[0] == L.RN_ERR_INVALID


def test_c_tables_equal_python_on_a_random_sweep():
    rng = np.random.default_rng(20240607)
    for _ in range(240):
        in_size = int(rng.integers(8, 4097))
        out_size = int(rng.integers(224, 513))
        count = int(rng.integers(1, min(out_size, 224) + 1))
        first = int(rng.integers(0, out_size - count + 1))
        check_axis(in_size, out_size, first, count)
    for in_size, out_size in ((8, 512), (4096, 224), (224, 224), (225, 224), (4096, 512)):
        check_axis(in_size, out_size, 0, out_size)


def test_c_coefficients_refuse_bad_arguments():
    lib = L.lib()
    ks = ctypes.c_uint64()
    b, k = np.zeros((4, 2), np.int32), np.zeros((4, 16), np.int32)
    args = (b.ctypes.data, k.ctypes.data, k.size, ctypes.byref(ks))
    assert lib.rn_resize_coefficients(500, 256, 0, 4, *args) == L.RN_OK and ks.value == 5
    assert lib.rn_resize_coefficients(0, 256, 0, 4, *args) == L.RN_ERR_INVALID
    assert lib.rn_resize_coefficients(500, 0, 0, 4, *args) == L.RN_ERR_INVALID
    assert lib.rn_resize_coefficients(500, 256, 253, 4, *args) == L.RN_ERR_INVALID     # past the last output
    assert lib.rn_resize_coefficients(500, 256, 0, 4, b.ctypes.data, k.ctypes.data, 19, ctypes.byref(ks)) == L.RN_ERR_INVALID


def test_table_of_a_batch_is_pure_host_code_and_shares_sizes():
    lib = L.lib()
    u64p = ctypes.POINTER(ctypes.c_uint64)
    hs = np.array([375, 500, 375, 64], dtype=np.uint64)
    ws = np.array([500, 375, 500, 48], dtype=np.uint64)
    offs = np.array([0, 562500, 1125000, 1687500], dtype=np.uint64)
    n = ctypes.c_uint64()
    a = (offs.ctypes.data_as(u64p), hs.ctypes.data_as(u64p), ws.ctypes.data_as(u64p))
    assert lib.rn_image_u8_resize_crop_table(*a, 4, 256, 224, None, 0, ctypes.byref(n)) == L.RN_OK
    tab = np.zeros(n.value // 4, dtype=np.uint32)
    assert lib.rn_image_u8_resize_crop_table(*a, 4, 256, 224, tab.ctypes.data, tab.nbytes, ctypes.byref(n)) == L.RN_OK
    d = tab[:48].reshape(4, 12)
    assert np.array_equal(d[0, 4:10], d[2, 4:10]) and not np.array_equal(d[0, 4:10], d[1, 4:10])
    assert list(d[:, 0]) == list(offs) and list(d[:, 10]) == [1500, 1125, 1500, 144]
    # image 0's horizontal table inside the batch table is the one rn_resize_coefficients gives
    nh, nw, top, left = P.resize_crop_geometry(375, 500)
    wb, wk, ks = P.resize_coefficients(500, nw, left, 224)
    assert d[0, 6] == ks
    assert np.array_equal(tab[d[0, 4]:d[0, 4] + 448].view(np.int32).reshape(224, 2), wb)
    assert np.array_equal(tab[d[0, 5]:d[0, 5] + 224 * ks].view(np.int32).reshape(224, ks), wk)
    assert lib.rn_image_u8_resize_crop_table(*a, 4, 256, 224, tab.ctypes.data, tab.nbytes - 4, ctypes.byref(n)) == L.RN_ERR_INVALID
    hs[3] = 0
    assert lib.rn_image_u8_resize_crop_table(*a, 4, 256, 224, None, 0, ctypes.byref(n)) == L.RN_ERR_INVALID
