"""The byte route's two input launches AT the limits include/rn_hip.h states, on the host: every input
test_input_limits_gpu.py runs is built here -- each generator, seed and shape in one place, cached, so the GPU file
runs what this file vetted -- and the numpy contract alone is run on it (preprocess.resize_crop_u8 for
rn_image_u8_resize_crop, preprocess.normalize_u8 padded in numpy for rn_image_u8_to_nhwc_pad_dt).  What is asserted
are the CONDITIONS: properties of the tables and of the reference that prove the input reaches the path its case
exists for (the kernel instantiation, the pixel walk's form, the LDS rounds, the second launch, the high offset word,
the 16-byte form and its divisor).  The launch rules of rn_resize.hip and rn_image.hip are restated here
(`launch_form`, `target`, `magic_div`).  Beside that: the C tables equal the Python restatement and the restatement
equals PIL on the axes and images of every case, so that the GPU file needs device == contract only.  No GPU.
profiles/input_limits/README.md lists which case is there for which path."""
import ctypes
import functools
import os

import numpy as np
import pytest

from resnet_c_amd import _lib as L
from resnet_c_amd import ops
from resnet_c_amd import preprocess as P

GRID_Y = 65535            # both launches cut a batch into launches of this many images (gridDim.y)
ACC = 24                  # RN_RS_ACC: accumulators a thread of the resize keeps
U64P = ctypes.POINTER(ctypes.c_uint64)


def cached(fn):
    """one computation per argument tuple for both files; the arrays are shared and never written to"""
    return functools.lru_cache(maxsize=None)(fn)


def record(line):
    """print a line and, where RN_INPUT_LIMITS_FILE names a file, append it there: that is how
    profiles/input_limits/results.txt is written"""
    print(line)
    path = os.environ.get("RN_INPUT_LIMITS_FILE")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


# =====================================================================================================================
# images
# =====================================================================================================================
BLOCK = (37, 53)          # primes: co-prime with every scale used here (powers of two, 65/64, 175/64, ...)


@cached
def structured_image(h, w, seed):
    """Flat blocks of 37 x 53 pixels of random colour, a diagonal ramp (7y + 13x) % 256 added to the green channel,
    30 % of the pixels replaced by noise.  Reduced 64 times, plain noise is a nearly constant grey on which a dropped
    or misplaced tap moves few bytes; the blocks and the ramp keep structure at every scale."""
    rng = np.random.default_rng(seed)
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    blocks = rng.integers(0, 256, size=(-(-h // BLOCK[0]), -(-w // BLOCK[1]), 3), dtype=np.uint8)
    img = blocks[y // BLOCK[0], x // BLOCK[1]]
    img[..., 1] += ((7 * y + 13 * x) % 256).astype(np.uint8)
    noisy = rng.random((h, w)) < 0.3
    img[noisy] = rng.integers(0, 256, size=(int(noisy.sum()), 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


# =====================================================================================================================
# A. rn_image_u8_resize_crop
# =====================================================================================================================
def launch_form(crop):
    """rn_image_u8_resize_crop_launch and launch<NCOL> restated: (NCOL, R, rows_cap, step_r, step_x, LDS bytes)"""
    need = -(-3 * crop // 256)
    ncol = next(n for n in (1, 2, 3, 4, 6, 8, 12, 24) if need <= n)
    rows_cap = min(65536 // (3 * crop), 32)
    step_r = 256 // crop
    return ncol, ACC // ncol, rows_cap, step_r, 256 - step_r * crop, rows_cap * 3 * crop


# name -> (H, W, resize, crop): one image per call
RESIZE_CASES = {
    "ncol2_reduce": (300, 200, 110, 100),
    "ncol2_enlarge": (97, 211, 110, 100),
    "ncol8_last_band_of_one": (700, 650, 640, 601),
    "ncol24_first_crop": (1100, 1300, 1040, 1025),
    "ncol12_last_crop": (1100, 1300, 1040, 1024),
    "crop_2048": (2100, 2300, 2048, 2048),
    "resize_16384": (2, 2, 16384, 2048),
    "long_side_131072": (6400, 100, 2048, 2048),
    "height_16384": (16384, 48, 48, 48),
    "width_16384": (48, 16384, 48, 48),
    "crop_1": (64, 64, 1, 1),
    "scale_64_both_axes": (512, 512, 8, 8),
    "scale_64_full_band": (4160, 4096, 64, 64),
}
SCALE_64 = ("scale_64_both_axes", "scale_64_full_band")       # the two with more than one output
REFUSED = ((2048, 2080, 32, 32), (4161, 4096, 64, 64))        # scale 65 on the horizontal / the vertical axis


@cached
def resize_image(name):
    h, w, _, _ = RESIZE_CASES[name]
    return structured_image(h, w, 1000 + sorted(RESIZE_CASES).index(name))


@cached
def resize_tables(name):
    """(nh, nw, top, left), (hb, hk, hks), (vb, vk, vks) of the Python restatement"""
    h, w, resize, crop = RESIZE_CASES[name]
    nh, nw, top, left = P.resize_crop_geometry(h, w, resize, crop)
    return (nh, nw, top, left), P.resize_coefficients(w, nw, left, crop), P.resize_coefficients(h, nh, top, crop)


@cached
def resize_want(name):
    _, _, resize, crop = RESIZE_CASES[name]
    want = P.resize_crop_u8(resize_image(name), resize, crop)
    want.setflags(write=False)
    return want


def band(vb, crop, R, index):
    """(r_lo, r_hi) of the kernel's band `index`: the source rows its R output rows read"""
    y0 = index * R
    last = min(y0 + R, crop) - 1
    return int(vb[y0, 0]), int(vb[last, 0] + vb[last, 1])


def test_the_launch_rule_restated():
    """every crop takes the smallest instantiation that holds its row, LDS stays within 64 KB, the walk's steps add up"""
    seen = {}
    for crop in range(1, 2049):
        ncol, R, rows_cap, step_r, step_x, lds = launch_form(crop)
        assert 256 * ncol >= 3 * crop and ncol * R == ACC and 1 <= rows_cap <= 32 and lds <= 65536
        assert step_r * crop + step_x == 256 and step_x < crop
        seen.setdefault(ncol, []).append(crop)
    assert {n: (c[0], c[-1]) for n, c in seen.items()} == {1: (1, 85), 2: (86, 170), 3: (171, 256), 4: (257, 341), 6: (342, 512),
                                                          8: (513, 682), 12: (683, 1024), 24: (1025, 2048)}


def test_the_pixel_walk_visits_every_pixel_once():
    """The horizontal pass's walk (rr, x) += (step_r, step_x) with the wrap, simulated for the crops of the cases and
    the forms between them, at nr = 1, rows_cap - 1 and rows_cap: every (row, column) exactly once."""
    crops = sorted({c[3] for c in RESIZE_CASES.values()} | {3, 85, 86, 127, 128, 129, 255, 256, 257})
    for crop in crops:
        _, _, rows_cap, step_r, step_x, _ = launch_form(crop)
        for nr in {1, max(rows_cap - 1, 1), rows_cap}:
            tid = np.arange(256)
            rr, x = tid // crop, tid % crop
            hits = np.zeros((nr, crop), np.int32)
            while (rr < nr).any():
                live = rr < nr
                np.add.at(hits, (rr[live], x[live]), 1)
                rr, x = rr + step_r, x + step_x
                wrap = x >= crop
                x, rr = np.where(wrap, x - crop, x), rr + wrap
            assert (hits == 1).all(), (crop, nr)


def test_ncol2_cases_take_the_two_row_walk():
    for name in ("ncol2_reduce", "ncol2_enlarge"):
        h, w, resize, crop = RESIZE_CASES[name]
        ncol, R, rows_cap, step_r, step_x, _ = launch_form(crop)
        assert -(-3 * crop // 256) == 2 and ncol == 2 and R == 12
        assert 256 // crop == 2 and step_r == 2 and step_x == 56 and rows_cap == 32
    assert resize_tables("ncol2_reduce")[1][2] > 3 and resize_tables("ncol2_reduce")[2][2] > 3      # a reduction: ksize > 3
    assert resize_tables("ncol2_enlarge")[2][2] == 3                                                # an enlargement (vertical)
    assert 97 < 110 and resize_tables("ncol2_enlarge")[0][0] == 110


def test_ncol8_case_ends_in_a_band_of_one_row():
    h, w, resize, crop = RESIZE_CASES["ncol8_last_band_of_one"]
    ncol, R, rows_cap, _, _, _ = launch_form(crop)
    assert (ncol, R) == (8, 3) and crop % 3 == 1 and crop == 200 * 3 + 1 and -(-crop // R) == 201
    assert rows_cap == 32 and 256 // crop == 0


def test_crops_1024_and_1025_sit_on_both_sides_of_the_last_threshold():
    assert -(-3075 // 256) == 13 and launch_form(1025)[:3] == (24, 1, 21)
    assert -(-3072 // 256) == 12 and launch_form(1024)[:3] == (12, 2, 21)
    assert RESIZE_CASES["ncol24_first_crop"][3] == 1025 and RESIZE_CASES["ncol12_last_crop"][3] == 1024
    # column 12 of the accumulators holds bytes 3072..3074 of a row: threads 0..2 only
    assert [t for t in range(256) if t + 256 * 12 < 3075] == [0, 1, 2]


def test_crop_2048_fills_every_accumulator_and_the_lds():
    h, w, resize, crop = RESIZE_CASES["crop_2048"]
    ncol, R, rows_cap, _, _, lds = launch_form(crop)
    assert 65536 // 6144 == 10 and (ncol, R, rows_cap, lds) == (24, 1, 10, 61440)
    assert all(tid + 256 * 23 < 6144 for tid in range(256)), "the last column of accumulators is live for every thread"
    assert -(-crop // R) == 2048, "2048 bands"
    (nh, nw, _, _), _, (vb, _, _) = resize_tables("crop_2048")
    assert min(nh, nw) == 2048


def test_resize_16384_is_an_enlargement_of_8192_times():
    (nh, nw, top, left), (hb, _, hks), (vb, _, vks) = resize_tables("resize_16384")
    assert nh == nw == 16384 and top == left == 7168 and hks == vks == 3
    for b in (hb, vb):
        assert b[:, 1].min() >= 1 and b[:, 1].max() <= 3 and set(b[:, 0]) <= {0, 1}
    (_, hk, _), (_, vk, _) = resize_tables("resize_16384")[1:]
    assert len(np.unique(hk[:, 0])) > 1000 and len(np.unique(vk[:, 0])) > 1000, "the weights move along the crop"


def test_long_side_of_131072_is_not_refused():
    (nh, nw, top, left), _, (vb, _, _) = resize_tables("long_side_131072")
    assert (nh, nw, top, left) == (131072, 2048, 64512, 0)
    assert vb[:, 0].max() >= 3149 and vb[0, 0] >= 3149
    st, got = c_geometry(*RESIZE_CASES["long_side_131072"])
    assert st == L.RN_OK and got == (nh, nw, top, left)


def test_sides_of_16384_crop_from_the_middle():
    (nh, nw, top, left), (hb, _, _), (vb, _, _) = resize_tables("height_16384")
    assert (nh, nw, top, left) == (16384, 48, 8168, 0) and vb[0, 0] >= 8167
    (nh2, nw2, top2, left2), (hb2, _, _), (vb2, _, _) = resize_tables("width_16384")
    assert (nh2, nw2, top2, left2) == (48, 16384, 0, 8168) and hb2[0, 0] >= 8167
    # the largest first-tap row and column of the file (the byte offset row * stride is larger at 4160 x 4096, whose
    # rows are 12288 bytes long: 50 MB, still far inside 32 bits; 16384 rows of 49152 bytes are out of scope)
    rows = {n: int(resize_tables(n)[2][0][:, 0].max()) for n in RESIZE_CASES}
    cols = {n: int(resize_tables(n)[1][0][:, 0].max()) for n in RESIZE_CASES}
    assert max(rows, key=rows.get) == "height_16384" and max(cols, key=cols.get) == "width_16384"


def test_crop_1_is_one_pixel_from_a_row_clipped_at_both_ends():
    (nh, nw, top, left), (hb, _, hks), (vb, _, vks) = resize_tables("crop_1")
    assert launch_form(1)[3:5] == (256, 0) and resize_want("crop_1").shape == (1, 1, 3)
    assert hks == vks == 129 and (nh, nw) == (1, 1)
    for b in (hb, vb):
        assert b.shape == (1, 2) and b[0, 0] == 0 and b[0, 0] + b[0, 1] == 64


def test_scale_64_rows_have_128_taps_in_rows_of_129():
    for name in SCALE_64:
        h, w, resize, crop = RESIZE_CASES[name]
        (nh, nw, top, left), (hb, hk, hks), (vb, vk, vks) = resize_tables(name)
        assert h == 64 * nh and w == 64 * nw, "one row or column more would be refused"
        assert hks == vks == 129
        for b in (hb, vb):
            # at scale exactly 64 every centre is a whole number, so a whole row is 128 taps in a row of ksize 129
            # ints; 129 live taps need a fractional centre at scale 64, which no size pair has
            # (the crop of 64 of 65 rows starts at row 0: its last row is whole)
            assert b[:, 1].max() == 128 and b[0, 1] < 128 and (b[:, 1] == 128).sum() >= len(b) - 2, "the first row clipped, interior rows whole"
    (nh, nw, _, _), _, (vb, _, _) = resize_tables("scale_64_full_band")
    assert (nh, nw) == (65, 64)
    ncol, R, rows_cap, _, _, _ = launch_form(64)
    # 24 rows at scale 64 span 23 * 64 + 128 = 1600 source rows, 50 rounds of 32; band 0 is clipped at the top (1568
    # rows, 49 rounds), band 1 is whole, band 2 has 16 rows (34 rounds)
    spans = [band(vb, 64, R, i) for i in range(3)]
    assert (ncol, R, rows_cap) == (1, 24, 32) and -(-64 // R) == 3
    assert [hi - lo for lo, hi in spans] == [1568, 1600, 1088] and [-(-(hi - lo) // 32) for lo, hi in spans] == [49, 50, 34]


def crop_with(name, hmod=None, vmod=None):
    """resize_crop_u8 of the case's image with changed coefficient rows: what wrong device code would compute"""
    (_, _, _, _), (hb, hk, _), (vb, vk, _) = resize_tables(name)
    hk, vk = (hmod(hb, hk) if hmod else hk), (vmod(vb, vk) if vmod else vk)
    px = resize_image(name)
    r0, r1 = int(vb[0, 0]), int(vb[-1, 0] + vb[-1, 1])
    hor = P._resample_axis0(np.ascontiguousarray(px[r0:r1].transpose(1, 0, 2)), hb, hk).transpose(1, 0, 2)
    shifted = vb.copy()
    shifted[:, 0] -= r0
    return P._resample_axis0(np.ascontiguousarray(hor), shifted, vk)


def taps_from_64_zeroed(b, k):
    k = k.copy()
    k[:, 64:] = 0
    return k


def last_tap_zeroed(b, k):
    k = k.copy()
    k[np.arange(len(k)), b[:, 1] - 1] = 0
    return k


@pytest.mark.parametrize("name", SCALE_64)
def test_scale_64_reference_tells_dropped_taps(name):
    """The reference must tell wrong code from right code: half of the taps dropped changes more than half of the
    bytes, the last tap alone at least one, on each axis (counts on the reference alone)."""
    want = resize_want(name)
    assert np.array_equal(crop_with(name), want)
    shares = {}
    for key, kw in (("h64", {"hmod": taps_from_64_zeroed}), ("v64", {"vmod": taps_from_64_zeroed}),
                    ("hlast", {"hmod": last_tap_zeroed}), ("vlast", {"vmod": last_tap_zeroed})):
        shares[key] = float((crop_with(name, **kw) != want).mean())
    record(f"input limits {name}: bytes changed by taps 64.. zeroed {shares['h64']:.3f} (horizontal) {shares['v64']:.3f} "
           f"(vertical), by the last tap zeroed {shares['hlast']:.4f} {shares['vlast']:.4f}")
    assert shares["h64"] > 0.5 and shares["v64"] > 0.5 and shares["hlast"] > 0 and shares["vlast"] > 0, shares


def test_reduced_outputs_are_not_grey():
    for name, (h, w, resize, crop) in RESIZE_CASES.items():
        n = len(np.unique(resize_want(name)))
        nh, nw, _, _ = resize_tables(name)[0]
        reduced = h > nh or w > nw          # (an enlargement of 2 x 2 pixels has the values between four colours: 30)
        assert n >= (3 if crop == 1 else 60 if reduced else 24), (name, n)


# ---- contract == C tables == PIL on the cases ------------------------------------------------------------------------
def c_geometry(h, w, resize, crop):
    out = [ctypes.c_uint64() for _ in range(4)]
    st = L.lib().rn_resize_crop_geometry(h, w, resize, crop, *[ctypes.byref(o) for o in out])
    return st, tuple(o.value for o in out)


def c_coefficients(in_size, out_size, first, count):
    lib = L.lib()
    ks = ctypes.c_uint64()
    lib.rn_resize_coefficients(in_size, out_size, first, count, None, None, 0, ctypes.byref(ks))
    bounds = np.full((count, 2), -7, dtype=np.int32)
    kk = np.full((count, ks.value), -7, dtype=np.int32)
    st = lib.rn_resize_coefficients(in_size, out_size, first, count, bounds.ctypes.data, kk.ctypes.data, kk.size, ctypes.byref(ks))
    assert st == L.RN_OK, (in_size, out_size, first, count)
    return bounds, kk, ks.value


def c_table(offsets, heights, widths, resize, crop):
    """(status, the table as uint32 words) of rn_image_u8_resize_crop_table"""
    lib = L.lib()
    a = [np.ascontiguousarray(v, dtype=np.uint64) for v in (offsets, heights, widths)]
    p = [v.ctypes.data_as(U64P) for v in a]
    n = ctypes.c_uint64()
    st = lib.rn_image_u8_resize_crop_table(*p, len(a[0]), resize, crop, None, 0, ctypes.byref(n))
    if st != L.RN_OK:
        return st, None
    tab = np.zeros(n.value // 4, dtype=np.uint32)
    st = lib.rn_image_u8_resize_crop_table(*p, len(a[0]), resize, crop, tab.ctypes.data, tab.nbytes, ctypes.byref(n))
    return st, tab


def axis_of_table(tab, d, which, crop):
    """(bounds, coefficients, ksize) of descriptor d's horizontal (0) or vertical (1) axis"""
    bi, ki, ks = (int(v) for v in d[4 + 3 * which:7 + 3 * which])
    return (tab[bi:bi + 2 * crop].view(np.int32).reshape(crop, 2), tab[ki:ki + crop * ks].view(np.int32).reshape(crop, ks), ks)


def same_axis(got, want):
    return got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name", sorted(RESIZE_CASES))
def test_c_tables_equal_python_on_the_cases(name):
    h, w, resize, crop = RESIZE_CASES[name]
    (nh, nw, top, left), hor, ver = resize_tables(name)
    st, got = c_geometry(h, w, resize, crop)
    assert st == L.RN_OK and got == (nh, nw, top, left)
    st, tab = c_table([5], [h], [w], resize, crop)
    assert st == L.RN_OK
    d = tab[:12]
    assert (d[0], d[1], d[2], d[3], d[10]) == (5, 0, h, w, 3 * w)
    assert same_axis(axis_of_table(tab, d, 0, crop), hor) and same_axis(axis_of_table(tab, d, 1, crop), ver)
    assert tab.size == 12 + crop * (4 + hor[2] + ver[2])
    for in_size, out_size, first, want in ((w, nw, left, hor), (h, nh, top, ver)):
        if out_size <= 16384:       # rn_resize_coefficients takes sizes up to 16384; the table has no such limit
            assert same_axis(c_coefficients(in_size, out_size, first, crop), want)
        else:
            ks = ctypes.c_uint64()
            assert L.lib().rn_resize_coefficients(in_size, out_size, first, crop, None, None, 0, ctypes.byref(ks)) == L.RN_ERR_INVALID


def test_c_tables_equal_python_on_a_sweep_up_to_the_limits():
    rng = np.random.default_rng(20240917)
    widest = 0.0
    for i in range(160):
        out_size = int(rng.integers(1, 2049)) if i % 4 else int(rng.integers(1, 65))
        top = min(16384, 64 * out_size)
        in_size = int(rng.integers(max(top // 2, 1), top + 1)) if i % 3 == 0 else int(rng.integers(1, top + 1))
        count = int(rng.integers(1, min(out_size, 64) + 1))
        first = int(rng.integers(0, out_size - count + 1))
        want = P.resize_coefficients(in_size, out_size, first, count)
        got = c_coefficients(in_size, out_size, first, count)
        assert same_axis(got, want), (in_size, out_size, first, count)
        assert (np.abs(got[1].sum(axis=1, dtype=np.int64) - (1 << 22)) <= got[2]).all() and (got[1] >= 0).all()
        assert (got[0][:, 0] >= 0).all() and (got[0][:, 0] + got[0][:, 1] <= in_size).all() and (got[0][:, 1] >= 1).all()
        widest = max(widest, in_size / out_size)
    assert widest > 48, widest
    for in_size, out_size in ((16384, 256), (64, 1), (128, 2), (16384, 2048), (1, 2048), (2, 16384)):
        assert same_axis(c_coefficients(in_size, out_size, 0, min(out_size, 2048)), P.resize_coefficients(in_size, out_size, 0, min(out_size, 2048)))


def pil_resize_crop(px, resize, crop):
    Image = pytest.importorskip("PIL.Image")
    im = Image.fromarray(px)
    w, h = im.size
    if w <= h:
        nw, nh = resize, int(resize * h / w)
    else:
        nw, nh = int(resize * w / h), resize
    left, top = int(round((nw - crop) / 2.0)), int(round((nh - crop) / 2.0))
    im = im.resize((nw, nh), Image.BILINEAR)
    return np.asarray(im.crop((left, top, left + crop, top + crop)), dtype=np.uint8)


@pytest.mark.parametrize("name", sorted(RESIZE_CASES))
def test_resize_crop_u8_is_pil_on_the_cases(name):
    _, _, resize, crop = RESIZE_CASES[name]
    got, want = resize_want(name), pil_resize_crop(resize_image(name), resize, crop)
    assert got.shape == want.shape == (crop, crop, 3) and np.array_equal(got, want), (name, int((got != want).sum()))


def test_scale_65_is_refused_on_the_host():
    for h, w, resize, crop in REFUSED:
        st, (nh, nw, _, _) = c_geometry(h, w, resize, crop)
        assert st == L.RN_OK and (h > 64 * nh or w > 64 * nw)
        assert c_table([0], [h], [w], resize, crop)[0] == L.RN_ERR_INVALID
    assert c_table([0], [2048], [2048], 32, 32)[0] == L.RN_OK and c_table([0], [4160], [4096], 64, 64)[0] == L.RN_OK


# ---- the batch case: B = 65537 ---------------------------------------------------------------------------------------
BATCH_B = GRID_Y + 2
BATCH_SIZES = [(3, 5), (4, 4), (5, 3), (7, 9), (9, 4), (4, 11), (6, 6), (8, 5)]
BATCH_SETTING = (4, 3)
BATCH_PERIOD = 8 * 64


@cached
def batch_case():
    """65537 images: image i has size BATCH_SIZES[i % 8] and the content of image i % 512; each sits at its own odd
    offset.  One period of 512 images is packed with every image on an odd offset and an even length, and tiled;
    the expected output is the period's 512 crops, tiled.  -> (packed, offsets, heights, widths, want)"""
    resize, crop = BATCH_SETTING
    imgs = [structured_image(*BATCH_SIZES[i % 8], seed=7000 + i) for i in range(BATCH_PERIOD)]
    rel, at = [], 1
    for a in imgs:
        rel.append(at)
        at += a.size
        at += 1 - at % 2                     # the next odd offset
    plen = at + 1                            # even: a period later the offsets are odd again
    period = np.full(plen, 0xEE, dtype=np.uint8)
    for o, a in zip(rel, imgs):
        period[o:o + a.size] = a.reshape(-1)
    reps = -(-BATCH_B // BATCH_PERIOD)
    packed = np.tile(period, reps)
    i = np.arange(BATCH_B)
    offsets = (np.asarray(rel, np.uint64)[i % BATCH_PERIOD] + (i // BATCH_PERIOD).astype(np.uint64) * np.uint64(plen)).astype(np.uint64)
    sizes = np.asarray(BATCH_SIZES, np.uint64)[i % 8]
    crops = np.stack([P.resize_crop_u8(a, resize, crop) for a in imgs])
    want = crops[i % BATCH_PERIOD]
    for a in (packed, offsets, want):
        a.setflags(write=False)
    return packed, offsets, np.ascontiguousarray(sizes[:, 0]), np.ascontiguousarray(sizes[:, 1]), want


def test_batch_case_puts_other_images_into_the_second_launch():
    packed, offsets, heights, widths, want = batch_case()
    resize, crop = BATCH_SETTING
    assert BATCH_B == 65537 and len(offsets) == BATCH_B and want.shape == (BATCH_B, crop, crop, 3)
    assert (offsets % 2 == 1).all() and len(np.unique(offsets)) == BATCH_B
    assert int(offsets[-1] + heights[-1] * widths[-1] * 3) <= packed.size < 1 << 31
    # the tiling is periodic: the bytes of EVERY image are the bytes of image i % 512, and of the size of i % 8
    i = np.arange(BATCH_B)
    for s, (h, w) in enumerate(BATCH_SIZES):
        idx = i[i % 8 == s]
        assert (heights[idx] == h).all() and (widths[idx] == w).all()
        got = packed[offsets[idx][:, None].astype(np.int64) + np.arange(h * w * 3)[None, :]]
        first = got[:BATCH_PERIOD // 8]
        assert np.array_equal(got, first[(idx // 8) % (BATCH_PERIOD // 8)])
        for j in (0, 17, 63):
            assert np.array_equal(first[j].reshape(h, w, 3), structured_image(h, w, seed=7000 + 8 * j + s))
        assert len({first[j].tobytes() for j in range(64)}) == 64, "64 contents per size"
    # what the second launch must read: images 65535 and 65536, not blockIdx.y = 0 and 1
    for late, early in ((GRID_Y, 0), (GRID_Y + 1, 1)):
        assert (heights[late], widths[late]) != (heights[early], widths[early])
        assert not np.array_equal(want[late], want[early])
    assert not np.array_equal(want[GRID_Y], want[GRID_Y + 1])
    # a few images against the contract, straight from the packed bytes
    for b in (0, 1, 511, 512, 4099, GRID_Y - 1, GRID_Y, GRID_Y + 1):
        h, w = int(heights[b]), int(widths[b])
        px = packed[int(offsets[b]):int(offsets[b]) + h * w * 3].reshape(h, w, 3)
        assert np.array_equal(P.resize_crop_u8(px, resize, crop), want[b]), b
    assert launch_form(crop)[:2] == (1, 24), "one block per image: grid (1, 65535) then (1, 2)"


def test_batch_table_shares_eight_axis_tables():
    _, offsets, heights, widths, _ = batch_case()
    resize, crop = BATCH_SETTING
    st, tab = c_table(offsets, heights, widths, resize, crop)
    assert st == L.RN_OK
    d = tab[:12 * BATCH_B].reshape(BATCH_B, 12)
    assert np.array_equal(d[:, 0], offsets.astype(np.uint32)) and not d[:, 1].any()
    assert np.array_equal(d[:, 2], heights.astype(np.uint32)) and np.array_equal(d[:, 3], widths.astype(np.uint32))
    assert np.array_equal(d[:, 4:10], d[np.arange(BATCH_B) % 8, 4:10]) and len(np.unique(d[:8, 4])) == 8
    for s, (h, w) in enumerate(BATCH_SIZES):
        nh, nw, top, left = P.resize_crop_geometry(h, w, resize, crop)
        assert same_axis(axis_of_table(tab, d[GRID_Y + 1 - 8 + s], 0, crop), P.resize_coefficients(w, nw, left, crop))
        assert same_axis(axis_of_table(tab, d[GRID_Y + 1 - 8 + s], 1, crop), P.resize_coefficients(h, nh, top, crop))


# ---- the offset case: an image behind 2^32 bytes ------------------------------------------------------------------------
OFFSET_BYTES = (1 << 32) + 65536
OFFSET_AT = (1, (1 << 32) + 3)
OFFSET_SETTING = (256, 224)


@cached
def offset_case():
    """two 33 x 35 images and their crops; `low`: the first 4096 bytes of the buffer (image 0 at offset 1)"""
    imgs = [structured_image(33, 35, 8100), structured_image(33, 35, 8101)]
    low = np.zeros(4096, dtype=np.uint8)
    low[1:1 + imgs[0].size] = imgs[0].reshape(-1)
    want = np.stack([P.resize_crop_u8(a, *OFFSET_SETTING) for a in imgs])
    return imgs, low, want


def test_offset_case_needs_the_high_word():
    imgs, low, want = offset_case()
    n = 33 * 35 * 3
    assert OFFSET_AT[1] >> 32 == 1 and OFFSET_AT[1] & 0xFFFFFFFF == 3 and OFFSET_AT[1] + n <= OFFSET_BYTES
    st, tab = c_table(OFFSET_AT, [33, 33], [35, 35], *OFFSET_SETTING)
    assert st == L.RN_OK and list(tab[:2]) == [1, 0] and list(tab[12:14]) == [3, 1]
    # without the high word image 1 is read at offset 3: image 0's bytes, shifted by 2
    wrong = P.resize_crop_u8(low[3:3 + n].reshape(33, 35, 3), *OFFSET_SETTING)
    assert np.array_equal(low[3:1 + n], imgs[0].reshape(-1)[2:])
    assert not np.array_equal(wrong, want[1]) and not np.array_equal(want[0], want[1])


# =====================================================================================================================
# B. rn_image_u8_to_nhwc_pad_dt
# =====================================================================================================================
def target(bf16, B, H, W, cpad, border, src_ptr=0, dst_ptr=0):
    """the `fast` predicate of rn_image_u8_to_nhwc_pad_dt restated: "x16" (one 16-byte store per thread and step)
    or "element" """
    per_img = (H + 2 * border) * (W + 2 * border) * cpad
    fast = (H * W > 0 and (H * W * 3) % 4 == 0 and H * W * 3 < 1 << 30 and per_img < 1 << 31 and per_img % (8 if bf16 else 4) == 0
            and (border == 0 or border >= 3) and W + 2 * border >= 4 and src_ptr % 4 == 0 and dst_ptr % 16 == 0)
    return "x16" if fast else "element"


def x16_form(bf16, B, H, W, cpad, border):
    """launch_x16 restated: (n16 stores per image, steps per thread, launches)"""
    n16 = (H + 2 * border) * (W + 2 * border) * cpad // (8 if bf16 else 4)
    return n16, 4 if B * n16 >= 4 * 256 * 2048 else 1, -(-B // GRID_Y)


def magic_div(d):
    """magic_div of rn_image.hip restated: n / d == (n * mul) >> (32 + shr) for n < 2^31"""
    lg = 0
    while (1 << lg) < d:
        lg += 1
    p = 31 + lg
    return ((1 << p) + d - 1) // d, p - 32


NORM_WIDE = (1 << 20) - 4
# (B, H, W, border): run in fp32 and bf16 with Cpad 3 and 4 unless `only` names one combination
NORM_CASES = {
    "x16_second_launch": (GRID_Y + 2, 2, 2, 3),
    "element_second_launch": (GRID_Y + 2, 1, 1, 0),
    "widest_row": (1, 1, NORM_WIDE, 0),
    "tallest_image": (1, NORM_WIDE, 4, 0),
    "widest_row_with_border": (1, 1, NORM_WIDE, 3),
    "wp_1372": (3, 30, 1366, 3),
    "wp_1366_four_steps": (2, 768, 1366, 0),
}
NORM_ONLY = {"widest_row_with_border": [(True, 4)]}
NORM_COMBOS = [(False, 3), (False, 4), (True, 3), (True, 4)]          # (bf16, Cpad)
# the kernel each combination is meant for.  3 * (2^20 - 4) elements are 4 mod 8: the bf16 / Cpad 3 row of the widest
# image is no whole number of 16-byte stores and goes to the element kernel, at the same width
NORM_ELEMENT = {("element_second_launch", c) for c in NORM_COMBOS} | {("widest_row", (True, 3))}


def norm_params():
    return [(name, bf16, cpad) for name in NORM_CASES for bf16, cpad in NORM_ONLY.get(name, NORM_COMBOS)]


@cached
def norm_pixels(name):
    B, H, W, _ = NORM_CASES[name]
    px = np.random.default_rng(9000 + sorted(NORM_CASES).index(name)).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    px.setflags(write=False)
    return px


@cached
def norm_want(name, bf16, cpad):
    """numpy alone, on purpose: preprocess.normalize_u8, NHWC, zero border and pad channel, for bf16 ops.to_bf16_bits --
    not another device kernel.  The raw bits: uint32 (fp32) or uint16 (bf16)."""
    B, H, W, border = NORM_CASES[name]
    x = P.normalize_u8(norm_pixels(name))
    want = np.zeros((B, H + 2 * border, W + 2 * border, cpad), dtype=np.float32)
    want[:, border:border + H, border:border + W, :3] = x.transpose(0, 2, 3, 1)
    bits = ops.to_bf16_bits(want).reshape(want.shape) if bf16 else want.view(np.uint32)
    bits.setflags(write=False)
    return bits


@pytest.mark.parametrize("name,bf16,cpad", norm_params())
def test_normaliser_cases_reach_their_kernel(name, bf16, cpad):
    B, H, W, border = NORM_CASES[name]
    assert H < 1 << 20 and W < 1 << 20
    want_target = "element" if (name, (bf16, cpad)) in NORM_ELEMENT else "x16"
    assert target(bf16, B, H, W, cpad, border) == want_target
    bits = norm_want(name, bf16, cpad)
    assert bits.shape == (B, H + 2 * border, W + 2 * border, cpad)
    inside = bits[:, border:border + H, border:border + W, :3]
    assert len(np.unique(inside)) >= min(200, len(np.unique(norm_pixels(name)))), "the inside carries the pixels"
    if border:
        assert not bits[:, :border].any() and not bits[:, :, -border:].any()
    if cpad == 4:
        assert not bits[..., 3].any()
    if B > GRID_Y:
        px = norm_pixels(name)
        assert -(-B // GRID_Y) == 2
        for late, early in ((GRID_Y, 0), (GRID_Y + 1, 1)):
            assert not np.array_equal(px[late], px[early]) and not np.array_equal(bits[late], bits[early])


def test_normaliser_divisors_and_steps():
    assert x16_form(False, *NORM_CASES["wp_1366_four_steps"][:3], 4, 0)[1] == 4, "fp32, Cpad 4: four stores a thread"
    assert x16_form(False, *NORM_CASES["wp_1372"][:3], 4, 3)[1] == 1
    assert x16_form(False, *NORM_CASES["x16_second_launch"][:3], 3, 3) == (48, 4, 2)
    assert x16_form(True, *NORM_CASES["x16_second_launch"][:3], 3, 3) == (24, 1, 2)
    wps = {n: c[2] + 2 * c[3] for n, c in NORM_CASES.items()}
    assert wps["widest_row"] == (1 << 20) - 4 and wps["tallest_image"] == 4 and wps["widest_row_with_border"] == (1 << 20) + 2
    assert wps["wp_1372"] == 1372 and wps["wp_1366_four_steps"] == 1366
    for wp in (1372, 1366):
        assert wp & (wp - 1), "no power of two"
    # divisions per padded row that do not land on a row start
    assert 36 * 1372 * 4 // 4 > 4000 and 768 * 1366 > 4000


def stores_that_wrap(bf16, H, W, cpad, border):
    """how many 16-byte stores of one padded image hold elements of two padded rows"""
    ne, wp = (8 if bf16 else 4), W + 2 * border
    first = np.arange(0, (H + 2 * border) * wp * cpad, ne, dtype=np.int64)
    return int(((first // (wp * cpad)) != ((first + ne - 1) // (wp * cpad))).sum())


def test_which_cases_have_stores_across_two_rows():
    """With Cpad 4 a bf16 store is two whole pixels, so an even W + 2b (2^20 + 2 is one) never splits a store over two
    rows; the stores that do wrap are those of Cpad 3 at Wp = 1372 and 1366."""
    _, H, W, border = NORM_CASES["widest_row_with_border"]
    assert stores_that_wrap(True, H, W, 4, border) == 0
    _, H, W, border = NORM_CASES["wp_1372"]
    assert stores_that_wrap(True, H, W, 3, border) > 0 and stores_that_wrap(True, H, W, 4, border) == 0
    _, H, W, border = NORM_CASES["wp_1366_four_steps"]
    assert stores_that_wrap(True, H, W, 3, border) > 0 and stores_that_wrap(False, H, W, 3, border) > 0


@pytest.mark.parametrize("wp", [4, 5, 7, 1366, 1372, 2054, (1 << 20) - 4, (1 << 20) + 2])
def test_magic_div_restated(wp):
    """(n * mul) >> (32 + shr) == n // Wp at n = 0, every multiple of Wp below 2^31 minus one and plus zero, and
    2^31 - 1: where a multiply-high division goes wrong first.  Needs no library."""
    mul, shr = magic_div(wp)
    assert 0 < mul < 1 << 32 and 0 <= shr < 32
    sh = np.uint64(32 + shr)
    for n in (0, (1 << 31) - 1):
        assert (n * mul) >> (32 + shr) == n // wp
    last = ((1 << 31) - 1) // wp
    step = 1 << 17            # (arrays that stay in cache: 2^29 multiples of 4 take a few seconds)
    for k0 in range(1, last + 1, step):
        k = np.arange(k0, min(k0 + step, last + 1), dtype=np.uint64)
        n = k * np.uint64(wp)
        assert np.array_equal((n * np.uint64(mul)) >> sh, k), (wp, k0)
        assert np.array_equal(((n - np.uint64(1)) * np.uint64(mul)) >> sh, k - np.uint64(1)), (wp, k0)
