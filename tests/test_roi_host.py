"""RoIAlign over the pyramid, the host side: the float64 reference against an oracle built from torch alone, the fp32
statement of the contract against the float64 reference within a derived bound, the level thresholds against
torchvision's LevelMapper formula, and the small helpers.  No test here needs a GPU.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import ops
from resnet_c_amd import roi as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24                       # the unit roundoff of fp32
MAP = (2, 8, 13, 17)                 # [B, C, h, w]
SCALE = 0.25                         # the image is 52 x 68
SPECIAL = np.array([[0, 900.0, 700.0, 960.0, 790.0],       # far outside
                    [1, 20.3, 17.7, 20.3, 17.7],           # zero size
                    [0, 31.2, 9.1, 31.5, 9.3],             # below a pixel of the map
                    [1, -40.0, -30.0, 120.0, 90.0]],       # larger than the image
                   dtype=np.float32)


def case_map(seed=11):
    return np.random.default_rng(seed).standard_normal(MAP).astype(np.float32)


def case_rois(seed=12, n=40):
    """n random boxes that reach outside the 52 x 68 image, then the four special ones"""
    rng = np.random.default_rng(seed)
    H, W = MAP[2] / SCALE, MAP[3] / SCALE
    cx, cy = rng.uniform(-8, W + 8, n), rng.uniform(-8, H + 8, n)
    bw, bh = rng.uniform(1, 50, n), rng.uniform(1, 40, n)
    r = np.stack([rng.integers(0, MAP[0], n).astype(np.float64), cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], axis=1)
    return np.concatenate([r.astype(np.float32), SPECIAL], axis=0)


def sample_coords(roi, scale, P, S, aligned):
    """the contract's sample coordinates of one axis pair in float64: (y [PH*S], x [PW*S]) and the largest magnitude
    among the values they are formed from"""
    off = 0.5 if aligned else 0.0
    _, x1, y1, x2, y2 = (float(v) for v in roi)
    x1s, y1s, x2s, y2s = x1 * scale - off, y1 * scale - off, x2 * scale - off, y2 * scale - off
    rw, rh = x2s - x1s, y2s - y1s
    if not aligned:
        rw, rh = max(rw, 1.0), max(rh, 1.0)
    bh, bw = rh / P[0], rw / P[1]
    y = (y1s + np.arange(P[0])[:, None] * bh + (np.arange(S)[None, :] + 0.5) * bh / S).reshape(-1)
    x = (x1s + np.arange(P[1])[:, None] * bw + (np.arange(S)[None, :] + 0.5) * bw / S).reshape(-1)
    return y, x, max(abs(x1s), abs(x2s), abs(y1s), abs(y2s), abs(rw), abs(rh), 1.0)


def torch_oracle(m_nchw, rois, scale, P, S, aligned):
    """RoIAlign from torch's own operators: bilinear grid_sample with align_corners=True and border padding on the
    sample grid (the contract's clamps), samples outside [-1, h] x [-1, w] zeroed, then the mean over S x S"""
    m = torch.from_numpy(np.asarray(m_nchw, dtype=np.float64))
    h, w = m.shape[2:]
    out = []
    for roi in np.asarray(rois, dtype=np.float64):
        y, x, _ = sample_coords(roi, scale, P, S, aligned)
        gy, gx = torch.from_numpy(2.0 * y / (h - 1) - 1.0), torch.from_numpy(2.0 * x / (w - 1) - 1.0)
        grid = torch.stack([gx[None, :].expand(len(y), -1), gy[:, None].expand(-1, len(x))], dim=-1)[None]
        v = F.grid_sample(m[int(roi[0]):int(roi[0]) + 1], grid, mode="bilinear", padding_mode="border", align_corners=True)
        ok = torch.from_numpy(((y >= -1) & (y <= h))[:, None] & ((x >= -1) & (x <= w))[None, :])
        out.append(F.avg_pool2d(v * ok, S)[0].numpy())
    return np.stack(out)


CASES = [(aligned, S) for aligned in (False, True) for S in (1, 2, 3)]


@pytest.mark.parametrize("aligned,S", CASES)
def test_float64_reference_is_torchs_arithmetic(aligned, S):
    m, rois = case_map(), case_rois()
    for P in ((7, 7), (3, 5)):
        got = RO.roi_align_f64([m], rois, [SCALE], P, S, aligned)
        want = torch_oracle(m, rois, SCALE, P, S, aligned)
        assert got.shape == want.shape == (len(rois), MAP[1]) + P and got.dtype == np.float64
        err = float(np.abs(got - want).max())
        print(f"\n  roi_align_f64 against torch: aligned={aligned} S={S} {P}: max difference {err:.3e}")
        assert err <= 1e-12, (aligned, S, P, err)
    assert np.abs(got[len(rois) - 4]).max() == 0.0          # the far-outside box: no sample contributes


@pytest.mark.parametrize("aligned,S", CASES)
def test_fp32_contract_within_its_bound_of_float64(aligned, S):
    """The fp32 statement against float64, per RoI.  With u = 2^-24, V = max |map| and A the largest magnitude among
    the values a coordinate is formed from (the scaled corners, the extent, 1):
      * a sample coordinate is the result of at most 9 fp32 operations (scale, offset, extent, bin size, ph * bin,
        the sum, (iy + 0.5) * bin, / S, the sum), each with a result of magnitude at most 2 A and none amplified by
        more than the bin index it is multiplied with, which the division by PH before has paid for: at most
        d = 16 u A off the float64 coordinate;
      * the bilinear value has slope at most 2 V along either axis (the difference of two neighbours), so the two
        coordinates move a sample by at most 4 V d;
      * the weights (1 - l, the product), the four products and three sums of a sample, the S^2 - 1 sums of a bin and
        the division round at most 7 + S^2 + 1 <= 20 times, each by at most u V.
    bound = V (64 u A + 20 u).  That holds while no sample sits within d of -1, h or w, where a sample's contribution
    jumps (the contract includes y == -1 and y == h): the test asserts that of its own inputs in float64."""
    m, rois = case_map(), case_rois()
    V = float(np.abs(m).max())
    nhwc = np.ascontiguousarray(m.transpose(0, 2, 3, 1))
    P = (7, 7)
    got = ops.roi_align_ref([nhwc], rois, [SCALE], P, S, aligned).astype(np.float64)
    ref = RO.roi_align_f64([m], rois, [SCALE], P, S, aligned)
    worst = 0.0
    for r, roi in enumerate(rois):
        y, x, A = sample_coords(roi.astype(np.float64), SCALE, P, S, aligned)
        d = 16 * U * A
        gap = min(np.abs(y + 1).min(), np.abs(y - MAP[2]).min(), np.abs(x + 1).min(), np.abs(x - MAP[3]).min())
        assert gap > d, ("a sample within the coordinate error of a jump", r, gap, d)
        bound = V * (64 * U * A + 20 * U)
        err = float(np.abs(got[r] - ref[r]).max())
        worst = max(worst, err)
        assert err <= bound, (r, err, bound)
    print(f"\n  roi_align_ref against float64: aligned={aligned} S={S}: max error {worst:.3e} (V = {V:.2f})")


def torchvision_levels(area, k_min, k_max, s0, k0, dtype):
    """torchvision's LevelMapper on areas: floor(k0 + log2(sqrt(area) / s0) + 1e-6) clamped, minus k_min"""
    a = torch.from_numpy(np.asarray(area)).to(dtype)
    lv = torch.floor(k0 + torch.log2(torch.sqrt(a) / s0) + torch.tensor(1e-6, dtype=dtype))
    return (torch.clamp(lv, min=k_min, max=k_max).to(torch.int64) - k_min).numpy()


def test_level_thresholds_are_torchvisions_level_mapper():
    scales = [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    thr = ops.roi_level_thresholds(scales)
    want = []
    for j in range(3):
        t = (224.0 * 2.0 ** (2 + 1 + j - 4 - 1e-6)) ** 2
        f = np.float32(t)
        want.append(f if float(f) >= t else np.nextafter(f, np.float32(np.inf)))
    assert thr.dtype == np.float32 and np.array_equal(thr, np.array(want, np.float32)), (thr, want)
    assert np.allclose(thr, [12543.983, 50175.934, 200703.73], rtol=1e-6)
    rng = np.random.default_rng(5)
    n = 400000
    x1, y1 = rng.uniform(0, 400, n).astype(np.float32), rng.uniform(0, 400, n).astype(np.float32)
    bw, bh = rng.uniform(4, 900, n).astype(np.float32), rng.uniform(4, 900, n).astype(np.float32)
    rois = np.stack([np.zeros(n, np.float32), x1, y1, x1 + bw, y1 + bh], axis=1)
    area = (rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2])
    k = 4 + np.log2(np.sqrt(area.astype(np.float64)) / 224.0)
    near = np.abs(k - np.round(k)) <= 1e-5            # torch's own fp32 log2 decides these either way
    assert near.mean() < 1e-3, near.mean()
    got = ops.roi_levels_ref(rois, thr)
    for dtype in (torch.float32, torch.float64):
        tv = torchvision_levels(area, 2, 5, 224.0, 4, dtype)
        assert np.array_equal(got[~near], tv[~near]), dtype
    assert set(got.tolist()) == {0, 1, 2, 3}
    squares = np.array([[0, 10, 20, 10 + s, 20 + s] for s in (56, 112, 224, 448, 896)], dtype=np.float32)
    assert (ops.roi_levels_ref(squares, thr) + 2).tolist() == [2, 3, 4, 5, 5]
    assert ops.roi_levels_ref(squares, thr, images=1).tolist() == [0, 1, 2, 3, 3]
    bad = squares.copy()
    bad[:, 0] = [-1, 1, 0.5, np.nan, 0]
    assert ops.roi_levels_ref(bad, thr, images=1).tolist() == [-1, -1, -1, -1, 3]
    # other pyramids: two levels from stride 8, a single level (no threshold), another canonical box
    assert np.array_equal(ops.roi_level_thresholds([1 / 8, 1 / 16]), thr[1:2])
    assert ops.roi_level_thresholds([1 / 16]).size == 0
    assert np.array_equal(ops.roi_level_thresholds(scales, 448.0, 5), thr)
    with pytest.raises(ValueError):
        ops.roi_level_thresholds([0.25, 0.0])
    with pytest.raises(ValueError):
        ops.roi_level_thresholds([0.5] * 5)


def test_boxes_to_rois_and_infer_scales():
    a = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.float32)
    b = np.zeros((0, 4), np.float32)
    c = np.array([[9, 10, 11, 12]], np.float64)
    rois = RO.boxes_to_rois([a, b, c])
    assert rois.dtype == np.float32 and rois.tolist() == [[0, 1, 2, 3, 4], [0, 5, 6, 7, 8], [2, 9, 10, 11, 12]]
    assert RO.boxes_to_rois([]).shape == (0, 5)
    assert RO.infer_scales([(200, 336), (100, 168), (50, 84), (25, 42)], (800, 1344)) == (0.25, 0.125, 0.0625, 0.03125)
    assert RO.infer_scales([(18, 10), (9, 5), (5, 3), (3, 2)], (72, 40)) == (0.25, 0.125, 0.0625, 0.03125)   # odd sizes round
    assert RO.infer_scales([(9, 5)], (9, 5)) == (1.0,)
    assert RO.infer_scales([(18, 5)], (72, 40)) == (0.25,)           # the height's, as torchvision returns it


def test_pooler_parameters_and_levels():
    p = R.MultiScaleRoIAlign(["0", "2"], 7, 2)
    assert p.output_size == (7, 7) and p.sampling_ratio == 2 and p.canonical_scale == 224.0 and p.canonical_level == 4
    assert p.level_indices(("0", "1", "2", "3", "pool")) == (0, 2)
    assert R.MultiScaleRoIAlign(["1"], (3, 5), 1).output_size == (3, 5)
    for names in (["0", "4"], ["pool"], ["2", "0"], ["1", "1"]):
        with pytest.raises(ValueError):
            R.MultiScaleRoIAlign(names, 7, 2).level_indices(("0", "1", "2", "3", "pool"))
    with pytest.raises(ValueError):
        R.MultiScaleRoIAlign([], 7, 2)
    req = p.request(("0", "1", "2", "3", "pool"), 0x1000, 9, (72, 40), 0x2000)
    assert (req.K, req.image_h, req.image_w, req.n_levels, list(req.level)[:2], req.PH, req.PW) == (9, 72, 40, 2, [0, 2], 7, 7)
    assert req.levels_out is None and req.canonical_scale == 224.0 and req.canonical_level == 4
    rois = np.array([[0, 1, 1, 5, 5], [2, 1, 1, 5, 5]], np.float32)
    assert ops.roi_image_valid(rois, 3).tolist() == [True, True] and ops.roi_image_valid(rois, 2).tolist() == [True, False]
    with pytest.raises(ValueError):
        RO.upload_rois(rois, 2)


def test_reference_rows_of_an_invalid_image_are_zero():
    m = np.ascontiguousarray(case_map().transpose(0, 2, 3, 1))
    rois = case_rois()[:6].copy()
    rois[1, 0], rois[3, 0], rois[4, 0] = 2, 0.5, np.nan
    out, lv = ops.roi_align_ref([m], rois, [SCALE], 7, 2, return_levels=True)
    assert lv.tolist() == [0, -1, 0, -1, -1, 0]
    assert not out[[1, 3, 4]].any() and out[0].any() and out[5].any()


def test_surface():
    text = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    declared = set(re.findall(r"RN_API[^;(]*?\b(rn_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rn_[a-z0-9_]+)", out))
    lib = L.lib()
    for name in ("rn_roi_level_thresholds", "rn_roi_align_forward_dt", "rn_fpn_forward_rois", "rn_model_forward_rois",
                 "rn_model_forward_rois_u8"):
        assert name in declared and name in exported and name in L.SIGNATURES and hasattr(lib, name), name
    assert "rn_roi_align_window" not in exported and "rn_fpn_roi_step" not in exported      # library-internal
    assert ctypes.sizeof(L.RoiPool) == 112
    for name in ("MultiScaleRoIAlign", "boxes_to_rois", "infer_scales", "roi_align_f64"):
        assert hasattr(R, name), name
    for name in ("roi_align", "roi_align_bf16", "roi_align_ref", "roi_level_thresholds", "roi_levels_ref"):
        assert hasattr(ops, name), name
