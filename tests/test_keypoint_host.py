"""The keypoint head's host side (resnet_c_amd.keypoint), no GPU: the numpy contracts against torch's own
conv_transpose2d, interpolate and torchvision's heatmaps_to_keypoints restated with torch.nn.functional (torchvision
itself is not a dependency), within bounds derived from the operation counts; the edge rows; the state handling.  The
generators at the top are shared with tests/test_keypoint_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from resnet_c_amd import detection as D
from resnet_c_amd import keypoint as KP

F32 = np.float32
U = 2.0 ** -24  # one fp32 rounding is at most U relative


# ---- generators shared with the GPU tests ----------------------------------------------------------------------
def gaussian_heat(K, Kp, S, seed=0):
    """[K,Kp,S,S] fp32: one Gaussian peak per map (amplitude 2..8, sigma 1.5..4, anywhere in the map) on an offset of -3
    under white noise of 0.3"""
    g = np.random.default_rng([seed, K, Kp, S])
    amp, sig = g.uniform(2.0, 8.0, (K, Kp, 1, 1)), g.uniform(1.5, 4.0, (K, Kp, 1, 1))
    cy, cx = g.uniform(0.0, S, (K, Kp, 1, 1)), g.uniform(0.0, S, (K, Kp, 1, 1))
    yy, xx = np.arange(S)[None, None, :, None] + 0.5, np.arange(S)[None, None, None, :] + 0.5
    v = amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * sig ** 2)) - 3.0 + 0.3 * g.standard_normal((K, Kp, S, S))
    return v.astype(F32)


def random_boxes(K, lo=1.0, hi=330.0, seed=0):
    """[K,4] fp32: sides lo..hi at fractional origins"""
    g = np.random.default_rng([seed, K, 0x424F58])
    x1, y1 = g.uniform(0.0, 40.0, K), g.uniform(0.0, 40.0, K)
    return np.stack([x1, y1, x1 + g.uniform(lo, hi, K), y1 + g.uniform(lo, hi, K)], axis=1).astype(F32)


def edge_boxes():
    """([n,4] fp32, labels [n] int32, what each row is): the edge rows of the contract at max_size (240, 320)"""
    rows = [((3.25, 2.5, 3.75, 2.75), 1, "under one pixel"),
            ((2.0, 1.0, 12.0, 8.0), 1, "integer sides"),
            ((1.5, 0.5, 4.0, 3.25), 2, "shrinking below S = 4 and 8"),
            ((0.0, 0.0, 1.0, 1.0), 1, "1 x 1"),
            ((10.0, 4.0, 309.5, 203.25), 3, "about 300 x 200: many chunks"),
            ((5.0, 5.0, float("nan"), 9.0), 1, "a NaN coordinate"),
            ((5.0, 5.0, float("inf"), 9.0), 1, "an infinite coordinate"),
            ((0.0, 0.0, 320.5, 9.0), 1, "over max_w"),
            ((0.0, 0.0, 9.0, 240.25), 1, "over max_h"),
            ((1.0, 1.0, 30.0, 20.0), 0, "label 0"),
            ((1.0, 1.0, 30.0, 20.0), -1, "label -1"),
            ((7.75, 3.125, 70.0, 33.0), 5, "fractional")]
    return np.array([r[0] for r in rows], F32), np.array([r[1] for r in rows], np.int32), [r[2] for r in rows]


EDGE_SIZE = (240, 320)
EDGE_OUT = (5, 6, 7, 8, 9, 10)  # the rows of edge_boxes that are OUT


def panel_case(Kp, M, K, seed=0):
    """(t [K,M,M,16Kp], bias [Kp]) fp32"""
    g = np.random.default_rng([seed, Kp, M, K])
    return g.standard_normal((K, M, M, 16 * Kp)).astype(F32), (g.standard_normal(Kp) * 0.5).astype(F32)


def same_bits(a, b):
    """equal bit for bit, a NaN equal to a NaN (its payload is no part of the contract)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | both_nan))


# ---- torchvision's code, restated ------------------------------------------------------------------------------
def tv_heatmaps_to_keypoints(maps, rois, dtype=torch.float64):
    """torchvision.models.detection.roi_heads.heatmaps_to_keypoints in `dtype`: (xy_preds [K,Kp,3], end_scores [K,Kp],
    the resized maps)"""
    maps, rois = torch.from_numpy(np.asarray(maps)).to(dtype), torch.from_numpy(np.asarray(rois)).to(dtype)
    offset_x, offset_y = rois[:, 0], rois[:, 1]
    widths, heights = (rois[:, 2] - rois[:, 0]).clamp(min=1), (rois[:, 3] - rois[:, 1]).clamp(min=1)
    widths_ceil, heights_ceil = widths.ceil(), heights.ceil()
    n = maps.shape[1]
    xy, scores, resized = torch.zeros((len(rois), 3, n), dtype=dtype), torch.zeros((len(rois), n), dtype=dtype), []
    for i in range(len(rois)):
        rw, rh = int(widths_ceil[i].item()), int(heights_ceil[i].item())
        wc, hc = widths[i] / rw, heights[i] / rh
        roi_map = F.interpolate(maps[i][:, None], size=(rh, rw), mode="bicubic", align_corners=False)[:, 0]
        w = roi_map.shape[2]
        pos = roi_map.reshape(n, -1).argmax(dim=1)
        x_int = pos % w
        y_int = torch.div(pos - x_int, w, rounding_mode="floor")
        xy[i, 0, :] = (x_int.to(dtype) + 0.5) * wc + offset_x[i]
        xy[i, 1, :] = (y_int.to(dtype) + 0.5) * hc + offset_y[i]
        xy[i, 2, :] = 1
        scores[i, :] = roi_map[torch.arange(n), y_int, x_int]
        resized.append(roi_map.numpy())
    return xy.permute(0, 2, 1).numpy(), scores.numpy(), resized


# ---- the bounds --------------------------------------------------------------------------------------------------
def heat_bound(t, bias) -> np.ndarray:
    """[K,Kp,4M,4M]: how far the fp32 heat map may lie from float64, from the operation count, first order in U.  With
    A = |bias| + the sum of the |taps| of a low-resolution pixel: the taps arrive rounded (U |tap| each) and each of the
    at most four additions rounds to U |partial sum| <= U A, so low is within 5 U A.  The resize's weights (0, 0.25, 0.75,
    1) are exact; an output is a convex combination of four low values through four roundings (a product and a sum per
    axis), each at most U times that combination of |low| <= A.  Both push through the same convex combination: 9 U
    times the resize of A.  The second-order terms are covered by the factor 1 + 2^-10."""
    A = KP.heatmaps_ref(np.abs(np.asarray(t, np.float64)), np.abs(np.asarray(bias, np.float64)), np.float64)
    return 9.0 * U * A * (1 + 2.0 ** -10)


def _cubic_constants():
    """(the largest sum over the four taps of |c_i(t)|, of |c_i'(t)|) over t in [0, 1], A = -0.75, on a grid of 2^-12
    with the slack a quadratic's (cubic's) slope allows between grid points"""
    t = np.linspace(0.0, 1.0, 4097)
    outer = lambda x: ((-0.75 * x + 3.75) * x - 6.0) * x + 3.0        # noqa: E731
    inner = lambda x: (1.25 * x - 2.25) * x * x + 1.0                  # noqa: E731
    d_outer = lambda x: (-2.25 * x + 7.5) * x - 6.0                    # noqa: E731
    d_inner = lambda x: (3.75 * x - 4.5) * x                           # noqa: E731
    c = np.abs(outer(t + 1)) + np.abs(inner(t)) + np.abs(inner(1 - t)) + np.abs(outer(2 - t))
    d = np.abs(d_outer(t + 1)) + np.abs(d_inner(t)) + np.abs(d_inner(1 - t)) + np.abs(d_outer(2 - t))
    return float(c.max()) + 4.2 * 2.0 ** -12, float(d.max()) + 16.0 * 2.0 ** -12


def score_bound(vmax: float, S: int) -> float:
    """How far a value of the fp32 bicubic resize may lie from float64 where |heat| <= vmax, first order in U.  Per axis:
      the source coordinate: scale = fl(S / n) is within U relative, its product with o + 0.5 (exact) rounds once more
        and is at most S, the subtraction of 0.5 rounds to U |src| <= U S: 3 U S; tt = src - floor(src) adds at most U.
        The interpolant is continuous in the coordinate (across cells too) with slope at most D vmax, D the largest
        sum of the |c_i'|: D (3 S + 1) U vmax.  This is the dominant term.
      the coefficients: an outer one is six roundings of intermediates of at most 4.5, each carried through at most
        two more multiplications by x <= 2, and its argument tt + 1 rounds once under a slope of at most 0.75:
        (6 * 4.5 * 4 + 1.5) U; an inner one five roundings of at most 2.25 and its argument under a slope of at most
        1.35: (5 * 2.25 + 1.35) U.  Two of each, times vmax.
      the sum: four products and three additions, each at most U times the sum of the |c_i v_i| <= C vmax: 7 C U vmax
        (C the largest sum of the |c_i|).
    The horizontal pass gives row values within e1 = that at vmax, of magnitude at most C vmax; the vertical pass
    carries e1 through coefficients that sum to at most C in magnitude and adds its own at C vmax.  The second-order
    terms are covered by the factor 1 + 2^-10."""
    C, Dc = _cubic_constants()
    per_axis = Dc * (3 * S + 1) + 2 * (6 * 4.5 * 4 + 1.5) + 2 * (5 * 2.25 + 1.35) + 7 * C
    return 2.0 * C * per_axis * U * vmax * (1 + 2.0 ** -10)


# ---- panel and heat map ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,Kp,M,K", [(8, 1, 1, 2), (8, 3, 2, 3), (16, 17, 14, 2), (4, 2, 5, 1)])
def test_panel_and_heatmaps_against_torch(cin, Kp, M, K):
    g = np.random.default_rng([cin, Kp, M])
    x = g.standard_normal((K, cin, M, M))
    w, b = g.standard_normal((cin, Kp, 4, 4)) / np.sqrt(cin), g.standard_normal(Kp) * 0.5
    low = F.conv_transpose2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride=2, padding=1)
    want = F.interpolate(low, scale_factor=2.0, mode="bilinear", align_corners=False, recompute_scale_factor=False).numpy()
    rows = KP.deconv_panel(w)
    assert rows.shape == (16 * Kp, cin)
    t = np.einsum("kchw,oc->khwo", x, rows)
    # float64: the identity itself
    got64 = KP.heatmaps_ref(t, b, np.float64)
    assert got64.shape == (K, Kp, 4 * M, 4 * M)
    scale = KP.heatmaps_ref(np.abs(t), np.abs(b), np.float64)
    assert np.all(np.abs(got64 - want) <= 16 * 2.0 ** -53 * scale + 1e-300)
    # fp32: the contract within its derived bound
    got = KP.heatmaps_ref(t.astype(F32), b.astype(F32))
    assert got.dtype == F32
    err, bound = np.abs(got.astype(np.float64) - want), heat_bound(t, b) + U * np.abs(b).max()  # (bias rounded to fp32)
    print(f"heat: max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)


def test_overlap_add_order_is_ky_then_kx():
    """a pixel whose four taps cancel badly shows the order: 1e8 + 1 - 1e8 + 1 differs by order in fp32"""
    t = np.zeros((1, 2, 2, 16), F32)
    # output (1, 1) reads (iy, ky) in ((0, 2), (1, 0)) and (ix, kx) likewise; ascending ky, then kx:
    # (ky 0, kx 0) = t[1][1][0], (0, 2) = t[1][0][2], (2, 0) = t[0][1][8], (2, 2) = t[0][0][10]
    t[0, 1, 1, 0], t[0, 1, 0, 2], t[0, 0, 1, 8], t[0, 0, 0, 10] = 1e8, 1.0, -1e8, 1.0
    low = KP._overlap_add(t, np.zeros(1, F32), F32)
    assert low[0, 0, 1, 1] == F32(F32(F32(F32(1e8) + F32(1.0)) + F32(-1e8)) + F32(1.0)) == F32(1.0)


# ---- the search --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def search_case():
    K, Kp, S = 48, 17, 56
    heat, boxes = gaussian_heat(K, Kp, S, seed=1), random_boxes(K, 1.0, 330.0, seed=1)
    return heat, boxes, KP.heatmaps_to_keypoints_ref(heat, boxes, (512, 512)), tv_heatmaps_to_keypoints(heat, boxes)


def test_search_scores_within_bound_of_float64(search_case):
    heat, boxes, (kps, scores), (xy64, s64, resized) = search_case
    K, Kp, S = heat.shape[:3]
    vmax = np.abs(heat.astype(np.float64)).max(axis=(2, 3))
    bound = np.array([[score_bound(vmax[k, j], S) for j in range(Kp)] for k in range(K)])
    # the fp32 maximum against float64's maximum: both lie within the bound of each other's value at their own pixel
    err = np.abs(scores.astype(np.float64) - s64)
    print(f"scores: max err {err.max():.3e}, max err / bound {np.max(err / bound):.4f}, max err / vmax {np.max(err / vmax):.3e}")
    assert np.all(err <= bound)
    # every pixel of the resized map, on the rows where that is cheap
    for k in range(0, K, 8):
        _, _, Wr, Hr, _ = KP.box_sizes_ref(boxes[k:k + 1], (512, 512))
        r32 = KP.bicubic_resize_ref(heat[k], (Hr[0], Wr[0])).astype(np.float64)
        assert np.all(np.abs(r32 - resized[k]) <= bound[k][:, None, None])


def test_search_positions_where_float64_is_decided(search_case):
    heat, boxes, (kps, scores), (xy64, s64, resized) = search_case
    K, Kp, S = heat.shape[:3]
    vmax = np.abs(heat.astype(np.float64)).max(axis=(2, 3))
    decided = np.zeros((K, Kp), bool)
    for k in range(K):
        flat = resized[k].reshape(Kp, -1)
        if flat.shape[1] == 1:
            decided[k] = True
            continue
        top2 = np.partition(flat, -2, axis=1)[:, -2:]
        decided[k] = (top2[:, 1] - top2[:, 0]) > 2.0 * np.array([score_bound(vmax[k, j], S) for j in range(Kp)])
    left_out = int((~decided).sum())
    print(f"positions: {left_out} of {K * Kp} pairs left out ({100.0 * left_out / (K * Kp):.2f} %)")
    assert left_out <= 0.05 * K * Kp
    # identical integer positions there: the coordinates agree to the rounding of three fp32 operations
    w, h, Wr, Hr, _ = KP.box_sizes_ref(boxes, (512, 512))
    tol = 4 * U * (np.abs(boxes).max(axis=1) + np.maximum(w, h))[:, None]
    assert np.all(np.abs(kps[..., 0].astype(np.float64) - xy64[..., 0])[decided] <= np.broadcast_to(tol, (K, Kp))[decided])
    assert np.all(np.abs(kps[..., 1].astype(np.float64) - xy64[..., 1])[decided] <= np.broadcast_to(tol, (K, Kp))[decided])
    assert np.all(kps[..., 2] == 1.0)


@pytest.mark.parametrize("S,size", [(56, (1, 1)), (56, (7, 3)), (56, (61, 100)), (56, (56, 56)), (8, (56, 23)), (1, (5, 4)), (4, (2, 9))])
def test_bicubic_restatement_in_float64(S, size):
    g = np.random.default_rng([S, size[0], size[1]])
    x = g.standard_normal((3, S, S))
    want = F.interpolate(torch.from_numpy(x)[None], size=size, mode="bicubic", align_corners=False)[0].numpy()
    got = KP.bicubic_resize_ref(x, size, np.float64)
    assert np.abs(got - want).max() <= 64 * 2.0 ** -53 * np.abs(x).max()


# ---- edge rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 4, 8, 56])
def test_edge_rows(S):
    boxes, labels, what = edge_boxes()
    K, Kp = len(boxes), 3
    heat = gaussian_heat(K, Kp, S, seed=2)
    kps, scores = KP.heatmaps_to_keypoints_ref(heat, boxes, EDGE_SIZE, labels)
    for k in range(K):
        if k in EDGE_OUT:
            assert np.all(kps[k] == 0.0) and np.all(scores[k] == 0.0), what[k]
        else:
            assert np.all(kps[k, :, 2] == 1.0), what[k]
            assert np.all((kps[k, :, 0] >= boxes[k, 0]) & (kps[k, :, 0] <= max(boxes[k, 2], boxes[k, 0] + 1))), what[k]
            assert np.all((kps[k, :, 1] >= boxes[k, 1]) & (kps[k, :, 1] <= max(boxes[k, 3], boxes[k, 1] + 1))), what[k]
    # a box under one pixel and the 1 x 1 box: a single resized pixel, the centre of the clamped box
    for k in (0, 3):
        assert np.all(kps[k, :, 0] == F32(F32(0.5) * F32(1.0) + boxes[k, 0])), what[k]
    # without labels the label rows are live
    kps2, _ = KP.heatmaps_to_keypoints_ref(heat, boxes, EDGE_SIZE)
    assert np.all(kps2[9, :, 2] == 1.0) and np.all(kps2[10, :, 2] == 1.0)
    # integer sides against torch's own fp32 positions where float64 is decided is the search test's; here: the sizes
    w, h, Wr, Hr, live = KP.box_sizes_ref(boxes, EDGE_SIZE, labels)
    assert (Wr[1], Hr[1]) == (10, 7) and (Wr[0], Hr[0]) == (1, 1) and (Wr[4], Hr[4]) == (300, 200)
    assert [k for k in range(K) if not live[k]] == list(EDGE_OUT)


def test_constant_and_nan_maps():
    boxes = np.array([[2.0, 3.0, 40.5, 25.25], [0.0, 0.0, 9.0, 9.0]], F32)
    const = np.full((2, 2, 8, 8), 1.5, F32)
    const[:, 1] = 0.0
    kps, scores = KP.heatmaps_to_keypoints_ref(const, boxes, (64, 64))
    w, h, Wr, Hr, _ = KP.box_sizes_ref(boxes, (64, 64))
    # a constant map: the partition of unity is not exact in fp32, so index 0 wins only among equal values -- on the
    # all-zero map it does, exactly
    assert np.all(scores[:, 1] == 0.0)
    for k in range(2):
        assert kps[k, 1, 0] == F32(F32(0.5) * (w[k] / F32(Wr[k])) + boxes[k, 0])
        assert kps[k, 1, 1] == F32(F32(0.5) * (h[k] / F32(Hr[k])) + boxes[k, 1])
    nan = np.full((2, 2, 8, 8), np.nan, F32)
    nan[:, 1] = gaussian_heat(2, 1, 8, seed=3)[:, 0]
    nan[1, 1, 0, 0] = np.nan  # a NaN among finite values: never the answer unless it is at index 0 of the resized map
    kps, scores = KP.heatmaps_to_keypoints_ref(nan, boxes, (64, 64))
    assert np.all(np.isnan(scores[:, 0]))  # all NaN: index 0 stays
    for k in range(2):
        assert kps[k, 0, 0] == F32(F32(0.5) * (w[k] / F32(Wr[k])) + boxes[k, 0])
    assert np.isfinite(scores[0, 1]) and np.isnan(scores[1, 1])  # (0, 0) of the resized map reads tap (0, 0) alone: a NaN there stays
    assert KP.argmax_ref(np.array([[[1.0, np.nan], [3.0, 3.0]]])) == 2
    assert KP.argmax_ref(np.array([[[np.nan, 5.0], [3.0, 3.0]]])) == 0
    assert KP.argmax_ref(np.array([[[-np.inf, np.nan], [-np.inf, -np.inf]]])) == 0


# ---- host plumbing -----------------------------------------------------------------------------------------------
def test_split_state_both_spellings_and_generate():
    st = KP.generate_keypoint_head_state(64, (64, 128), 5, seed=3)
    shapes = KP.head_shapes(64, (64, 128), 5)
    assert set(st) == set(shapes) and all(st[k].shape == shapes[k] and st[k].dtype == F32 for k in st)
    assert shapes["keypoint_head.2.weight"] == (128, 64, 3, 3) and shapes[KP.PREDICTOR_KEYS[0]] == (128, 5, 4, 4)
    assert KP.layers_of(st) == (64, 128)
    pre = KP.generate_keypoint_head_state(64, (64, 128), 5, seed=3, prefix="roi_heads.")
    other = {"roi_heads.box_head.fc6.weight": np.zeros(1, F32), "keypoint_head.1.weight": np.zeros(1, F32)}
    mine, rest = KP.split_state({**pre, **other})
    assert set(mine) == set(st) and all(np.array_equal(mine[k], st[k]) for k in st)
    assert set(rest) == set(other)  # the odd entries of the Sequential are ReLUs: no such key is the head's
    mine2, rest2 = KP.split_state(st)
    assert set(mine2) == set(st) and not rest2
    assert KP.generate_keypoint_head_state(64, (64,), 3, seed=1)["keypoint_head.0.bias"].shape == (64,)
    assert not np.array_equal(KP.generate_keypoint_head_state(64, (64,), 3, seed=1)["keypoint_head.0.weight"],
                              KP.generate_keypoint_head_state(64, (64,), 3, seed=2)["keypoint_head.0.weight"])


def test_split_detector_state_gains_keypoint_head():
    st = KP.generate_keypoint_head_state(64, (64,), 3, prefix="roi_heads.")
    box = D.generate_box_head_state(64, 64, 3)
    out = D.split_detector_state({**{"roi_heads." + k: v for k, v in box.items()}, **st})
    assert set(out["keypoint_head"]) == set(KP.head_shapes(64, (64,), 3)) and "mask_head" not in out
    assert "keypoint_head" not in D.split_detector_state({"roi_heads." + k: v for k, v in box.items()})


def test_output_spec():
    spec = KP.output_spec(2, 5, 14, 256, 17)
    assert spec == {"keypoints": (F32, (2, 5, 17, 3)), "keypoints_scores": (F32, (2, 5, 17))}
    spec = KP.output_spec(2, 5, 14, 256, 17, ("heatmaps", "rois", "pooled"))
    assert spec == {"keypoint_rois": (F32, (10, 5)), "keypoint_pooled": (F32, (10, 14, 14, 256)),
                    "keypoint_heatmaps": (F32, (2, 5, 17, 56, 56))}
    with pytest.raises(ValueError):
        KP.output_spec(1, 1, 2, 64, 3, ("masks",))
    with pytest.raises(ValueError):
        KP.output_spec(1, 1, 2, 64, 3, ("rois",))


def test_keypoint_head_ref_against_torch_modules():
    """the float64 reference against the modules built by hand: convs with ReLU, conv_transpose2d, interpolate"""
    st = KP.generate_keypoint_head_state(8, (8, 16), 3, seed=5)
    g = np.random.default_rng(5)
    x = g.standard_normal((2, 8, 3, 3))
    y = torch.from_numpy(x)
    for i in range(2):
        y = F.relu(F.conv2d(y, torch.from_numpy(st[f"keypoint_head.{2 * i}.weight"]).double(),
                            torch.from_numpy(st[f"keypoint_head.{2 * i}.bias"]).double(), padding=1))
    y = F.conv_transpose2d(y, torch.from_numpy(st[KP.PREDICTOR_KEYS[0]]).double(), torch.from_numpy(st[KP.PREDICTOR_KEYS[1]]).double(),
                           stride=2, padding=1)
    want = F.interpolate(y, scale_factor=2.0, mode="bilinear", align_corners=False, recompute_scale_factor=False).numpy()
    got = KP.keypoint_head_ref(x, st)
    assert got.shape == (2, 3, 12, 12) and np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)
