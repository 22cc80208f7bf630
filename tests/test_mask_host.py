"""The mask head's host side (resnet_c_amd.mask), no GPU: the numpy contracts against torchvision's code restated with
torch.nn.functional (torchvision itself is not a dependency), the float64 references against hand-built modules, the
state handling.  The generators at the top are shared with tests/test_mask_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from resnet_c_amd import detection as D
from resnet_c_amd import mask as MK

F32 = np.float32


# ---- generators shared with the GPU tests ----------------------------------------------------------------------
def paste_boxes(H, W):
    """[n,4] fp32: boxes inside the image, on its borders, one pixel, x1 == x2, the whole image, expanded past 0 and
    past W (and H), fractional ones, one wholly outside"""
    fw, fh = float(W), float(H)
    rows = [(1.3, 0.7, min(fw - 1.2, 9.6), min(fh - 0.6, 4.2)),      # inside, fractional
            (0.0, 0.0, fw / 2, fh / 2),                             # on the top-left borders
            (fw / 2, fh / 2, fw, fh),                               # on the bottom-right borders
            (1.0, 1.0, 2.0, 2.0),                                   # one pixel
            (2.0, 1.0, 2.0, fh - 1.0),                              # x1 == x2
            (1.0, 2.5, fw - 1.0, 2.5),                              # y1 == y2
            (0.0, 0.0, fw, fh),                                     # the whole image
            (-3.5, -2.25, fw / 3, fh / 3),                          # expanded past 0
            (fw * 0.6, fh * 0.5, fw + 4.75, fh + 1.5),              # past W and H
            (-fw, -fh, 2 * fw, 2 * fh),                             # far past every border
            (fw + 5.0, fh + 5.0, fw + 9.0, fh + 8.0),               # wholly outside
            (0.49, 0.51, 1.49, 1.51)]
    return np.array(rows, F32)


def paste_probs(K, Mo, seed=0):
    g = np.random.default_rng([seed, K, Mo])
    return g.uniform(0.0, 1.0, (K, Mo, Mo)).astype(F32)


def predict_case(Cr, M, C, K, seed=0):
    """(t [K,M,M,4Cr] >= 0 as behind a ReLU, labels with 0, -1, C, C - 1 and 1 among them, weight [C,Cr], bias [C])"""
    g = np.random.default_rng([seed, Cr, M, C])
    t = np.maximum(g.standard_normal((K, M, M, 4 * Cr)), 0).astype(F32)
    w = (g.standard_normal((C, Cr)) * 4.0 / np.sqrt(Cr)).astype(F32)
    b = (g.standard_normal(C) * 0.5).astype(F32)
    labels = np.array(([0, -1, C, C - 1, 1] + list(g.integers(1, C, max(K - 5, 0))))[:K], np.int32)
    return t, labels, w, b


# ---- torchvision's code, restated ------------------------------------------------------------------------------
def tv_expand_boxes(boxes, Mo):
    """torchvision.models.detection.roi_heads.expand_boxes and the .to(int64) of paste_masks_in_image, in fp32 torch"""
    b = torch.from_numpy(np.asarray(boxes, F32))
    scale = float(Mo + 2) / Mo
    w_half = (b[:, 2] - b[:, 0]) * 0.5
    h_half = (b[:, 3] - b[:, 1]) * 0.5
    x_c = (b[:, 2] + b[:, 0]) * 0.5
    y_c = (b[:, 3] + b[:, 1]) * 0.5
    w_half *= scale
    h_half *= scale
    out = torch.zeros_like(b)
    out[:, 0], out[:, 2] = x_c - w_half, x_c + w_half
    out[:, 1], out[:, 3] = y_c - h_half, y_c + h_half
    return out.to(dtype=torch.int64).numpy()


def tv_paste(mask, box, H, W, dtype=torch.float64):
    """torchvision's paste_mask_in_image on the padded mask and the integer box"""
    m = F.pad(torch.from_numpy(np.asarray(mask)).to(dtype)[None, None], (1, 1, 1, 1))
    w, h = max(int(box[2] - box[0] + 1), 1), max(int(box[3] - box[1] + 1), 1)
    m = F.interpolate(m, size=(h, w), mode="bilinear", align_corners=False)[0, 0]
    out = torch.zeros((H, W), dtype=dtype)
    x0, x1, y0, y1 = max(int(box[0]), 0), min(int(box[2]) + 1, W), max(int(box[1]), 0), min(int(box[3]) + 1, H)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = m[(y0 - int(box[1])):(y1 - int(box[1])), (x0 - int(box[0])):(x1 - int(box[0]))]
    return out.numpy()


@pytest.mark.parametrize("Mo", [1, 2, 4, 28])
def test_paste_contract_is_torchvisions(Mo):
    """paste_masks_ref against torchvision's code: the expanded integer boxes, computed in fp32 torch, are EQUAL; the
    values, interpolated in float64 on those integers, agree within (8 + 4 (Mo + 2)) 2^-24 max|mask| -- the bound of
    test_contract_is_torchs_interpolate with the padded side (the rounding of src, of the weights and of the three
    sums)."""
    H, W = 37, 53
    boxes = paste_boxes(H, W)
    probs = paste_probs(boxes.shape[0], Mo)
    ib, live = MK.expand_boxes_ref(boxes, Mo)
    assert live.all()
    assert np.array_equal(ib, tv_expand_boxes(boxes, Mo))
    got = MK.paste_masks_ref(probs, boxes, (H, W))
    assert got.dtype == F32 and got.shape == (boxes.shape[0], H, W)
    bound = (8 + 4 * (Mo + 2)) * 2.0 ** -24 * float(probs.max())
    worst, pasted = 0.0, 0
    for k in range(boxes.shape[0]):
        want = tv_paste(probs[k], ib[k], H, W)
        err = float(np.abs(got[k].astype(np.float64) - want).max())
        assert err <= bound, (Mo, k, err, bound)
        worst, pasted = max(worst, err), pasted + int((want != 0).sum())
    assert pasted > 0 and not got[10].any()       # the box wholly outside pastes nothing
    print(f"\n  paste Mo={Mo}: max error {worst:.3e}, bound {bound:.3e}")


def test_paste_dead_rows_and_random_boxes():
    """rows of a label below 1 or a non-finite box are zeros; 200 random boxes agree with torchvision's integers"""
    H, W, Mo = 37, 53, 4
    g = np.random.default_rng(5)
    c = g.uniform(-10, 60, (200, 2))
    wh = g.uniform(0, 40, (200, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], axis=1).astype(F32)
    assert np.array_equal(MK.expand_boxes_ref(boxes, Mo)[0], tv_expand_boxes(boxes, Mo))
    probs = paste_probs(4, Mo)
    bx = np.array([[1, 1, 9, 9], [1, 1, np.nan, 9], [1, -np.inf, 9, 9], [2, 2, 12, 7]], F32)
    got = MK.paste_masks_ref(probs, bx, (H, W), labels=[1, 1, 1, -1])
    assert got[0].any() and not got[1:].any()
    assert MK.paste_masks_ref(probs, bx, (H, W))[3].any()


def test_deconv_is_a_1x1_panel():
    """ConvTranspose2d(Cin, Cr, 2, 2) as one 1x1 panel of 4 Cr channels plus the (dy, dx) rearrangement, against
    F.conv_transpose2d in float64"""
    g = np.random.default_rng(2)
    K, Cin, Cr, M = 3, 8, 6, 5
    x, w, b = g.standard_normal((K, Cin, M, M)), g.standard_normal((Cin, Cr, 2, 2)), g.standard_normal(Cr)
    rows, shift = MK.deconv_panel(w, b)
    assert rows.shape == (4 * Cr, Cin) and shift.shape == (4 * Cr,)
    t = np.einsum("kchw,oc->khwo", x, rows) + shift
    want = F.conv_transpose2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride=2).numpy()
    got = MK.panel_to_nchw(t)
    assert got.shape == want.shape == (K, Cr, 2 * M, 2 * M)
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(MK.nchw_to_panel(got), t)


def torch_mask_head(state, pooled):
    """MaskRCNNHeads + conv5_mask + ReLU, hand-built from torch.nn in eval mode, float64"""
    st, _ = MK.split_state(state)
    mods, i = [], 0
    while f"mask_head.{i}.0.weight" in st:
        w = st[f"mask_head.{i}.0.weight"]
        conv = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, padding=1).double()
        conv.weight.data = torch.from_numpy(w.astype(np.float64))
        conv.bias.data = torch.from_numpy(st[f"mask_head.{i}.0.bias"].astype(np.float64))
        mods += [conv, torch.nn.ReLU()]
        i += 1
    w = st[MK.PREDICTOR_KEYS[0]]
    up = torch.nn.ConvTranspose2d(w.shape[0], w.shape[1], 2, 2).double()
    up.weight.data, up.bias.data = torch.from_numpy(w.astype(np.float64)), torch.from_numpy(st[MK.PREDICTOR_KEYS[1]].astype(np.float64))
    net = torch.nn.Sequential(*mods, up, torch.nn.ReLU()).eval()
    with torch.no_grad():
        return net(torch.from_numpy(np.asarray(pooled, np.float64))).numpy()


@pytest.mark.parametrize("old", [False, True])
def test_mask_head_ref_against_modules(old):
    st = MK.generate_mask_head_state(16, (24, 8), 12, 5, seed=3, old=old, prefix="roi_heads." if old else "")
    g = np.random.default_rng(7)
    pooled = np.maximum(g.standard_normal((4, 16, 6, 6)), 0).astype(F32)
    got = MK.mask_head_ref(pooled, st)
    want = torch_mask_head(st, pooled)
    assert got.shape == want.shape == (4, 12, 12, 12)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    layers = MK.mask_head_ref(pooled, st, layers=True)
    assert [v.shape[1] for v in layers] == [24, 8, 12] and np.array_equal(layers[-1], got)


def test_predict_ref_against_the_full_1x1():
    """predict_ref against the sigmoid of the full 1x1 followed by maskrcnn_inference's gather"""
    t, labels, w, b = predict_case(64, 3, 7, 9)
    x = MK.panel_to_nchw(t)
    p, z = MK.predict_ref(x, labels, w, b, return_logits=True)
    full = torch.sigmoid(F.conv2d(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w.astype(np.float64))[:, :, None, None],
                                  torch.from_numpy(b.astype(np.float64)))).numpy()
    for k, l in enumerate(labels):
        if 1 <= l < 7:
            assert np.abs(p[k] - full[k, l]).max() <= 1e-14
        else:
            assert not p[k].any() and not z[k].any()
    assert set(labels[:5].tolist()) == {0, -1, 7, 6, 1}


def test_split_state_both_spellings():
    new = MK.generate_mask_head_state(64, (64, 128), 64, 5, seed=1)
    old = MK.generate_mask_head_state(64, (64, 128), 64, 5, seed=1, old=True, prefix="roi_heads.")
    assert "roi_heads.mask_head.mask_fcn2.weight" in old and "mask_head.1.0.weight" in new
    extra = {"roi_heads.box_head.fc6.weight": np.zeros(1, F32), "backbone.body.conv1.weight": np.zeros(1, F32)}
    for st in (new, old, {"roi_heads." + k: v for k, v in new.items()}):
        mine, rest = MK.split_state({**st, **extra})
        assert sorted(mine) == sorted(new) and sorted(rest) == sorted(extra)
        assert all(np.array_equal(mine[k], new[k]) for k in new)
    assert MK.layers_of(old) == (64, 128)
    assert sorted(MK.head_shapes(64, (64, 128), 64, 5)) == sorted(new)
    assert {k: v.shape for k, v in new.items()} == MK.head_shapes(64, (64, 128), 64, 5)


def test_split_detector_state_without_mask_keys_is_todays():
    st = {"backbone.body.conv1.weight": np.zeros((4, 3, 7, 7), F32), "backbone.fpn.inner_blocks.0.0.weight": np.zeros((8, 4, 1, 1), F32),
          "rpn.head.conv.0.0.weight": np.zeros((8, 8, 3, 3), F32), "roi_heads.box_head.fc6.weight": np.zeros((4, 8), F32)}
    got = D.split_detector_state(st)
    assert sorted(got) == ["backbone", "box_head", "neck", "rpn"]
    assert sorted(got["box_head"]) == ["box_head.fc6.weight"] and sorted(got["backbone"]) == ["conv1.weight"]
    st.update(MK.generate_mask_head_state(8, (8,), 8, 3, prefix="roi_heads."))
    with_mask = D.split_detector_state(st)
    assert sorted(with_mask) == ["backbone", "box_head", "mask_head", "neck", "rpn"]
    assert sorted(with_mask["mask_head"]) == sorted(MK.head_shapes(8, (8,), 8, 3))
    for k in got:
        assert sorted(with_mask[k]) == sorted(got[k])


def test_detection_rois_ref():
    boxes = np.arange(2 * 3 * 4, dtype=F32).reshape(2, 3, 4)
    labels = np.array([[1, -1, 4], [0, 2, -1]], np.int32)
    r = MK.detection_rois_ref(boxes, labels)
    assert r.shape == (6, 5) and r.dtype == F32
    assert r[:, 0].tolist() == [0, -1, 0, -1, 1, -1]
    assert np.array_equal(r[0, 1:], boxes[0, 0]) and np.array_equal(r[4, 1:], boxes[1, 1]) and not r[[1, 3, 5], 1:].any()
