"""The detector's launches AT the limits their refusals state, on the GPU: the inputs test_detector_limits_host.py built
and vetted, each through ONE call on views between guard bands -- outputs pre-filled with 0xA5 and checked written
everywhere, launch counts asserted -- against the numpy contract bit for bit.  No tolerance is new here: a decoded box
stays within test_rpn_host.decode_bound, a mask probability (its expf is not bit-defined) within test_mask_gpu.prob_bound
of float64 and bit for bit the same row's at another position, a head object within the bound of the neighbouring
test_object_against_float64.  The host file's conditions are asserted again on what the device returned, where its own
boxes or probabilities enter the reference.  profiles/detector_limits/README.md maps the cases to the paths they reach."""
import numpy as np
import pytest

import views as V
import resnet_c_amd as R
import test_detector_limits_host as H
from resnet_c_amd import _lib as L
from resnet_c_amd import keypoint as KP
from resnet_c_amd import mask as MK
from resnet_c_amd import rpn
from test_detect_gpu import check_contract, postprocess
from test_detect_gpu import record as record_detect
from test_dilation_gpu import bits, tol_f32
from test_fpn_gpu import SIZE, launches
from test_keypoint_gpu import run_predict as run_keypoint_predict
from test_keypoint_gpu import run_search
from test_keypoint_host import EDGE_SIZE, heat_bound, same_bits
from test_mask_gpu import prob_bound, run_paste
from test_mask_gpu import record as record_mask
from test_mask_gpu import run_predict as run_mask_predict
from test_rpn_gpu import assert_proposals, check_candidates, merge_call, nms_call, select_decode
from test_rpn_gpu import record as record_rpn

pytestmark = pytest.mark.gpu

F = np.float32


# =====================================================================================================================
# 1. NMS at 64 mask words
# =====================================================================================================================
@pytest.mark.parametrize("n", H.NMS_N)
def test_nms_at_64_words(n):
    case = H.nms_case(n)
    boxes = case["boxes"]
    for thr in H.NMS_THR:
        want = case["want"][thr]
        got = nms_call(boxes, thr, offs={"boxes": 4, "keep": 1} if thr == 0.5 else None)
        assert np.array_equal(got, want), f"n {n} threshold {thr}: {np.argwhere(got != want)[:8].tolist()}"
        record_rpn(f"nms limits n = {n} threshold {thr}: kept {want.sum(axis=1).tolist()}, in the last word "
                   f"{want[:, H.LAST_WORD:].sum(axis=1).tolist()} of {n - H.LAST_WORD}")
    for mask, want in ((case["valid"], case["want_valid"]), (case["last"], case["want_last"])):
        got = nms_call(boxes, 0.5, mask)
        assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    assert got[1, n - 1] and got[1].sum() == 1


# =====================================================================================================================
# 2. the RPN at A = 12, L = 5, pre = 4096
# =====================================================================================================================
@pytest.mark.parametrize("kind", sorted(H.RPN_KINDS))
def test_rpn_at_twelve_anchors_five_levels(kind):
    heads, base = H.rpn_case(12, kind)
    for pre in H.RPN_PRE:
        cand = select_decode(heads, base, H.RPN_IMAGE, pre, min_size=H.RPN_MIN_SIZE)
        err, ratio = check_candidates(cand, heads, base, H.RPN_IMAGE, pre, H.RPN_MIN_SIZE, -np.inf)
        record_rpn(f"rpn limits A = 12 ({kind}, k = {pre}): max |box - decode_f64| = {err:.3e}, {ratio:.3f} of the bound")
    merged = {}
    for post in H.RPN_POST:      # on the candidates of pre = 4096 the device returned
        merged[post] = rpn.nms_merge_ref(cand, post, H.RPN_THR)
        assert_proposals(merge_call(cand, post, H.RPN_THR), merged[post])
    valid, kept = H.rpn_conditions(cand, merged)
    record_rpn(f"rpn limits A = 12 ({kind}): {valid} valid candidates, {kept} survivors, counts {merged[4096]['count'].tolist()} "
               f"of post 4096, {merged[1000]['count'].tolist()} of post 1000")


@pytest.mark.parametrize("A", [1, 4])
def test_rpn_select_decode_at_other_anchor_counts(A):
    heads, base = H.rpn_case(A, "random")
    for pre in H.RPN_PRE:
        cand = select_decode(heads, base, H.RPN_IMAGE, pre, min_size=H.RPN_MIN_SIZE)
        err, ratio = check_candidates(cand, heads, base, H.RPN_IMAGE, pre, H.RPN_MIN_SIZE, -np.inf)
        record_rpn(f"rpn limits A = {A} (P = {heads[0].shape[3]}, k = {pre}): max |box - decode_f64| = {err:.3e}, {ratio:.3f} of the bound")


# =====================================================================================================================
# 3. box post-processing at C = 1024, and 4. one class over all four slots
# =====================================================================================================================
@pytest.mark.parametrize("seed,B,Rn,C,st,Dn", H.DETECT_WIDE)
def test_detect_at_1024_classes(seed, B, Rn, C, st, Dn):
    head, rois = H.detect_limit_case(seed, B, Rn, C)
    got = postprocess(head, rois, B, C, Dn, st=st)
    want, worst = check_contract(got, head, rois, B, C, Dn, st=st)
    total = H.wide_conditions(got, B, Rn, C, Dn)
    assert (got["count"] == Dn).all() and (Rn != 64 or total[0] > 4096), (total.tolist(), got["count"].tolist())
    record_detect(f"detect limits C = {C} R = {Rn} D = {Dn}: {int(got['valid'].sum())} valid candidates, survivors {total.tolist()}; "
                  f"box error {worst:.3f} of the bound")


@pytest.mark.parametrize("seed,B,Rn,C,st,Dn", H.DETECT_DEEP)
def test_detect_one_class_over_every_slot(seed, B, Rn, C, st, Dn):
    head, rois = H.detect_limit_case(seed, B, Rn, C)
    got = postprocess(head, rois, B, C, Dn, st=st)
    want, worst = check_contract(got, head, rois, B, C, Dn, st=st)
    nv, nk = H.deep_conditions(got, C)
    assert got["count"][0] == min(sum(nk), Dn)
    record_detect(f"detect limits R = {Rn} C = {C}: valid per class {nv}, survivors {nk}; box error {worst:.3f} of the bound")


# =====================================================================================================================
# 5. the mask predictor, one limit at a time
# =====================================================================================================================
def check_predict(got, t, labels, w, b, Cr, C):
    """dead rows zeros, live rows within prob_bound of float64; returns (largest error, its largest share of the bound)"""
    p64, z64 = MK.predict_ref(MK.panel_to_nchw(t), labels, w, b, return_logits=True)
    ok = (labels >= 1) & (labels < C)
    assert not got[~ok].any() and got[ok].min() > 0
    bound = prob_bound(p64[ok], tol_f32(z64[ok], Cr))
    err = np.abs(got[ok].astype(np.float64) - p64[ok])
    assert (err <= bound).all(), float((err / bound).max())
    return float(err.max()), float((err / bound).max())


@pytest.mark.parametrize("Cr,M,C", H.PREDICT_SHAPES)
def test_mask_predict_one_limit_at_a_time(Cr, M, C):
    t, labels, w, b = H.predict_limit_case(Cr, M, C)
    got = run_mask_predict(t, labels, w, b, C)
    err, share = check_predict(got, t, labels, w, b, Cr, C)
    record_mask(f"mask_predict limits Cr {Cr} M {M} C {C}: max error {err:.3e}, largest share of the bound {share:.3e}")
    # a row's bits do not depend on its position: the same rows in reverse order
    again = run_mask_predict(t[::-1], labels[::-1], w, b, C)
    assert np.array_equal(bits(again[::-1]), bits(got))


# =====================================================================================================================
# 6. the paste at Mo = 64
# =====================================================================================================================
@pytest.mark.parametrize("size", H.PASTE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_paste_at_64(size):
    H_, W = size
    probs, boxes, labels, want = H.paste_limit_case(H_, W)
    want_bits = (want > F(0.5)).astype(np.uint8)
    masks, got_bits = run_paste(probs, boxes, labels, H_, W)
    assert np.array_equal(bits(masks), bits(want)), np.flatnonzero(bits(masks) != bits(want))[:8]
    assert np.array_equal(got_bits, want_bits)
    only_m, none = run_paste(probs, boxes, labels, H_, W, bits_=False)
    none2, only_b = run_paste(probs, boxes, labels, H_, W, masks=False)
    assert none is None and none2 is None and np.array_equal(bits(only_m), bits(want)) and np.array_equal(only_b, want_bits)


# =====================================================================================================================
# 7. more rows than grid y
# =====================================================================================================================
def test_mask_predict_more_rows_than_grid_y():
    t, labels, w, b = H.rows_predict_case()
    period = run_mask_predict(t, labels, w, b, 2)
    err, share = check_predict(period, t, labels, w, b, 64, 2)
    got = run_mask_predict(H.tile_rows(t), H.tile_rows(labels), w, b, 2)
    want = H.tile_rows(period)
    wrong = np.flatnonzero((bits(got) != bits(want)).reshape(H.ROWS_K, -1).any(axis=1))
    assert wrong.size == 0, f"{wrong.size} rows differ from the period's bits, the first {wrong[:8].tolist()}"
    record_mask(f"mask_predict limits K = {H.ROWS_K}: every row the period's bits; max error {err:.3e}, {share:.3e} of the bound")


def test_paste_more_rows_than_grid_y():
    probs, boxes, labels, want = H.rows_paste_case()
    masks, got_bits = run_paste(H.tile_rows(probs), H.tile_rows(boxes), H.tile_rows(labels), 3, 5)
    want = H.tile_rows(want)
    wrong = np.flatnonzero((bits(masks) != bits(want)).reshape(H.ROWS_K, -1).any(axis=1))
    assert wrong.size == 0, f"{wrong.size} rows differ, the first {wrong[:8].tolist()}"
    assert np.array_equal(got_bits, (want > F(0.5)).astype(np.uint8))


def test_search_more_rows_than_grid_y():
    heat, boxes, labels, (want_k, want_s) = H.rows_search_case()
    kps, scores = run_search(H.tile_rows(heat), H.tile_rows(boxes), H.tile_rows(labels), EDGE_SIZE)
    want_k, want_s = H.tile_rows(want_k), H.tile_rows(want_s)
    wrong = np.flatnonzero((bits(kps) != bits(want_k)).reshape(H.ROWS_K, -1).any(axis=1) | (bits(scores) != bits(want_s)).reshape(H.ROWS_K, -1).any(axis=1))
    assert wrong.size == 0, f"{wrong.size} rows differ, the first {wrong[:8].tolist()}"


# =====================================================================================================================
# 8. the keypoint head at its limits
# =====================================================================================================================
@pytest.mark.parametrize("Kp", H.SEARCH_KP)
def test_search_at_64(Kp):
    heat, boxes, labels, (want_k, want_s) = H.search_limit_case(Kp)
    kps, scores = run_search(heat, boxes, labels, EDGE_SIZE)
    assert same_bits(kps, want_k) and same_bits(scores, want_s)


def test_keypoint_predict_at_16_and_256():
    t, bias, boxes, labels = H.keypoint_predict_limit_case()
    heat, kps, scores = run_keypoint_predict(t, bias, boxes, labels, EDGE_SIZE)
    assert same_bits(heat, KP.heatmaps_ref(t, bias)), "heat is not heatmaps_ref's bits"
    want_k, want_s = KP.heatmaps_to_keypoints_ref(heat, boxes, EDGE_SIZE, labels)
    assert same_bits(kps, want_k) and same_bits(scores, want_s)
    assert not kps[[3, 4]].any() and (kps[[0, 1, 2, 5], :, 2] == 1).all()
    _, only_k, only_s = run_keypoint_predict(t, bias, boxes, labels, EDGE_SIZE, heat=False)     # no heat map reaches memory
    assert same_bits(only_k, kps) and same_bits(only_s, scores)


def test_search_in_an_8192_image():
    heat, boxes, (want_k, want_s) = H.wide_search_case()
    kps, scores = run_search(heat, boxes, None, H.WIDE_SIZE)
    assert same_bits(kps, want_k) and same_bits(scores, want_s)


# =====================================================================================================================
# 9. towers with unequal widths
# =====================================================================================================================
def l1(w):
    return np.abs(w.reshape(w.shape[0], -1)).sum(axis=1).max()


def tower_alone(st, stem, pooled, layers, panel_w, panel_shift, panel_relu):
    """the tower as stand-alone launches: every 3x3 (bias, ReLU) and the 1x1 panel through rn_conv2d_nhwc_forward_dt on
    views between guard bands, each reading the previous one's host copy: the panel's output [K, M, M, panel]"""
    x = pooled
    for i in range(len(layers)):
        x = V.run_conv_dt(x, st[stem(i) + "weight"], 1, 1, None, st[stem(i) + "bias"], None, True, L.RN_DTYPE_F32, L.RN_DTYPE_F32)
    w = np.ascontiguousarray(panel_w, F).reshape(panel_w.shape[0], -1, 1, 1)
    t = V.run_conv_dt(x, w, 1, 0, None, panel_shift, None, panel_relu, L.RN_DTYPE_F32, L.RN_DTYPE_F32)
    return np.ascontiguousarray(t.transpose(0, 2, 3, 1))


def tower_error(st, stem, outs, in_channels, layers):
    """test_object_against_float64's accumulation: (the bound of the last 3x3's output, its channels)"""
    e, cin = 0.0, in_channels
    for i, c in enumerate(layers):
        e = e * l1(st[stem(i) + "weight"].astype(np.float64)) + tol_f32(outs[i], 9 * cin)
        cin = c
    return e, cin


@pytest.mark.parametrize("in_channels,layers", H.TOWERS)
def test_mask_head_with_unequal_widths(in_channels, layers):
    """test_mask_gpu.test_object_against_float64's statement and bound; two forwards, the second of more rows.  That bound
    grows by a layer's largest L1 norm per layer and says little behind eight of them, so the object is also held, bit for
    bit, to the same launches made one by one on views: the scratch tensors the object reads at several widths hold what a
    tensor of exactly that width holds."""
    st, _, pooled, labels, _ = H.tower_case(in_channels, layers)
    C, Cr = H.TOWER_C, H.TOWER_CR
    mh = R.MaskHead(in_channels, layers, Cr, C, {"roi_heads." + k: v for k, v in st.items()}, resolution=H.TOWER_M)
    mh.poison = True
    try:
        for K in H.TOWER_ROWS:
            x, lab = pooled[:K], labels[:K]
            n0 = launches()
            out = mh(np.ascontiguousarray(x.transpose(0, 2, 3, 1)), lab)
            n = len(layers) + 1
            assert n + 1 <= launches() - n0 <= 2 * n + 1, "n_layers + 1 contractions of one or two launches and the predict"
            probs = out["mask_probs"][0]
            V.check_written(np.ascontiguousarray(probs).view(np.uint8), 4, "mask_probs")
            outs = MK.mask_head_ref(x, st, layers=True)
            e, cin = tower_error(st, lambda i: f"mask_head.{i}.0.", outs, in_channels, layers)
            rows, _ = MK.deconv_panel(st[MK.PREDICTOR_KEYS[0]].astype(np.float64), st[MK.PREDICTOR_KEYS[1]])
            e_t = e * l1(rows) + tol_f32(outs[-1], cin)
            wl = st[MK.PREDICTOR_KEYS[2]].reshape(C, Cr).astype(np.float64)
            p64, z64 = MK.predict_ref(outs[-1], lab, wl, st[MK.PREDICTOR_KEYS[3]], return_logits=True)
            ok = lab >= 1
            e_z = (e_t * np.abs(wl[np.clip(lab, 0, C - 1)]).sum(axis=1))[:, None, None] + tol_f32(z64[ok], Cr)
            bound = prob_bound(p64[ok], e_z[ok])
            err = np.abs(probs[ok].astype(np.float64) - p64[ok])
            assert (err <= bound).all(), float((err / bound).max())
            assert not probs[~ok].any() and 0 < probs[ok].min() and probs[ok].max() < 1
            record_mask(f"mask head limits in {in_channels} layers {layers} K {K}: prob error {err.max():.3e}, largest share of the "
                        f"bound {float((err / bound).max()):.3e}")
            rows32, shift32 = MK.deconv_panel(st[MK.PREDICTOR_KEYS[0]], st[MK.PREDICTOR_KEYS[1]])
            t = tower_alone(st, lambda i: f"mask_head.{i}.0.", x, layers, rows32, shift32, True)
            alone = run_mask_predict(t, lab, st[MK.PREDICTOR_KEYS[2]].reshape(C, Cr), st[MK.PREDICTOR_KEYS[3]], C)
            assert np.array_equal(bits(alone), bits(probs)), "the object's bits are not the stand-alone launches'"
    finally:
        mh.close()


@pytest.mark.parametrize("in_channels,layers", H.TOWERS)
def test_keypoint_head_with_unequal_widths(in_channels, layers):
    """test_keypoint_gpu.test_object_against_float64's statement and bound; two forwards, the second of more rows; and,
    as for the mask head, bit for bit the same launches made one by one on views"""
    _, st, pooled, labels, boxes = H.tower_case(in_channels, layers)
    kh = R.KeypointHead(in_channels, layers, H.TOWER_KP, {"roi_heads." + k: v for k, v in st.items()}, resolution=H.TOWER_M)
    kh.poison = True
    try:
        for K in H.TOWER_ROWS:
            x, lab, bx = pooled[:K], labels[:K], boxes[:K]
            n0 = launches()
            out = kh(np.ascontiguousarray(x.transpose(0, 2, 3, 1)), lab, bx, SIZE, keypoints=("keypoints", "heatmaps"))
            n = len(layers) + 1
            assert n + 1 <= launches() - n0 <= 2 * n + 1, "n_layers + 1 contractions of one or two launches and ONE predict launch"
            for k, v in out.items():
                V.check_written(np.ascontiguousarray(v).view(np.uint8), v.dtype.itemsize, k)
            heat = out["keypoint_heatmaps"][0]
            outs = KP.keypoint_head_ref(x, st, layers=True)
            e, cin = tower_error(st, lambda i: f"keypoint_head.{2 * i}.", outs, in_channels, layers)
            rows = KP.deconv_panel(st[KP.PREDICTOR_KEYS[0]].astype(np.float64))
            t64 = np.einsum("kchw,oc->khwo", outs[len(layers) - 1], rows, optimize=True)
            e_t = e * l1(rows) + tol_f32(t64, cin)
            bound = 4 * e_t + heat_bound(t64, st[KP.PREDICTOR_KEYS[1]])
            err = np.abs(heat.astype(np.float64) - outs[-1])
            assert (err <= bound).all(), float((err / bound).max())
            want_k, want_s = KP.heatmaps_to_keypoints_ref(heat, bx, SIZE, lab)
            assert same_bits(out["keypoints"][0], want_k) and same_bits(out["keypoints_scores"][0], want_s)
            assert not out["keypoints"][0][2].any() and (out["keypoints"][0][[0, 1, 3], :, 2] == 1).all()
            record_mask(f"keypoint head limits in {in_channels} layers {layers} K {K}: heat error {err.max():.3e}, largest share of the "
                        f"bound {float((err / bound).max()):.3e}")
            t = tower_alone(st, lambda i: f"keypoint_head.{2 * i}.", x, layers, KP.deconv_panel(st[KP.PREDICTOR_KEYS[0]]), None, False)
            alone_h, alone_k, alone_s = run_keypoint_predict(t, st[KP.PREDICTOR_KEYS[1]], bx, lab, SIZE)
            assert same_bits(alone_h, heat), "the object's bits are not the stand-alone launches'"
            assert same_bits(alone_k, out["keypoints"][0]) and same_bits(alone_s, out["keypoints_scores"][0])
    finally:
        kh.close()
