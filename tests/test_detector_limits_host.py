"""The detector's launches AT the limits their refusals state, on the host: every input test_detector_limits_gpu.py runs is
built here -- each generator call, seed and shape in one place, cached, so the GPU file runs what this file vetted -- and
the numpy contract alone is run on it.  What is asserted are the CONDITIONS: properties of the reference that prove the
input reaches the path its case exists for (the last mask word, every wave's class count, slot 3, the second trip of a
block, ...).  No GPU.  profiles/detector_limits/README.md lists which case is there for which path."""
import functools

import numpy as np
import pytest

from resnet_c_amd import detection as D
from resnet_c_amd import keypoint as KP
from resnet_c_amd import mask as MK
from resnet_c_amd import ops, rpn
from test_detect_host import IMAGE, detect_case
from test_keypoint_host import EDGE_OUT, EDGE_SIZE, edge_boxes, gaussian_heat, panel_case, same_bits
from test_mask_host import paste_boxes, paste_probs, predict_case
from test_rpn_host import chain_cases, clustered_boxes, random_heads

F = np.float32
GRID_Y = 65535            # the launches' cap on gridDim.y: row k of a longer call is block k % GRID_Y's second trip
LAST_WORD = 4032          # rank 4032 is bit 0 of mask word 63, the last one a segment of 4096 has


def cached(fn):
    """one computation per argument tuple for both files; the arrays are shared and never written to"""
    return functools.lru_cache(maxsize=None)(fn)


# =====================================================================================================================
# 1. NMS at 64 mask words
# =====================================================================================================================
NMS_N = (4033, 4095, 4096)
NMS_THR = (0.5, 0.7)


@cached
def nms_case(n):
    """boxes [2, n, 4]; want[thr] the reference's keep; at 0.5 the two `valid` variants of
    test_nms_bit_for_bit_on_clustered_boxes in one mask, and a mask that leaves segment 1 its last rank alone (the one
    rank a last word of 4033 boxes has: there it survives for certain)"""
    boxes = np.stack([clustered_boxes(n), clustered_boxes(n, seed=n + 7919)])
    valid = np.ones((2, n), np.uint8)
    valid[0, 0] = 0
    valid[1, :] = 0
    last = valid.copy()
    last[1, n - 1] = 1
    return {"boxes": boxes, "want": {thr: ops.nms_segments_ref(boxes, thr) for thr in NMS_THR}, "valid": valid,
            "want_valid": ops.nms_segments_ref(boxes, 0.5, valid), "last": last, "want_last": ops.nms_segments_ref(boxes, 0.5, last)}


def last_word_both_ways(keep, live):
    """among the ranks of the last mask word that can survive at all: one that does and one that does not"""
    tail, ok = np.asarray(keep).astype(bool)[LAST_WORD:], np.asarray(live).astype(bool)[LAST_WORD:]
    return bool((tail & ok).any() and (~tail & ok).any())


@pytest.mark.parametrize("n", NMS_N)
def test_nms_inputs_reach_the_last_word(n):
    case = nms_case(n)
    assert (n + 63) // 64 == 64, "64 mask words: every lane of the scan holds one"
    kept_tail = gone_tail = 0
    for thr in NMS_THR:
        want = case["want"][thr]
        for s in range(2):
            share = want[s].sum() / n
            assert 0.05 <= share <= 0.60, (n, thr, s, share)
            kept_tail += int(want[s, LAST_WORD:].sum())
            gone_tail += int((~want[s, LAST_WORD:]).sum())
        assert chain_cases(case["boxes"][0], want[0], thr) >= 1, (n, thr)
    wv, wl = case["want_valid"], case["want_last"]
    assert not wv[0, 0] and not wv[1].any() and np.array_equal(wl[0], wv[0])
    assert wl[1].sum() == 1 and wl[1, n - 1], "the last rank alone: bit n - 1 - 4032 of word 63 survives"
    # over the segments and thresholds of a case the last word holds a survivor and a suppressed box; the one rank that
    # 4033 boxes have there is suppressed in every draw, so its survivor is the last-rank mask's
    assert gone_tail >= 1 and kept_tail >= (1 if n - LAST_WORD >= 63 else 0), (n, kept_tail, gone_tail)
    assert kept_tail + int(wl[1, LAST_WORD:].sum()) >= 1


# =====================================================================================================================
# 2. the RPN at A = 12, L = 5, pre = 4096
# =====================================================================================================================
RPN_IMAGE = (152, 152)
RPN_SIZES = [(38, 38), (19, 19), (8, 8), (4, 4), (2, 2)]     # strides 4, 8, 19, 38, 76: all whole
RPN_B, RPN_MIN_SIZE, RPN_THR = 2, 12.0, 0.7
RPN_AG = {12: rpn.AnchorGenerator(((16, 32, 64, 128),) * 5, (0.5, 1.0, 2.0)),
          4: rpn.AnchorGenerator(((16, 32, 64, 128),) * 5, (1.0,)),
          1: rpn.AnchorGenerator(((32,),) * 5, (1.0,))}
RPN_KINDS = {"random": 21, "quantised": 22}
RPN_PRE = (100, 4096)
RPN_POST = (1000, 4096)


@cached
def rpn_case(A, kind):
    """(heads of five levels [2, h, w, P], base anchors [5, A, 4])"""
    g = np.random.default_rng(RPN_KINDS[kind] + 100 * A)
    return random_heads(g, RPN_B, RPN_SIZES, A, kind), RPN_AG[A].base_anchors()


def rpn_conditions(cand, merged):
    """on candidates of pre = 4096 and the reference's merges {post: nms_merge_ref}: two full levels, whose last mask word
    holds a survivor and a suppressed candidate; post = 4096 is not filled, post = 1000 is"""
    full = [l for l in range(5) if (cand["count"][:, l] == 4096).all()]
    assert len(full) >= 2, cand["count"].tolist()
    keep = merged[4096]["cand_keep"]
    for b in range(RPN_B):
        for l in full:
            assert last_word_both_ways(keep[b, l], cand["valid"][b, l]), (b, l)
    assert (merged[4096]["count"] < 4096).all() and (merged[4096]["count"] > 1000).all(), merged[4096]["count"].tolist()
    assert (merged[1000]["count"] == 1000).all()
    valid, kept = int(cand["valid"].sum()), int(keep.sum())
    assert 0.05 * valid <= kept <= 0.60 * valid, (valid, kept)
    return valid, kept


@pytest.mark.parametrize("kind", sorted(RPN_KINDS))
def test_rpn_inputs_fill_two_levels_and_the_merge(kind):
    heads, base = rpn_case(12, kind)
    assert base.shape == (5, 12, 4) and heads[0].shape[3] == 60 == rpn.head_channels(12), "P = 60: no pad column"
    assert all(RPN_IMAGE[0] % h == 0 and RPN_IMAGE[1] % w == 0 for h, w in RPN_SIZES)
    cand = rpn.select_decode_ref(heads, base, RPN_IMAGE, 4096, RPN_MIN_SIZE, -np.inf)
    assert cand["count"][0].tolist() == [4096, 4096, 768, 192, 48]
    assert cand["valid"].any() and not cand["valid"][cand["index"] >= 0].all(), "both outcomes of the validity rule"
    a = cand["index"][cand["index"] >= 0] % 12
    assert set(a.tolist()) == set(range(12)), "every base anchor, a >= 3 included, is selected somewhere"
    merged = {post: rpn.nms_merge_ref(cand, post, RPN_THR) for post in RPN_POST}
    valid, kept = rpn_conditions(cand, merged)
    assert 5 * 4096 > 4096 and int(cand["count"][0].sum()) > 4096, "the merge selects among more keys than a selection holds"
    print(f"\n  rpn limits ({kind}): {valid} valid candidates, {kept} survivors, counts {merged[4096]['count'].tolist()}")


@pytest.mark.parametrize("A,P", [(1, 8), (4, 20)])
def test_rpn_other_anchor_counts(A, P):
    heads, base = rpn_case(A, "random")
    assert rpn.head_channels(A) == P == heads[0].shape[3] and (5 * A == P) == (A == 4)
    for pre in RPN_PRE:
        cand = rpn.select_decode_ref(heads, base, RPN_IMAGE, pre, RPN_MIN_SIZE, -np.inf)
        assert cand["count"][0].tolist() == [min(pre, h * w * A) for h, w in RPN_SIZES]
        assert cand["valid"].any()


# =====================================================================================================================
# 3. box post-processing at C = 1024, and 4. one class over all four slots
# =====================================================================================================================
# (seed, B, R, C, score threshold, detections per image)
DETECT_WIDE = [(8, 2, 16, 1024, 0.001, 100), (8, 2, 16, 1024, 0.001, 1024), (9, 1, 64, 1024, 0.0005, 1024)]
DETECT_DEEP = [(8, 1, 4096, 2, -1.0, 1024), (8, 1, 4096, 3, 0.05, 1024)]


@cached
def detect_limit_case(seed, B, Rn, C):
    return detect_case(seed, B, Rn, C)


def wide_conditions(out, B, Rn, C, Dn):
    """on the nine outputs (the reference's, or the device's held to the reference): survivors in every wave of the merge's
    class-count prefix sum; returns the survivors per image"""
    keep = np.asarray(out["keep"]).astype(bool).reshape(B, Rn, C)
    per_class = keep.sum(axis=1)[:, 1:]                      # [B, C - 1]: thread t of the merge block holds class t + 1
    for b in range(B):
        for w in range(16):
            assert per_class[b, 64 * w:64 * (w + 1)].any(), f"image {b}: wave {w} of the prefix sum holds no survivor"
        for w in range(1, 8):
            assert per_class[b, 128 * w:].any(), f"image {b}: no survivor beyond class index {128 * w}"
    total = per_class.sum(axis=1)
    assert (np.asarray(out["count"]) == np.minimum(total, Dn)).all()
    return total


@pytest.mark.parametrize("seed,B,Rn,C,st,Dn", DETECT_WIDE)
def test_detect_inputs_reach_every_wave_of_the_prefix_sum(seed, B, Rn, C, st, Dn):
    head, rois = detect_limit_case(seed, B, Rn, C)
    out = D.postprocess_ref(head, rois, B, C, IMAGE, st, 0.5, Dn)
    total = wide_conditions(out, B, Rn, C, Dn)
    assert C - 1 > 128 and (out["count"] == Dn).all(), (total.tolist(), out["count"].tolist())
    if Rn == 64:
        assert total[0] > 4096, "more survivors than a selection holds"
    print(f"\n  detect limits C = {C} R = {Rn} D = {Dn}: survivors {total.tolist()}, "
          f"{int((out['keep'].reshape(B, Rn, C).sum(axis=1)[:, 1:] > 0).sum(axis=1).min())} of {C - 1} classes with survivors")


def deep_conditions(out, C):
    """one class with more than 3072 valid candidates (its chunks are owned by slot 3 too) or, with three classes, every
    class with more than 2048 (slot 2); survivors between 5 % and 60 % of the valid candidates"""
    valid, keep = np.asarray(out["valid"]).astype(bool), np.asarray(out["keep"]).astype(bool)
    nv, nk = valid.sum(axis=0)[1:], keep.sum(axis=0)[1:]
    assert (nv > 3072).any() if C == 2 else (nv > 2048).all(), nv.tolist()
    assert (0.05 * nv <= nk).all() and (nk <= 0.60 * nv).all(), (nv.tolist(), nk.tolist())
    return nv.tolist(), nk.tolist()


@pytest.mark.parametrize("seed,B,Rn,C,st,Dn", DETECT_DEEP)
def test_detect_inputs_fill_every_slot_of_a_class(seed, B, Rn, C, st, Dn):
    head, rois = detect_limit_case(seed, B, Rn, C)
    out = D.postprocess_ref(head, rois, B, C, IMAGE, st, 0.5, Dn)
    nv, nk = deep_conditions(out, C)
    print(f"\n  detect limits R = 4096 C = {C}: valid per class {nv}, survivors {nk}")


def test_both_detect_depths_are_covered():
    """over the two deep cases: one class above 3072 valid candidates and another above 2048"""
    tops = []
    for seed, B, Rn, C, st, Dn in DETECT_DEEP:
        head, rois = detect_limit_case(seed, B, Rn, C)
        tops += D.score_decode_ref(head, rois, B, C, IMAGE, st)["valid"].sum(axis=0)[1:].tolist()
    tops = sorted(tops)
    assert tops[-1] > 3072 and tops[-2] > 2048, tops


# =====================================================================================================================
# 5. the mask predictor, one limit at a time
# =====================================================================================================================
PREDICT_SHAPES = [(1024, 2, 5), (64, 32, 2), (64, 1, 1024), (1024, 1, 1024)]     # (Cr, M, C)
PREDICT_K = 8


def predict_labels(C):
    """1, C - 1, 0, -1, a value at C, one far above it, then two more live rows"""
    return np.array([1, C - 1, 0, -1, C, C + 1000, max(1, C // 2), max(1, C - 2)], np.int32)


@cached
def predict_limit_case(Cr, M, C):
    t, _, w, b = predict_case(Cr, M, C, PREDICT_K)
    return t, predict_labels(C), w, b


@pytest.mark.parametrize("Cr,M,C", PREDICT_SHAPES)
def test_predict_inputs(Cr, M, C):
    t, labels, w, b = predict_limit_case(Cr, M, C)
    assert t.shape == (PREDICT_K, M, M, 4 * Cr) and w.shape == (C, Cr) and t.nbytes <= 70e6
    assert {1, C - 1, 0, -1, C} <= set(labels.tolist()) and labels.max() > C
    assert Cr == 1024 or M == 32 or C == 1024
    if Cr == 1024:
        assert Cr // 4 == 256 and Cr // 4 // 16 > 1, "the whole weight row of LDS; more than one trip per lane group"
    p64 = MK.predict_ref(MK.panel_to_nchw(t), labels, w, b)
    ok = (labels >= 1) & (labels < C)
    assert ok.sum() == 4 and not p64[~ok].any() and p64[ok].min() > 0
    assert p64[ok].min() < 0.2 and p64[ok].max() > 0.8, "the probabilities spread over (0, 1)"
    if C > 2:   # the rows of labels 1 and C - 1 read different weight rows, and that shows
        other = MK.predict_ref(MK.panel_to_nchw(t[1:2]), labels[:1], w, b)
        assert np.abs(other - p64[1:2]).max() > 1e-3


# =====================================================================================================================
# 6. the paste at Mo = 64
# =====================================================================================================================
PASTE_SIZES = [(96, 131), (5, 3)]
PASTE_SPAN = 8192      # elements of a plane one block pastes


@cached
def paste_limit_case(H, W, Mo=64):
    """test_mask_gpu.paste_case's rows: the host test's boxes, then a label of -1, a NaN and an infinity"""
    boxes = np.concatenate([paste_boxes(H, W), np.array([[1, 1, W - 1, H - 1], [1, np.nan, W - 1, H - 1], [0, 0, np.inf, H]], F)])
    labels = np.ones(boxes.shape[0], np.int32)
    labels[-3], labels[2] = -1, 7
    probs = paste_probs(boxes.shape[0], Mo, seed=H)
    return probs, boxes, labels, MK.paste_masks_ref(probs, boxes, (H, W), labels)


@pytest.mark.parametrize("size", PASTE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_paste_inputs(size):
    H, W = size
    probs, boxes, labels, want = paste_limit_case(H, W)
    assert probs.shape[1:] == (64, 64), "the largest padded map: 66 x 66"
    assert want.any() and not want[-3:].any() and not want[10].any()
    b = want > F(0.5)
    assert b.any() and not b.all()
    if size == (96, 131):
        assert H * W > PASTE_SPAN and W % 4, "more than one block to a plane, an odd width"
        assert want[6].reshape(-1)[PASTE_SPAN:].any(), "the second block of a plane pastes something"


# =====================================================================================================================
# 7. more rows than grid y
# =====================================================================================================================
ROWS_K = GRID_Y + 2


def second_trips(period):
    """(row of the period a block's first trip reads, row its second trip reads) for the blocks that make two trips"""
    return [(y % period, (y + GRID_Y) % period) for y in range(ROWS_K - GRID_Y)]


def tile_rows(a, K=ROWS_K):
    a = np.asarray(a)
    return np.ascontiguousarray(np.resize(a, (K,) + a.shape[1:]))   # np.resize repeats whole rows in order


@cached
def rows_predict_case():
    """(Cr, M, C) = (64, 1, 2): a period of 8 rows.  Row 0 is live and row 7 dead with weight row 0, row 1 dead and row 0
    live: a block that starts its second row's weight row before every wave finished the first, either way round, shows"""
    t, _, w, b = predict_case(64, 1, 2, 8, seed=7)
    return t, np.array([1, 0, 1, -1, 2, 1, 1, 0], np.int32), w, b


@cached
def rows_paste_case():
    """Mo = 2 in a 3 x 5 image: eight of the paste rows"""
    H, W = 3, 5
    boxes = paste_boxes(H, W)[[6, 2, 0, 1, 3, 7, 8, 9]]
    labels = np.array([1, 1, 1, 0, 1, 1, 1, 1], np.int32)
    probs = paste_probs(8, 2, seed=65537)
    return probs, boxes, labels, MK.paste_masks_ref(probs, boxes, (H, W), labels)


@cached
def rows_search_case():
    """S = 4, Kp = 1: the twelve edge rows"""
    boxes, labels, _ = edge_boxes()
    heat = gaussian_heat(len(boxes), 1, 4, seed=65537)
    return heat, boxes, labels, KP.heatmaps_to_keypoints_ref(heat, boxes, EDGE_SIZE, labels)


def test_row_periods_put_another_row_on_the_second_trip():
    assert ROWS_K == 65537 and len(second_trips(8)) == 2
    for period in (8, 12):
        assert GRID_Y % period != 0
        assert all(a != b for a, b in second_trips(period)), second_trips(period)
    assert np.array_equal(tile_rows(np.arange(8))[[0, 7, 8, 65535, 65536]], [0, 7, 0, 7, 0])
    # the predictor: the two rows of a block differ in liveness, so in the weight row they stage and in their output
    t, labels, w, b = rows_predict_case()
    p64 = MK.predict_ref(MK.panel_to_nchw(t), labels, w, b)
    assert t.shape == (8, 1, 1, 256) and tile_rows(t).nbytes <= 70e6
    for first, second in second_trips(8):
        assert (labels[first] == 1) != (labels[second] == 1) and p64[first].any() != p64[second].any()
    # the paste: both rows of a block paste something, and not the same
    probs, boxes, plabels, want = rows_paste_case()
    for first, second in second_trips(8):
        assert want[first].any() and want[second].any() and not np.array_equal(want[first], want[second])
    assert not want[3].any()
    # the search: both rows of a block are live and answer differently
    heat, eboxes, elabels, (kps, scores) = rows_search_case()
    for first, second in second_trips(12):
        assert first not in EDGE_OUT and second not in EDGE_OUT
        assert not same_bits(kps[first], kps[second]) and not same_bits(scores[first], scores[second])


# =====================================================================================================================
# 8. the keypoint head at its limits
# =====================================================================================================================
SEARCH_KP = (1, 256)
PREDICT_ROWS = (1, 2, 4, 5, 9, 11)     # of edge_boxes: integer sides, shrinking, 300 x 200, a NaN, label 0, fractional
WIDE_BOXES = np.array([[0.0, 0.0, 8192.0, 3.0], [0.0, 0.0, 3.0, 8192.0]], F)
WIDE_SIZE = (8192, 8192)


@cached
def search_limit_case(Kp, S=64):
    """test_keypoint_gpu.edge_case(S, Kp) and the contract's answer"""
    boxes, labels, _ = edge_boxes()
    heat = gaussian_heat(len(boxes), Kp, S, seed=S + Kp)
    if Kp >= 3:
        heat[:, 1] = 0.0
        heat[:, 2, 0, 0] = np.nan
    return heat, boxes, labels, KP.heatmaps_to_keypoints_ref(heat, boxes, EDGE_SIZE, labels)


@cached
def keypoint_predict_limit_case():
    boxes, labels, _ = edge_boxes()
    rows = list(PREDICT_ROWS)
    t, bias = panel_case(256, 16, len(rows), seed=5)
    return t, bias, boxes[rows], labels[rows]


@cached
def wide_search_case():
    heat = gaussian_heat(2, 1, 64, seed=8192)
    return heat, WIDE_BOXES, KP.heatmaps_to_keypoints_ref(heat, WIDE_BOXES, WIDE_SIZE)


@pytest.mark.parametrize("Kp", SEARCH_KP)
def test_search_inputs_fill_both_lds_maps(Kp):
    heat, boxes, labels, (kps, scores) = search_limit_case(Kp)
    assert heat.shape == (12, Kp, 64, 64) and heat.nbytes <= 70e6
    w, h, Wr, Hr, live = KP.box_sizes_ref(boxes, EDGE_SIZE, labels)
    assert (Wr[live] >= 128).any() and (Hr[live] >= 64).any(), "a whole chunk of 128 columns over all 64 rows of the row values"
    assert [k for k in range(12) if not live[k]] == list(EDGE_OUT) and not kps[list(EDGE_OUT)].any()
    assert np.all(kps[live][..., 2] == 1.0)
    # the last element of the map is read: a peak in the map's last corner is found there
    corner = np.full((1, 1, 64, 64), -3.0, F)
    corner[0, 0, 63, 63] = 5.0
    k, s = KP.heatmaps_to_keypoints_ref(corner, np.array([[0, 0, 64, 64]], F), EDGE_SIZE)
    assert k[0, 0, 0] == 63.5 and k[0, 0, 1] == 63.5 and s[0, 0] == 5.0


def test_keypoint_predict_inputs():
    t, bias, boxes, labels = keypoint_predict_limit_case()
    K = len(PREDICT_ROWS)
    assert t.shape == (K, 16, 16, 16 * 256) and t.nbytes <= 64e6 and bias.shape == (256,)
    assert 16 * 16 * 16 + 32 * 32 <= 64 * 128, "the panel's tile and the low-resolution map fit the row values' LDS"
    heat = KP.heatmaps_ref(t[:1, :, :, :32], bias[:2])
    assert heat.shape == (1, 2, 64, 64) and np.isfinite(heat).all() and heat.std() > 0.5
    live = KP.box_sizes_ref(boxes, EDGE_SIZE, labels)[4]
    assert live.tolist() == [True, True, True, False, False, True]


def test_wide_boxes_reach_64_chunks():
    heat, boxes, (kps, scores) = wide_search_case()
    w, h, Wr, Hr, live = KP.box_sizes_ref(boxes, WIDE_SIZE)
    assert live.all() and Wr.tolist() == [8192, 3] and Hr.tolist() == [3, 8192]
    assert Wr[0] // 128 == 64, "64 column chunks of 128"
    assert np.all(kps[..., 2] == 1.0) and kps[0, 0, 0] > 128.0 and kps[1, 0, 1] > 128.0, "the maximum lies past the first chunk"
    assert KP.box_sizes_ref(boxes + F(0.5) * np.array([0, 0, 1, 1], F), WIDE_SIZE)[4].tolist() == [False, False]


# =====================================================================================================================
# 9. towers with unequal widths
# =====================================================================================================================
# (in_channels, layers): the widest tensor in the middle of eight layers; the input the widest
TOWERS = [(128, (64, 192, 64, 128, 64, 64, 64, 64)), (256, (64, 128))]
TOWER_M, TOWER_C, TOWER_CR, TOWER_KP = 2, 5, 64, 3
TOWER_ROWS = (4, 6)     # the second forward has more rows than the first: the scratch grows once


@cached
def tower_case(in_channels, layers):
    """(mask head state, keypoint head state, pooled [6, a, 2, 2] >= 0, labels, boxes)"""
    g = np.random.default_rng(in_channels + len(layers))
    pooled = np.maximum(g.standard_normal((TOWER_ROWS[1], in_channels, TOWER_M, TOWER_M)), 0).astype(F)
    labels = np.array([1, 4, -1, 2, 3, 1], np.int32)
    boxes = np.array([[1.5, 2.0, 30.0, 60.0], [0, 0, 40, 72], [1, 1, 9, 9], [3, 3, 3.5, 3.25], [2, 1, 12, 8], [5.25, 4.5, 37.0, 19.75]], F)
    return (MK.generate_mask_head_state(in_channels, layers, TOWER_CR, TOWER_C, seed=len(layers)),
            KP.generate_keypoint_head_state(in_channels, layers, TOWER_KP, seed=len(layers)), pooled, labels, boxes)


@pytest.mark.parametrize("in_channels,layers", TOWERS)
def test_tower_inputs(in_channels, layers):
    mst, kst, pooled, labels, boxes = tower_case(in_channels, layers)
    widest = max((in_channels,) + layers)
    if len(layers) == 8:
        assert widest > in_channels and widest > layers[-1] and layers.index(widest) not in (0, 7)
        assert len(set(layers)) >= 3, "ping and pong are read at several widths"
    else:
        assert widest == in_channels > max(layers)
    assert all(c % 64 == 0 for c in (in_channels,) + layers)
    mouts, kouts = MK.mask_head_ref(pooled, mst, layers=True), KP.keypoint_head_ref(pooled, kst, layers=True)
    assert [o.shape[1] for o in mouts[:-1]] == list(layers) == [o.shape[1] for o in kouts[:-1]]
    for o in mouts[:-1] + kouts[:-1]:
        assert o.std() > 0.05 and (o > 0).mean() > 0.1, "no layer's activations die on the way"
    assert kouts[-1].shape == (6, TOWER_KP, 8, 8) and kouts[-1].std() > 0.05
    p64 = MK.predict_ref(mouts[-1], labels, mst[MK.PREDICTOR_KEYS[2]].reshape(TOWER_C, TOWER_CR), mst[MK.PREDICTOR_KEYS[3]])
    assert p64[labels >= 1].min() > 0 and p64[labels >= 1].max() < 1 and np.ptp(p64[labels >= 1]) > 0.2
