"""RPN proposals behind the head, on the host: the numpy statement of the contract (resnet_c_amd/rpn.py) against known
answers and against a second, independently written float64 pipeline; the decode bound as a formula; the C-ABI's
symbols.  No GPU.  (test_rpn_gpu.py imports the generators and the second pipeline from here.)"""
import os
import re

import numpy as np
import pytest

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import rpn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("rn_rpn_select_decode_forward", "rn_rpn_nms_merge_forward", "rn_nms_forward", "rn_box_decode_forward", "rn_rpn_create",
         "rn_rpn_set_tensor", "rn_rpn_finalize", "rn_rpn_destroy", "rn_rpn_forward", "rn_fpn_forward_proposals")
KNOWN = np.array([[0, 0, 2, 1], [0, 0, 1, 1], [0, 0, 4, 1], [0, 0, 3, 1]], F)   # IoUs with box 0: 1/2, 1/2, 2/3


# ---- the decode bound, derived here ------------------------------------------------------------------------------
EXPF_ULP = 1.0   # the documented error of the device's expf, in units in the last place (HIP math API)


def decode_bound(anchors, deltas, weights=(1.0, 1.0, 1.0, 1.0)) -> np.ndarray:
    """[N, 4]: how far a coordinate of the fp32 decode may lie from decode_f64, from the operation count.  With
    u = 2^-24 (one fp32 rounding is at most u relative) and E = EXPF_ULP (an error of E units in the last place is at
    most 2 E u relative), first order in u:
        wa = ax2 - ax1                     u |wa|
        cx = ax1 + 0.5 wa                  u |wa| / 2 + u |cx|
        dx = d0 / wx; dx * wa              u (1 + 1 + 1) |dx wa|        (dx, wa, the product)
        pcx = dx wa + cx                   the two above + u |pcx|
        dw = d2 / ww                       u |dw| absolute, which the exponential turns into u |dw| relative
        pw = expf(dw) * wa                 u (|dw| + 2 E + 1 + 1) |pw|  (argument, expf, wa, the product)
        x = pcx -+ 0.5 pw                  the sum of pcx's and half of pw's + u |x|
    The clip to the image moves no two values apart.  The second-order terms are covered by the factor 1 + 2^-10."""
    a, d = np.asarray(anchors, dtype=np.float64).reshape(-1, 4), np.asarray(deltas, dtype=np.float64).reshape(-1, 4)
    u = 2.0 ** -24
    wgt = [float(F(v)) for v in weights]
    out = np.empty((a.shape[0], 4))
    for ax in (0, 1):
        wa = a[:, 2 + ax] - a[:, ax]
        cx = a[:, ax] + 0.5 * wa
        dx, dw = d[:, ax] / wgt[ax], np.minimum(d[:, 2 + ax] / wgt[2 + ax], float(rpn.BBOX_XFORM_CLIP))
        pcx, pw = dx * wa + cx, np.exp(dw) * wa
        e_pcx = np.abs(wa) / 2 + np.abs(cx) + 3 * np.abs(dx * wa) + np.abs(pcx)
        e_pw = (np.abs(dw) + 2 * EXPF_ULP + 2) * np.abs(pw)
        for sign, col in ((-1.0, ax), (1.0, 2 + ax)):
            out[:, col] = u * (e_pcx + 0.5 * e_pw + np.abs(pcx + sign * 0.5 * pw)) * (1 + 2.0 ** -10)
    return out


# ---- generators shared with the GPU tests ----------------------------------------------------------------------
def clustered_boxes(n, seed=None):
    """[n,4]: max(1, n // 6) centres in 64 x 48, widths and heights uniform in 4..32, every box a cluster's box with
    every coordinate jittered by up to 8 % of the cluster's size; from default_rng(n) unless a seed is given"""
    g = np.random.default_rng(n if seed is None else seed)
    m = max(1, n // 6)
    cx, cy = g.uniform(0, 64, m), g.uniform(0, 48, m)
    w, h = g.uniform(4, 32, m), g.uniform(4, 32, m)
    c = g.integers(0, m, n)
    size = np.stack([w[c], h[c], w[c], h[c]], axis=1)
    box = np.stack([cx[c] - w[c] / 2, cy[c] - h[c] / 2, cx[c] + w[c] / 2, cy[c] + h[c] / 2], axis=1)
    return (box + g.uniform(-1, 1, (n, 4)) * 0.08 * size).astype(F)


def chain_cases(boxes, keep, thr):
    """suppressed boxes that would themselves have suppressed a later survivor"""
    n, cases = boxes.shape[0], 0
    for j in np.flatnonzero(~keep):
        later = np.flatnonzero(keep[j + 1:]) + j + 1
        if later.size and (rpn.iou_ref(boxes[j], boxes[later]) > F(thr)).any():
            cases += 1
    return cases


def special_logits(g, shape):
    """N(0,1) with +-0, NaN and +-inf sown in"""
    x = g.standard_normal(shape).astype(F)
    flat = x.reshape(-1)
    pick = g.permutation(flat.size)
    vals = [0.0, -0.0, np.nan, np.inf, -np.inf]
    for i, p in enumerate(pick[:max(5, flat.size // 4)]):
        flat[p] = vals[i % 5]
    return x


def random_heads(g, B, sizes, A, kind="random", delta_std=0.3):
    """one [B,h,w,P] head output per level; kind: random, quantised (8 values: mass ties) or special"""
    heads = []
    for h, w in sizes:
        hd = np.zeros((B, h, w, rpn.head_channels(A)), F)
        lg = g.standard_normal((B, h, w, A)).astype(F)
        if kind == "quantised":
            lg = np.round(lg * 2).clip(-4, 3).astype(F) / 2
        elif kind == "special":
            lg = special_logits(g, (B, h, w, A))
        hd[..., :A] = lg
        hd[..., A:5 * A] = (g.standard_normal((B, h, w, 4 * A)) * delta_std).astype(F)
        heads.append(hd)
    return heads


# ---- a second pipeline, written independently in float64 with explicit loops ------------------------------------
def second_pipeline(heads, sizes_per_level, ratios, image_size, pre, post, nms_thresh, min_size):
    """filter_proposals for image 0 only, scalar float64 code: returns (selected anchor ids per level, boxes per
    level, kept ranks per level, merged (level, rank) list, the minimum distance of any IoU from the threshold)"""
    import math
    H, W = image_size
    sel, boxes, kept, gap = [], [], [], math.inf
    for l, hd in enumerate(heads):
        _, h, w, _ = hd.shape
        base = []
        for r in ratios:
            for s in sizes_per_level[l]:
                hr = float(F(math.sqrt(F(r))))
                wr = float(F(1) / F(hr))
                base.append([float(np.rint(F(v) / F(2))) for v in (F(-wr) * F(s), F(-hr) * F(s), F(wr) * F(s), F(hr) * F(s))])
        A = len(base)
        sh, sw = H // h, W // w
        entries = []
        for y in range(h):
            for x in range(w):
                for a in range(A):
                    v = float(hd[0, y, x, a])
                    entries.append((-(v if v == v else -math.inf), (y * w + x) * A + a))
        entries.sort()   # by descending logit, then ascending index (-0.0 == 0.0 compare equal)
        ids = [n for _, n in entries[:pre]]
        bl = []
        for n in ids:
            pos, a = divmod(n, A)
            y, x = divmod(pos, w)
            ax1, ay1, ax2, ay2 = base[a][0] + x * sw, base[a][1] + y * sh, base[a][2] + x * sw, base[a][3] + y * sh
            d = [float(v) for v in hd[0, y, x, A + 4 * a:A + 4 * a + 4]]
            wa, ha = ax2 - ax1, ay2 - ay1
            pcx, pcy = d[0] * wa + ax1 + 0.5 * wa, d[1] * ha + ay1 + 0.5 * ha
            pw = math.exp(min(d[2], float(rpn.BBOX_XFORM_CLIP))) * wa
            ph = math.exp(min(d[3], float(rpn.BBOX_XFORM_CLIP))) * ha
            bl.append([min(max(pcx - pw / 2, 0.0), W), min(max(pcy - ph / 2, 0.0), H),
                       min(max(pcx + pw / 2, 0.0), W), min(max(pcy + ph / 2, 0.0), H)])
        ok = [b[2] - b[0] >= min_size and b[3] - b[1] >= min_size for b in bl]
        kl = []
        for i, b in enumerate(bl):
            if not ok[i]:
                continue
            alive = True
            for j in kl:
                c = bl[j]
                inter = max(min(b[2], c[2]) - max(b[0], c[0]), 0.0) * max(min(b[3], c[3]) - max(b[1], c[1]), 0.0)
                union = (b[2] - b[0]) * (b[3] - b[1]) + (c[2] - c[0]) * (c[3] - c[1]) - inter
                iou = inter / union if union > 0 else math.nan
                if iou == iou:
                    gap = min(gap, abs(iou - nms_thresh))
                if iou > nms_thresh:
                    alive = False
                    break
            if alive:
                kl.append(i)
        sel.append(ids), boxes.append(bl), kept.append(kl)
    merged = sorted(((-float(heads[l][0].reshape(-1, heads[l].shape[3])[ids_l[r] // len(base), ids_l[r] % len(base)]),
                      l * pre + r) for l, (ids_l, kl) in enumerate(zip(sel, kept)) for r in kl))[:post]
    return sel, boxes, kept, [divmod(p, pre) for _, p in merged], gap


# ---- the tests ---------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_typed():
    text = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    lib = L.lib()
    for n in NAMES:
        assert re.search(r"RN_API int " + n + r"\(", text), n
        assert n in L.SIGNATURES and getattr(lib, n).argtypes == L.SIGNATURES[n][1]
    assert [f[0] for f in L.RpnCandidates._fields_] == ["index", "logit", "box", "valid", "count"]
    assert [f[0] for f in L.RpnProposals._fields_] == ["boxes", "logits", "levels", "count", "rois", "cand_keep"]
    assert R.AnchorGenerator is rpn.AnchorGenerator


def test_base_anchor_known_answers():
    base = rpn.AnchorGenerator(((32,), (512,)), (0.5, 1.0, 2.0)).base_anchors()
    assert base.dtype == F and base.shape == (2, 3, 4)
    assert base[0].tolist() == [[-23, -11, 23, 11], [-16, -16, 16, 16], [-11, -23, 11, 23]]
    assert base[1].tolist() == [[-362, -181, 362, 181], [-256, -256, 256, 256], [-181, -362, 181, 362]]
    # the index is ratio * n_sizes + size
    two = rpn.AnchorGenerator(((32, 512),), ((0.5, 1.0, 2.0),)).base_anchors()[0]
    assert two[0].tolist() == [-23, -11, 23, 11] and two[1].tolist() == [-362, -181, 362, 181] and two[5].tolist() == [-181, -362, 181, 362]
    assert rpn.AnchorGenerator().num_anchors_per_location() == 3
    with pytest.raises(ValueError):
        rpn.AnchorGenerator(((32,), (64, 128)), (0.5, 1.0))


def test_grid_anchors_at_strides_that_do_not_divide():
    ag = rpn.AnchorGenerator(((32,),), (0.5, 1.0, 2.0))
    (g,) = ag.grid_anchors([(5, 3)], (72, 40))   # strides 72 // 5 = 14 and 40 // 3 = 13
    base = ag.base_anchors()[0]
    assert g.shape == (45, 4) and g.dtype == F
    for y in range(5):
        for x in range(3):
            for a in range(3):
                want = base[a] + np.array([x * 13, y * 14, x * 13, y * 14], F)
                assert np.array_equal(g[(y * 3 + x) * 3 + a], want)


def test_nms_ref_known_answers():
    assert np.flatnonzero(rpn.nms_ref(KNOWN, 0.5)).tolist() == [0, 1, 2]                # IoU exactly 0.5 does not suppress
    assert np.flatnonzero(rpn.nms_ref(KNOWN, np.nextafter(F(0.5), F(0)))).tolist() == [0]
    assert rpn.nms_ref(np.zeros((2, 4), F), 0.5).tolist() == [True, True]               # 0/0 is a NaN: no suppression
    assert np.flatnonzero(rpn.nms_ref(KNOWN, np.nextafter(F(0.5), F(0)), valid=[0, 1, 1, 1])).tolist() == [1, 2]   # IoU(1,2) = 1/4, IoU(2,3) = 3/4
    assert not rpn.nms_ref(KNOWN, 0.5, valid=np.zeros(4)).any()


def test_select_ref_is_the_stable_argsort():
    g = np.random.default_rng(5)
    rows = [special_logits(g, 50), np.round(g.standard_normal(300)).astype(F), np.array([np.nan, np.nan, -np.inf, 0.0, -0.0], F)]
    for x in rows:
        v = np.where(np.isnan(x), -np.inf, x)
        for k in (1, 7, x.size, x.size + 3):
            got = rpn.select_ref(x, k)
            assert np.array_equal(got, np.argsort(-v, kind="stable")[:k])
            for a, b in zip(got[:-1], got[1:]):   # the order itself, pair by pair
                assert v[a] > v[b] or (v[a] == v[b] and a < b)
    assert rpn.select_ref(np.array([0.0, -0.0, np.nan, -np.inf], F), 4).tolist() == [0, 1, 2, 3]


def test_merge_ref_orders_by_logit_then_position():
    lg = np.array([[1.0, 0.5, 0.5], [2.0, 0.5, -1.0]], F)
    bx = np.arange(24, dtype=F).reshape(2, 3, 4)
    keep = np.array([[1, 1, 1], [1, 1, 0]], bool)
    boxes, logits, levels, cnt = rpn.merge_ref(lg, bx, keep, 4)
    assert cnt == 4 and levels.tolist() == [1, 0, 0, 0] and logits.tolist() == [2.0, 1.0, 0.5, 0.5]
    assert np.array_equal(boxes, bx.reshape(-1, 4)[[3, 0, 1, 2]])
    boxes, logits, levels, cnt = rpn.merge_ref(lg, bx, keep, 7)
    assert cnt == 5 and levels.tolist() == [1, 0, 0, 0, 1, -1, -1] and np.isneginf(logits[5:]).all() and not boxes[5:].any()


def test_decode_bound_is_a_formula_of_the_operation_count():
    """u = 2^-24 per fp32 rounding, expf within EXPF_ULP units in the last place (the HIP math API's figure): for an
    anchor (0,0,16,16) and zero deltas the terms are wa/2 + cx + pcx = 8 + 8 + 8, pw (0 + 2 E + 2) / 2 = 32 and
    |x| = 0 resp. 16"""
    assert EXPF_ULP == 1.0
    b = decode_bound([[0, 0, 16, 16]], [[0, 0, 0, 0]])
    u = 2.0 ** -24
    assert np.allclose(b[0], [u * 56 * (1 + 2.0 ** -10), u * 56 * (1 + 2.0 ** -10), u * 72 * (1 + 2.0 ** -10), u * 72 * (1 + 2.0 ** -10)], rtol=1e-12)
    # and numpy's own fp32 decode obeys it
    g = np.random.default_rng(1)
    a = rpn.grid_anchors(rpn.AnchorGenerator(((64,),)).base_anchors(), [(9, 7)], (144, 112))[0]
    d = (g.standard_normal(a.shape) * 0.5).astype(F)
    d[::17, 2] = 6.0   # above the clip
    for wgt in ((1, 1, 1, 1), (10, 10, 5, 5)):
        err = np.abs(rpn.decode_ref(a, d, wgt).astype(np.float64) - rpn.decode_f64(a, d, wgt))
        assert (err <= decode_bound(a, d, wgt)).all(), (err / decode_bound(a, d, wgt)).max()


def test_filter_proposals_ref_against_the_second_pipeline():
    sizes, ratios, image = ((16,), (32,), (64,)), (0.5, 1.0, 2.0), (72, 40)
    base = rpn.AnchorGenerator(sizes, ratios).base_anchors()
    for seed in range(4):
        g = np.random.default_rng(seed)
        heads = random_heads(g, 1, [(18, 10), (9, 5), (5, 3)], 3, "random" if seed else "quantised")
        pre, post, thr, ms = 100, 60, 0.7, 4.0
        got = rpn.filter_proposals_ref(heads, base, image, pre, post, thr, 0.0, ms)
        sel, boxes, kept, merged, gap = second_pipeline(heads, sizes, ratios, image, pre, post, thr, ms)
        anchors = rpn.grid_anchors(base, [(18, 10), (9, 5), (5, 3)], image)
        for l in range(3):
            k = int(got["cand"]["count"][0, l])
            assert got["cand"]["index"][0, l, :k].tolist() == sel[l], f"seed {seed} level {l}: the selection differs"
            _, deltas = rpn.unpack_head(heads[l], 3)
            bound = decode_bound(anchors[l][sel[l]], deltas[0][sel[l]])
            err = np.abs(got["cand"]["box"][0, l, :k].astype(np.float64) - np.array(boxes[l]))
            assert (err <= bound).all(), f"seed {seed} level {l}: box error {(err / bound).max():.3f} of the bound"
            mine = np.flatnonzero(got["cand_keep"][0, l]).tolist()
            assert mine == kept[l], f"seed {seed} level {l}: survivors differ; the nearest IoU is {gap:.3e} from the threshold"
        c = int(got["count"][0])
        assert c == len(merged) and c <= post
        ranks = [(int(lv), int(np.flatnonzero((got["cand"]["box"][0, lv] == got["boxes"][0, i]).all(axis=1))[0]))
                 for i, lv in enumerate(got["levels"][0, :c])]
        assert [lv for lv, _ in ranks] == [lv for lv, _ in merged]
        assert (got["levels"][0, c:] == -1).all() and np.isneginf(got["logits"][0, c:]).all()
        assert np.array_equal(got["rois"][:c, 0], np.zeros(c, F)) and (got["rois"][c:, 0] == -1).all()


def test_logit_threshold_and_head_packing():
    assert rpn.logit_of(0.0) == -np.inf and rpn.logit_of(1.0) == np.inf and rpn.logit_of(0.5) == 0.0
    assert abs(rpn.logit_of(0.9) - np.log(9.0)) < 1e-6
    g = np.random.default_rng(0)
    o, d = g.standard_normal((2, 3, 4, 5)).astype(F), g.standard_normal((2, 12, 4, 5)).astype(F)
    hd = rpn.pack_head(o, d)
    assert hd.shape == (2, 4, 5, 16) and not hd[..., 15].any()
    lg, dl = rpn.unpack_head(hd, 3)
    # torchvision's permute_and_flatten: anchor n = (y*w + x)*A + a, delta c of anchor a in channel 4a + c
    assert lg[1, (2 * 5 + 3) * 3 + 1] == o[1, 1, 2, 3] and dl[1, (2 * 5 + 3) * 3 + 1, 2] == d[1, 4 * 1 + 2, 2, 3]


def test_the_clustered_generator_bites_on_the_reference():
    """for every n >= 63 the reference keeps between 5 % and 60 % of the boxes at every threshold, and at least one
    threshold has a chain case"""
    for n in (63, 64, 65, 129, 300):
        b = clustered_boxes(n)
        chains = []
        for thr in (0.3, 0.5, 0.7):
            keep = rpn.nms_ref(b, thr)
            assert 0.05 * n <= keep.sum() <= 0.60 * n, (n, thr, int(keep.sum()))
            chains.append(chain_cases(b, keep, thr))
        assert max(chains) >= 1, (n, chains)


def test_head_state_keys_and_reference():
    st = rpn.generate_rpn_state(64, 3, seed=2, std=0.03)
    assert {k: v.shape for k, v in st.items()} == rpn.head_shapes(64, 3)
    old = {"rpn." + k.replace("conv.0.0", "conv"): v for k, v in st.items()}
    old["backbone.x"] = 1
    mine, rest = rpn.split_state(old)
    assert sorted(mine) == sorted(rpn.HEAD_KEYS) and list(rest) == ["backbone.x"]
    g = np.random.default_rng(0)
    x = g.standard_normal((1, 64, 4, 3))
    hd = rpn.rpn_head_ref([x], old, 3)[0]
    assert hd.shape == (1, 4, 3, 16) and not hd[..., 15].any()
    # one output by hand: anchor 1's delta 2 at (y, x) = (2, 1) is channel A + 4 * 1 + 2
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    t = np.maximum(np.einsum("ocij,cij->o", st["head.conv.0.0.weight"].astype(np.float64), xp[0, :, 2:5, 1:4])
                   + st["head.conv.0.0.bias"], 0)
    want = st["head.bbox_pred.weight"].reshape(12, 64)[6].astype(np.float64) @ t + st["head.bbox_pred.bias"][6]
    assert abs(hd[0, 2, 1, 3 + 6] - want) < 1e-12
