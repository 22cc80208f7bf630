"""The box head's post-processing on the host: the numpy statement of the contract (resnet_c_amd/detection.py) against
known answers and against a second, independently written scalar float64 pipeline; the generator the GPU tests share;
the state keys; the C-ABI's symbols.  No GPU.  (test_detect_gpu.py imports the generator from here.)"""
import math
import os
import re

import numpy as np

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import detection as D
from resnet_c_amd import rpn
from test_rpn_host import chain_cases, clustered_boxes, decode_bound, special_logits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("rn_detect_postprocess_forward", "rn_box_head_create", "rn_box_head_set_tensor", "rn_box_head_finalize",
         "rn_box_head_destroy", "rn_box_head_forward", "rn_fpn_forward_detections", "rn_model_forward_detections",
         "rn_model_forward_detections_u8")
IMAGE = (56, 72)   # clustered_boxes lives in 64 x 48 and reaches a little past it: the clip bites on a few boxes


# ---- the generator shared with the GPU tests --------------------------------------------------------------------
def detect_case(seed, B, Rn, C, kind="random", delta_std=0.5, pad=True):
    """(head [B*Rn, P], rois [B*Rn, 5]): per image clustered proposals with small deltas.  The logit of the class a
    box's centre hashes to is raised, so the boxes of a cluster compete inside one class.  kind: random; quantised (the
    rows are drawn from 6 distinct ones: probabilities tie in mass, across RoIs and across classes); special (NaN,
    +-inf, +-0 sown into the logits of every fourth row).  pad: the last RoIs of an image are the RPN's padding rows (index -1, box 0), one
    RoI has no width, one no height and one carries another image's index."""
    g = np.random.default_rng([seed, B, Rn, C])
    K = B * Rn
    rois = np.zeros((K, 5), F)
    for b in range(B):
        rois[b * Rn:(b + 1) * Rn, 0] = b
        rois[b * Rn:(b + 1) * Rn, 1:] = clustered_boxes(Rn, seed=1000 * seed + 31 * b + Rn)
    rois[:, 1:] = np.clip(rois[:, 1:], 0, [IMAGE[1], IMAGE[0], IMAGE[1], IMAGE[0]]).astype(F)
    lg = (g.standard_normal((K, C)) * 1.5).astype(F)
    if kind == "quantised":
        pool = np.round(g.standard_normal((6, C)) * 2).astype(F) / 2
        lg = pool[g.integers(0, 6, K)]
    else:
        cx, cy = (rois[:, 1] + rois[:, 3]) / 2, (rois[:, 2] + rois[:, 4]) / 2
        hot = ((cx // 8).astype(np.int64) + 8 * (cy // 8).astype(np.int64)) % (C - 1) + 1
        lg[np.arange(K), hot] += F(3.0)
        if kind == "special":   # every fourth row: most of those come out as NaN throughout, a few hold -inf or +-0 only
            lg[::4] = special_logits(g, lg[::4].shape)
            lg[::8, 1:] = np.where(np.isfinite(lg[::8, 1:]) | np.isneginf(lg[::8, 1:]), lg[::8, 1:], F(-0.0))
            lg[::8, 0] = F(0.0)
    deltas = (g.standard_normal((K, 4 * C)) * delta_std).astype(F)
    if pad and Rn >= 8:
        for b in range(B):
            last = (b + 1) * Rn
            rois[last - max(1, Rn // 10):last] = [-1, 0, 0, 0, 0]
            rois[b * Rn + 1, 3] = rois[b * Rn + 1, 1]                  # no width: min_size fails whatever the deltas
            rois[b * Rn + 3, 4] = rois[b * Rn + 3, 2]                  # no height
            deltas[b * Rn + 1] = deltas[b * Rn + 3] = 0
            rois[b * Rn + 2, 0] = b + 1                                # not this image's row
    return D.pack_head(lg, deltas), rois


# ---- a second pipeline, written independently in float64 with explicit loops ------------------------------------
def second_pipeline(head, rois, B, C, image, score_thresh, nms_thresh, Dn, weights, min_size):
    """postprocess_detections, scalar float64: per image the list of (label, roi) and the smallest distance of any
    compared IoU from nms_thresh and of any score from score_thresh"""
    H, W = image
    K = head.shape[0]
    Rn = K // B
    clip = float(rpn.BBOX_XFORM_CLIP)
    gap_iou, gap_score, out = math.inf, math.inf, []
    for b in range(B):
        cands = {}
        for r in range(Rn):
            k = b * Rn + r
            row = [float(v) for v in head[k, :C]]
            mx = max(row)
            e = [math.exp(v - mx) for v in row]
            tot = sum(e)
            x1, y1, x2, y2 = (float(v) for v in rois[k, 1:])
            if float(rois[k, 0]) != b:
                continue
            for c in range(1, C):
                p = e[c] / tot
                gap_score = min(gap_score, abs(p - score_thresh))
                d = [float(v) for v in head[k, C + 4 * c:C + 4 * c + 4]]
                wa, ha = x2 - x1, y2 - y1
                pcx, pcy = d[0] / weights[0] * wa + x1 + 0.5 * wa, d[1] / weights[1] * ha + y1 + 0.5 * ha
                pw, ph = math.exp(min(d[2] / weights[2], clip)) * wa, math.exp(min(d[3] / weights[3], clip)) * ha
                bx = [min(max(pcx - pw / 2, 0.0), W), min(max(pcy - ph / 2, 0.0), H), min(max(pcx + pw / 2, 0.0), W),
                      min(max(pcy + ph / 2, 0.0), H)]
                if p > score_thresh and bx[2] - bx[0] >= min_size and bx[3] - bx[1] >= min_size:
                    cands.setdefault(c, []).append((-p, r, bx))
        survivors = []
        for c, lst in cands.items():
            lst.sort(key=lambda t: (t[0], t[1]))
            kept = []
            for negp, r, bx in lst:
                alive = True
                for _, _, o in kept:
                    inter = max(min(bx[2], o[2]) - max(bx[0], o[0]), 0.0) * max(min(bx[3], o[3]) - max(bx[1], o[1]), 0.0)
                    union = (bx[2] - bx[0]) * (bx[3] - bx[1]) + (o[2] - o[0]) * (o[3] - o[1]) - inter
                    if union > 0:
                        gap_iou = min(gap_iou, abs(inter / union - nms_thresh))
                        if inter / union > nms_thresh:
                            alive = False
                            break
                if alive:
                    kept.append((negp, r, bx))
            survivors += [(negp, r * (C - 1) + (c - 1), c, r) for negp, r, _ in kept]
        survivors.sort(key=lambda t: (t[0], t[1]))
        out.append([(c, r) for _, _, c, r in survivors[:Dn]])
    return out, gap_iou, gap_score


# ---- the tests ---------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_typed():
    text = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    lib = L.lib()
    for n in NAMES:
        assert re.search(r"RN_API int " + n + r"\(", text), n
        assert n in L.SIGNATURES and getattr(lib, n).argtypes == L.SIGNATURES[n][1]
    assert [f[0] for f in L.Detections._fields_] == ["boxes", "scores", "labels", "roi", "count", "probs", "class_boxes", "valid", "keep"]
    assert L.DetectRequest.detections_per_img.offset == 16 and L.DetectRequest.weights.offset == 24 and L.DetectRequest.out.offset == 40
    assert R.BoxHead is D.BoxHead and "launches" in text[text.index("The box head behind the pooler"):]


def test_postprocess_ref_against_the_second_pipeline():
    """seeds for which the float64 pipeline keeps every IoU and every score at least 1e-5 from its threshold: there the
    fp32 statement must reach the same labels and rows in the same order"""
    ran = 0
    for seed, (B, Rn, C) in enumerate([(1, 40, 5), (2, 64, 5), (1, 100, 9), (2, 30, 2)]):
        head, rois = detect_case(seed, B, Rn, C)
        want, gap_iou, gap_score = second_pipeline(head, rois, B, C, IMAGE, 0.05, 0.5, 20, D.BOX_WEIGHTS, D.MIN_SIZE)
        assert min(gap_iou, gap_score) >= 1e-5, f"seed {seed}: choose another; gaps {gap_iou:.3e} (IoU) {gap_score:.3e} (score)"
        got = D.postprocess_ref(head, rois, B, C, IMAGE, 0.05, 0.5, 20)
        for b in range(B):
            n = int(got["count"][b])
            mine = list(zip(got["labels"][b, :n].tolist(), got["roi"][b, :n].tolist()))
            assert mine == want[b], f"seed {seed} image {b}: nearest IoU {gap_iou:.3e}, nearest score {gap_score:.3e} from the threshold"
            assert (got["labels"][b, n:] == -1).all() and (got["roi"][b, n:] == -1).all() and not got["scores"][b, n:].any()
            ran += n
        logits, deltas = D.unpack_head(head, C)
        for c in range(1, C):
            err = np.abs(got["class_boxes"][:, c].astype(np.float64) - rpn.decode_f64(rois[:, 1:], deltas[:, c], D.BOX_WEIGHTS, IMAGE))
            assert (err <= decode_bound(rois[:, 1:], deltas[:, c], D.BOX_WEIGHTS)).all()
    assert ran > 40


def _case(probs, boxes, Dn=4, st=0.25, nt=0.5, image_idx=None):
    """one image; probs [R,C] given, boxes [R,4] used for every class"""
    p = np.asarray(probs, F)
    Rn, C = p.shape
    bx = np.repeat(np.asarray(boxes, F)[:, None, :], C, axis=1)
    rois = np.zeros((Rn, 5), F)
    if image_idx is not None:
        rois[:, 0] = image_idx
    out = D.score_decode_ref(np.zeros((Rn, D.head_pitch(C)), F), rois, 1, C, (100, 100), st, 1e-2, probs=p, class_boxes=bx)
    out["keep"] = D.class_nms_ref(p, bx, out["valid"], 1, nt)
    out.update(D.merge_ref(p, bx, out["keep"], 1, Dn))
    return out


def test_known_answers():
    far = [[0, 0, 2, 1], [10, 0, 12, 1], [20, 0, 22, 1], [30, 0, 32, 1], [40, 0, 42, 1], [50, 0, 52, 1]]
    # strict > at the score threshold; the background never appears, whatever its probability
    out = _case([[0.5, 0.25, 0.25], [0.2, 0.3, 0.5]], far[:2])
    assert out["valid"].tolist() == [[0, 0, 0], [0, 1, 1]] and out["count"][0] == 2
    assert out["labels"][0].tolist() == [2, 1, -1, -1] and out["roi"][0].tolist() == [1, 1, -1, -1] and out["scores"][0].tolist() == [0.5, F(0.3), 0, 0]
    # IoU exactly at the threshold does not suppress: boxes 0 and 1 of test_rpn_host.KNOWN overlap by exactly 1/2
    known = [[0, 0, 2, 1], [0, 0, 1, 1], [0, 0, 4, 1], [0, 0, 3, 1]]
    out = _case([[0.1, 0.9], [0.2, 0.8], [0.3, 0.7], [0.4, 0.6]], known, Dn=4)
    assert out["keep"][:, 1].tolist() == [1, 1, 1, 0] and out["roi"][0].tolist() == [0, 1, 2, -1]
    out = _case([[0.1, 0.9], [0.2, 0.8], [0.3, 0.7], [0.4, 0.6]], known, nt=np.nextafter(F(0.5), F(0)))
    assert out["keep"][:, 1].tolist() == [1, 0, 0, 0]
    # equal probabilities order by f = r * (C - 1) + (c - 1): row first, then class
    out = _case([[0.0, 0.5, 0.5], [0.0, 0.5, 0.5]], far[:2], Dn=3)
    assert list(zip(out["roi"][0].tolist(), out["labels"][0].tolist())) == [(0, 1), (0, 2), (1, 1)] and out["count"][0] == 3
    # inside a class equal probabilities order by r: the earlier row suppresses the later one
    out = _case([[0.0, 0.9], [0.0, 0.9]], [[0, 0, 4, 4], [0, 0, 4, 3]])
    assert out["keep"][:, 1].tolist() == [1, 0]
    # a padding row (image index -1) and a row of another image never appear
    out = _case([[0.0, 0.9], [0.0, 0.8], [0.0, 0.7]], far[:3], image_idx=[0, -1, 1])
    assert out["valid"][:, 1].tolist() == [1, 0, 0] and out["count"][0] == 1
    # more survivors than D; no survivor at all
    out = _case([[0.0, 0.4 + 0.1 * i] for i in range(6)], far, Dn=4)
    assert out["count"][0] == 4 and out["roi"][0].tolist() == [5, 4, 3, 2] and out["keep"][:, 1].sum() == 6
    out = _case([[0.9, 0.1]] * 3, far[:3])
    assert out["count"][0] == 0 and (out["labels"] == -1).all() and not out["boxes"].any() and not out["keep"].any()
    # a NaN anywhere fails, a box below min_size fails
    out = _case([[0.0, np.nan], [0.0, 0.9]], [[0, 0, 2, 1], [0, 0, 0.005, 1]])
    assert not out["valid"].any()


def test_the_generator_bites_on_the_reference():
    """the inputs of the GPU tests, judged on the CPU: some class keeps between 5 % and 60 % of its valid candidates,
    a chain case exists, every clause of Valid fails somewhere and holds somewhere"""
    seen = np.zeros((4, 2), bool)
    for B, Rn, C in [(1, 63, 2), (3, 100, 5), (1, 1000, 91), (3, 65, 5)]:
        head, rois = detect_case(7, B, Rn, C)
        out = D.postprocess_ref(head, rois, B, C, IMAGE, 0.05, 0.5, 100)
        valid, keep = out["valid"].astype(bool), out["keep"].astype(bool)
        bites, chains = 0, 0
        for b in range(B):
            rows = slice(b * Rn, (b + 1) * Rn)
            for c in range(1, C):
                nv, nk = valid[rows, c].sum(), keep[rows, c].sum()
                if nv >= 10 and 0.05 * nv <= nk <= 0.60 * nv:
                    bites += 1
                r = np.flatnonzero(valid[rows, c])
                r = r[rpn.select_ref(out["probs"][rows, c][r], r.size)]
                chains += chain_cases(out["class_boxes"][rows, c][r], keep[rows, c][r], 0.5)
        assert bites >= 1 and chains >= 1, (B, Rn, C, bites, chains)
        bx, p = out["class_boxes"][:, 1:], out["probs"][:, 1:]
        real = rois[:, 0] == np.repeat(np.arange(B), Rn)
        for i, clause in enumerate((np.broadcast_to(real[:, None], p.shape), p > F(0.05), bx[..., 2] - bx[..., 0] >= F(1e-2),
                                    bx[..., 3] - bx[..., 1] >= F(1e-2))):
            seen[i] |= [clause.any(), not clause.all()]
        assert seen[[0, 2, 3]].all(), (B, Rn, C, seen.tolist())   # (with two classes no score lies below the threshold)
    assert seen.all(), seen.tolist()


def test_state_keys_and_reference():
    import torch
    st = D.generate_box_head_state(256, 64, 5, seed=2)
    assert {k: v.shape for k, v in st.items()} == D.head_shapes(256, 64, 5)
    pre = {"roi_heads." + k: v for k, v in st.items()}
    pre["backbone.body.conv1.weight"] = np.zeros((64, 3, 7, 7), F)
    for state in (st, pre):
        mine, rest = D.split_state(state)
        assert sorted(mine) == sorted(D.HEAD_KEYS) and all(np.array_equal(mine[k], st[k]) for k in st)
    assert list(D.split_state(pre)[1]) == ["backbone.body.conv1.weight"]
    whole = dict(pre)
    whole.update({"rpn." + k: v for k, v in rpn.generate_rpn_state(64, 3).items()})
    whole.update({"backbone.fpn." + k: v for k, v in R.fpn.generate_fpn_state((64, 128), 64).items()})
    parts = D.split_detector_state(whole)
    assert sorted(parts["box_head"]) == sorted(D.HEAD_KEYS) and sorted(parts["rpn"]) == sorted(rpn.HEAD_KEYS)
    assert list(parts["backbone"]) == ["conv1.weight"] and len(parts["neck"]) == 8
    g = np.random.default_rng(0)
    x = g.standard_normal((7, 64, 2, 2))
    t = lambda k: torch.from_numpy(st[k].astype(np.float64))  # noqa: E731
    lin = torch.nn.functional.linear
    h = torch.relu(lin(torch.from_numpy(x).flatten(1), t(D.HEAD_KEYS[0]), t(D.HEAD_KEYS[1])))
    h = torch.relu(lin(h, t(D.HEAD_KEYS[2]), t(D.HEAD_KEYS[3])))
    want = torch.cat([lin(h, t(D.HEAD_KEYS[4]), t(D.HEAD_KEYS[5])), lin(h, t(D.HEAD_KEYS[6]), t(D.HEAD_KEYS[7]))], dim=1).numpy()
    got = D.box_head_ref(x, pre, 5)
    assert got.shape == (7, 28) and not got[:, 25:].any() and np.abs(got[:, :25] - want).max() < 1e-12
    # pack_head: torchvision's bbox_pred row 4c + j is column C + 4c + j
    hd = D.pack_head(want[:, :5], want[:, 5:])
    assert hd.shape == (7, 28) and hd[3, 5 + 4 * 2 + 1] == F(want[3, 5 + 9])
