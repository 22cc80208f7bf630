"""The box head behind the pooler (rn_detect.hip): torchvision's TwoMLPHead, FastRCNNPredictor and
RoIHeads.postprocess_detections in eval mode.

The arithmetic is the contract of include/rn_hip.h ("The box head behind the pooler"); this module restates it in numpy
-- every operation in fp32 and rounded on its own -- on top of rpn.py's decode, IoU and NMS.  Two operations are not
bit-defined against numpy: the softmax's and the decode's expf.  So a test compares the probabilities bit for bit with
ops.softmax (the same device code), the class boxes within a bound of the float64 decode, and everything behind them --
validity, NMS survivors, the merge -- bit for bit on the probabilities and boxes the device itself returned.

The *_ref functions are pure numpy and need no device.
"""
from __future__ import annotations

import numpy as np

from . import rpn
from ._lib import Handle

F = np.float32
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)   # torchvision's bbox_reg_weights of the box head
MIN_SIZE = 1e-2                        # torchvision's remove_small_boxes in postprocess_detections


def head_pitch(C: int) -> int:
    """P: 5 C rounded up to a multiple of 4"""
    return (5 * int(C) + 3) // 4 * 4


def pack_head(class_logits, box_regression) -> np.ndarray:
    """FastRCNNPredictor's outputs, class_logits [K,C] and box_regression [K,4C], as the [K,P] the launches read:
    column c the logit of class c, column C + 4c + j delta j of class c, zeros up to P"""
    lg, d = np.asarray(class_logits, dtype=F), np.asarray(box_regression, dtype=F)
    K, C = lg.shape
    assert d.shape == (K, 4 * C), (lg.shape, d.shape)
    out = np.zeros((K, head_pitch(C)), F)
    out[:, :C], out[:, C:5 * C] = lg, d
    return out


def unpack_head(head, C: int):
    """(logits [K,C], deltas [K,C,4]) of a [K,P] head output"""
    head = np.asarray(head)
    return head[:, :C], head[:, C:5 * C].reshape(-1, C, 4)


# ---- the contract in numpy ---------------------------------------------------------------------------------------
def softmax_ref(logits) -> np.ndarray:
    """expf(x - max) / sum in fp32 with numpy's exp and sum: the contract up to the device's expf and its summation
    order (ops.softmax is the bit-defined statement)"""
    x = np.asarray(logits, dtype=F)
    with np.errstate(all="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True)).astype(F)
        return (e / e.sum(axis=1, keepdims=True, dtype=F)).astype(F)


def score_decode_ref(head, rois, B: int, C: int, image_size, score_thresh: float = 0.05, min_size: float = MIN_SIZE,
                     weights=BOX_WEIGHTS, probs=None, class_boxes=None) -> dict:
    """Score, Decode and Valid: "probs" [K,C], "class_boxes" [K,C,4], "valid" [K,C] bytes.  probs / class_boxes: take
    these (the device's own) in place of softmax_ref's and decode_ref's, for a bit-for-bit check of what follows."""
    head, rois = np.asarray(head, dtype=F), np.asarray(rois, dtype=F).reshape(-1, 5)
    K = head.shape[0]
    R = K // B
    logits, deltas = unpack_head(head, C)
    p = softmax_ref(logits) if probs is None else np.asarray(probs, dtype=F).reshape(K, C)
    if class_boxes is None:
        bx = np.zeros((K, C, 4), F)
        for c in range(1, C):
            bx[:, c] = rpn.decode_ref(rois[:, 1:], deltas[:, c], weights, image_size)
    else:
        bx = np.asarray(class_boxes, dtype=F).reshape(K, C, 4)
    real = rois[:, 0] == np.repeat(np.arange(B, dtype=F), R)
    with np.errstate(all="ignore"):
        valid = (real[:, None] & (p > F(score_thresh)) & (bx[..., 2] - bx[..., 0] >= F(min_size))
                 & (bx[..., 3] - bx[..., 1] >= F(min_size)))
    valid[:, 0] = False
    return {"probs": p, "class_boxes": bx, "valid": valid.astype(np.uint8)}


def class_nms_ref(probs, class_boxes, valid, B: int, nms_thresh: float) -> np.ndarray:
    """keep [K,C] bytes: per (image, class c >= 1) the valid candidates in the order (p descending, r ascending),
    -0 == +0, and rpn.nms_ref on them"""
    p, bx, ok = np.asarray(probs, dtype=F), np.asarray(class_boxes, dtype=F), np.asarray(valid).astype(bool)
    K, C = p.shape
    R = K // B
    keep = np.zeros((K, C), np.uint8)
    for b in range(B):
        rows = slice(b * R, (b + 1) * R)
        for c in range(1, C):
            r = np.flatnonzero(ok[rows, c])
            if r.size == 0:
                continue
            r = r[rpn.select_ref(p[rows, c][r], r.size)]
            kept = rpn.nms_ref(bx[rows, c][r], nms_thresh)
            keep[b * R + r[kept], c] = 1
    return keep


def merge_ref(probs, class_boxes, keep, B: int, detections_per_img: int) -> dict:
    """The detections of every image: the survivors in the order (p descending, f ascending), f = r*(C-1) + (c-1),
    the first D; rows at or past count hold box 0, score 0, label -1, roi -1"""
    p, bx, kp = np.asarray(probs, dtype=F), np.asarray(class_boxes, dtype=F), np.asarray(keep).astype(bool)
    K, C = p.shape
    R, D = K // B, int(detections_per_img)
    out = {"boxes": np.zeros((B, D, 4), F), "scores": np.zeros((B, D), F), "labels": np.full((B, D), -1, np.int32),
           "roi": np.full((B, D), -1, np.int32), "count": np.zeros(B, np.int32)}
    for b in range(B):
        rows = slice(b * R, (b + 1) * R)
        f = np.flatnonzero(kp[rows, 1:].reshape(-1))
        f = f[rpn.select_ref(p[rows, 1:].reshape(-1)[f], D)]
        r, c = f // (C - 1), f % (C - 1) + 1
        n = f.size
        out["boxes"][b, :n], out["scores"][b, :n] = bx[rows][r, c], p[rows][r, c]
        out["labels"][b, :n], out["roi"][b, :n], out["count"][b] = c, r, n
    return out


def postprocess_ref(head, rois, B: int, C: int, image_size, score_thresh: float = 0.05, nms_thresh: float = 0.5,
                    detections_per_img: int = 100, weights=BOX_WEIGHTS, min_size: float = MIN_SIZE, probs=None,
                    class_boxes=None) -> dict:
    """postprocess_detections in the contract's fp32: rn_detect_postprocess_forward's nine outputs"""
    out = score_decode_ref(head, rois, B, C, image_size, score_thresh, min_size, weights, probs, class_boxes)
    out["keep"] = class_nms_ref(out["probs"], out["class_boxes"], out["valid"], B, nms_thresh)
    out.update(merge_ref(out["probs"], out["class_boxes"], out["keep"], B, detections_per_img))
    return out


# ---- the head's state ------------------------------------------------------------------------------------------
HEAD_KEYS = ("box_head.fc6.weight", "box_head.fc6.bias", "box_head.fc7.weight", "box_head.fc7.bias",
             "box_predictor.cls_score.weight", "box_predictor.cls_score.bias",
             "box_predictor.bbox_pred.weight", "box_predictor.bbox_pred.bias")


def head_shapes(in_features: int, representation: int, classes: int) -> dict:
    Fi, M, C = int(in_features), int(representation), int(classes)
    return dict(zip(HEAD_KEYS, ((M, Fi), (M,), (M, M), (M,), (C, M), (C,), (4 * C, M), (4 * C,))))


def split_state(state) -> tuple:
    """(the box head's tensors under HEAD_KEYS, the rest): takes the keys with or without the "roi_heads." prefix"""
    mine, rest = {}, {}
    for k, v in state.items():
        key = k[len("roi_heads."):] if k.startswith("roi_heads.") else k
        if key in HEAD_KEYS:
            mine[key] = v
        else:
            rest[k] = v
    return mine, rest


def split_detector_state(state) -> dict:
    """A whole fasterrcnn_resnet50_fpn state dict taken apart through the existing split_state's: "backbone" (the keys
    NativeModel reads) and "neck" (fpn.split_state), "rpn" (rpn.split_state) and "box_head" (split_state above); a
    maskrcnn_resnet50_fpn state also gives "mask_head" (mask.split_state) -- an entry that exists only when the state
    holds such keys; a keypointrcnn_resnet50_fpn state gives "keypoint_head" (keypoint.split_state) likewise"""
    from . import fpn, keypoint, mask
    backbone, neck = fpn.split_state(state)
    head, _ = rpn.split_state(state)
    box, _ = split_state(state)
    out = {"backbone": backbone, "neck": neck, "rpn": head, "box_head": box}
    mine, _ = mask.split_state(state)
    if mine:
        out["mask_head"] = mine
    mine, _ = keypoint.split_state(state)
    if mine:
        out["keypoint_head"] = mine
    return out


def generate_box_head_state(in_features: int, representation: int, classes: int, seed: int = 0, std=None) -> dict:
    """a seeded head: N(0, std) weights (default: 1 / sqrt(fan_in)) and small biases"""
    g = np.random.default_rng([seed, 0x424F58])
    out = {}
    for k, shape in head_shapes(in_features, representation, classes).items():
        scale = (std if std is not None else 1.0 / np.sqrt(shape[-1])) if k.endswith("weight") else 0.1
        out[k] = (g.standard_normal(shape) * scale).astype(F)
    return out


def box_head_ref(pooled, state, classes: int) -> np.ndarray:
    """TwoMLPHead + FastRCNNPredictor in float64 on pooled [K,a,PH,PW]: the [K,P] head output in the launches' layout"""
    st, _ = split_state(state)
    x = np.asarray(pooled, dtype=np.float64).reshape(np.shape(pooled)[0], -1)
    w = [np.asarray(st[k], dtype=np.float64) for k in HEAD_KEYS]
    x = np.maximum(x @ w[0].T + w[1], 0.0)
    x = np.maximum(x @ w[2].T + w[3], 0.0)
    out = np.zeros((x.shape[0], head_pitch(classes)))
    out[:, :classes] = x @ w[4].T + w[5]
    out[:, classes:5 * classes] = x @ w[6].T + w[7]
    return out


# ---- on the device -------------------------------------------------------------------------------------------
DET_SPEC = (("boxes", F, 4), ("scores", F, 1), ("labels", np.int32, 1), ("roi", np.int32, 1))
MID_SPEC = (("probs", F, 1), ("class_boxes", F, 4), ("valid", np.uint8, 1), ("keep", np.uint8, 1))


def output_spec(B: int, R: int, C: int, D: int, intermediates: bool = False) -> dict:
    """name -> (dtype, shape) of rn_detections for B images"""
    spec = {k: (t, (B, D) + ((4,) if n == 4 else ())) for k, t, n in DET_SPEC}
    spec["count"] = (np.int32, (B,))
    if intermediates:
        spec.update({k: (t, (B * R, C) + ((4,) if n == 4 else ())) for k, t, n in MID_SPEC})
    return spec


def make_request(bufs, score_thresh, nms_thresh, min_size, detections_per_img, weights):
    """the rn_detect_request over a mapping name -> object with .ptr (missing names are NULL)"""
    from . import _lib as L
    p = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
    return L.DetectRequest(float(score_thresh), float(nms_thresh), float(min_size), int(detections_per_img),
                           (L.c_float * 4)(*[float(v) for v in weights]),
                           L.Detections(*[p(k) for k in ("boxes", "scores", "labels", "roi", "count", "probs", "class_boxes",
                                                         "valid", "keep")]))


class BoxHead(Handle):
    """rn_box_head_*: TwoMLPHead (fc6, fc7 with ReLU) and FastRCNNPredictor as three contractions, then the three
    launches of the post-processing.  in_channels and resolution are the pooler's a and (PH, PW); state holds the eight
    tensors (split_state normalises the keys)."""
    DESTROY = "rn_box_head_destroy"

    def __init__(self, in_channels: int, resolution, representation: int, classes: int, state, score_thresh: float = 0.05,
                 nms_thresh: float = 0.5, detections_per_img: int = 100, bbox_reg_weights=BOX_WEIGHTS, min_size: float = MIN_SIZE,
                 ctx=None):
        import ctypes
        from . import _lib as L
        from .tensor import get_ctx
        self.ctx = ctx or get_ctx()
        res = (resolution, resolution) if np.ndim(resolution) == 0 else tuple(resolution)
        self.in_features = int(in_channels) * int(res[0]) * int(res[1])
        self.representation, self.classes, self.pitch = int(representation), int(classes), head_pitch(classes)
        self.score_thresh, self.nms_thresh, self.min_size = float(score_thresh), float(nms_thresh), float(min_size)
        self.detections_per_img, self.weights = int(detections_per_img), tuple(float(v) for v in bbox_reg_weights)
        self.handle = None
        self.poison = False   # buffers() fills every output with 0xA5 bytes first (tests: a row never written shows)
        h = ctypes.c_void_p()
        L.check(L.lib().rn_box_head_create(self.ctx.handle, ctypes.byref(h), self.in_features, self.representation, self.classes),
                "rn_box_head_create", self.ctx.handle)
        self.handle = h
        mine, _ = split_state(state)
        L.set_tensors(h, "rn_box_head", self.ctx, head_shapes(self.in_features, self.representation, self.classes), mine)

    def buffers(self, B: int, R: int, intermediates: bool = False):
        """device buffers of a forward of B images of R RoIs: (spec, buffers)"""
        from . import _lib as L
        from .tensor import _DeviceBuffer
        spec = output_spec(B, R, self.classes, self.detections_per_img, intermediates)
        bufs = {k: _DeviceBuffer(self.ctx, max(int(np.prod(sh)) * np.dtype(t).itemsize, 16)) for k, (t, sh) in spec.items()}
        if self.poison:
            for k, (t, sh) in spec.items():
                L.check(L.lib().rn_memset(self.ctx.handle, bufs[k].ptr, 0xA5, int(np.prod(sh)) * np.dtype(t).itemsize), "rn_memset",
                        self.ctx.handle)
        return spec, bufs

    def request(self, bufs):
        return make_request(bufs, self.score_thresh, self.nms_thresh, self.min_size, self.detections_per_img, self.weights)

    def collect(self, spec, bufs) -> dict:
        """downloads, padded as the device wrote them; "detections" is the count per image"""
        from .ops import _down_raw
        out = {k: _down_raw(bufs[k], t, int(np.prod(sh))).reshape(sh) for k, (t, sh) in spec.items()}
        out["detections"] = out.pop("count")
        out["detection_rois"] = out.pop("roi")
        return out

    def __call__(self, pooled, rois, B: int, image_size, intermediates: bool = False, return_head: bool = False) -> dict:
        """pooled [K,a,PH,PW] and rois [K,5] host arrays of B images (K = B*R): the stand-alone run.  Returns "boxes"
        [B,D,4], "scores", "labels", "detection_rois", "detections" [B]; with intermediates also "probs", "class_boxes",
        "valid", "keep"; with return_head also "head" [K,P]."""
        import ctypes
        from . import _lib as L
        from .ops import _down_raw, _up_raw
        from .tensor import _DeviceBuffer
        x = np.ascontiguousarray(pooled, dtype=F).reshape(np.shape(pooled)[0], -1)
        r = np.ascontiguousarray(rois, dtype=F).reshape(-1, 5)
        K = x.shape[0]
        assert x.shape[1] == self.in_features and r.shape[0] == K and K % B == 0, (x.shape, r.shape, B)
        dx, dr = _up_raw(x), _up_raw(r)
        spec, bufs = self.buffers(B, K // B, intermediates)
        head = _DeviceBuffer(self.ctx, max(K * self.pitch * 4, 16)) if return_head else None
        req = self.request(bufs)
        L.check(L.lib().rn_box_head_forward(self.handle, dx.ptr, dr.ptr, B, K // B, int(image_size[0]), int(image_size[1]),
                                            ctypes.byref(req), head.ptr if head else None), "rn_box_head_forward", self.ctx.handle)
        self.ctx.sync()
        out = self.collect(spec, bufs)
        if head:
            out["head"] = _down_raw(head, F, K * self.pitch).reshape(K, self.pitch)
        return out
