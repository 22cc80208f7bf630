"""RPN proposals behind the head (rn_rpn.hip): torchvision's AnchorGenerator, BoxCoder.decode and filter_proposals.

The arithmetic is the contract of include/rn_hip.h ("RPN proposals behind the head"); this module restates it in
numpy -- every operation in fp32 and rounded on its own -- the way ops.roi_align_ref restates the pooler's.  The one
operation that is not bit-defined is the exponential of the decode: the device's expf and numpy's may differ in the
last place, so a test compares boxes within a bound (derived in tests/test_rpn_host.py) and everything behind them bit for bit on the
boxes the device itself returned.

The *_ref functions are pure numpy and need no device; filter_proposals runs the three launches.
"""
from __future__ import annotations

import numpy as np

from ._lib import Handle

F = np.float32
BBOX_XFORM_CLIP = F(np.log(1000.0 / 16.0))   # (float)log(1000.0 / 16.0)


# ---- anchors ------------------------------------------------------------------------------------------------
class AnchorGenerator:
    """torchvision's AnchorGenerator: sizes and aspect_ratios are one tuple per level; every level must have the
    same number of anchors per position."""

    def __init__(self, sizes=((32,), (64,), (128,), (256,), (512,)), aspect_ratios=(0.5, 1.0, 2.0)):
        sizes = tuple(tuple(s) if np.ndim(s) else (s,) for s in sizes)
        if np.ndim(aspect_ratios[0]) == 0:
            aspect_ratios = (tuple(aspect_ratios),) * len(sizes)
        aspect_ratios = tuple(tuple(r) for r in aspect_ratios)
        if len(sizes) != len(aspect_ratios):
            raise ValueError("sizes and aspect_ratios must have one entry per level")
        self.sizes, self.aspect_ratios = sizes, aspect_ratios
        counts = {len(s) * len(r) for s, r in zip(sizes, aspect_ratios)}
        if len(counts) != 1:
            raise ValueError(f"every level must have the same number of anchors per position, not {sorted(counts)}")

    def num_anchors_per_location(self) -> int:
        return len(self.sizes[0]) * len(self.aspect_ratios[0])

    def base_anchors(self) -> np.ndarray:
        """[L, A, 4] fp32: anchor (ratio i, size j) at index i * n_sizes + j is rint((-wr*s, -hr*s, wr*s, hr*s) / 2),
        hr = sqrtf(r), wr = 1 / hr, every operation fp32, rounding half to even."""
        out = []
        for sizes, ratios in zip(self.sizes, self.aspect_ratios):
            s, r = np.asarray(sizes, dtype=F), np.asarray(ratios, dtype=F)
            hr = np.sqrt(r)
            wr = F(1) / hr
            ws, hs = (wr[:, None] * s[None, :]).reshape(-1), (hr[:, None] * s[None, :]).reshape(-1)
            out.append(np.rint(np.stack([-ws, -hs, ws, hs], axis=1) / F(2)).astype(F))
        return np.stack(out)

    def grid_anchors(self, level_sizes, image_size) -> list:
        """One [h*w*A, 4] fp32 array per level: anchor n = (y*w + x)*A + a is base[a] + (x*sw, y*sh, x*sw, y*sh) with
        the strides sh = H // h and sw = W // w."""
        return grid_anchors(self.base_anchors(), level_sizes, image_size)


def grid_anchors(base, level_sizes, image_size) -> list:
    H, W = int(image_size[0]), int(image_size[1])
    out = []
    for b, (h, w) in zip(np.asarray(base, dtype=F), level_sizes):
        sh, sw = H // int(h), W // int(w)
        ys, xs = np.meshgrid(np.arange(h, dtype=np.int64) * sh, np.arange(w, dtype=np.int64) * sw, indexing="ij")
        shift = np.stack([xs, ys, xs, ys], axis=-1).reshape(-1, 1, 4).astype(F)
        out.append((shift + b[None, :, :]).reshape(-1, 4))
    return out


def head_channels(A: int) -> int:
    """P: 5 A rounded up to a multiple of 4"""
    return (5 * int(A) + 3) // 4 * 4


def pack_head(objectness, bbox_deltas) -> np.ndarray:
    """torchvision's RPNHead outputs of one level, objectness [B,A,h,w] and bbox_deltas [B,4A,h,w], as the NHWC
    [B,h,w,P] the launches read: channel a the logit of anchor a, channel A + 4a + c its delta c, zeros up to P."""
    o, d = np.asarray(objectness, dtype=F), np.asarray(bbox_deltas, dtype=F)
    B, A, h, w = o.shape
    assert d.shape == (B, 4 * A, h, w), (o.shape, d.shape)
    out = np.zeros((B, h, w, head_channels(A)), dtype=F)
    out[..., :A] = o.transpose(0, 2, 3, 1)
    out[..., A:5 * A] = d.transpose(0, 2, 3, 1)
    return out


def unpack_head(head, A: int):
    """(logits [B, h*w*A], deltas [B, h*w*A, 4]) of one level's [B,h,w,P], in anchor order"""
    head = np.asarray(head)
    B, h, w, _ = head.shape
    return head[..., :A].reshape(B, h * w * A), head[..., A:5 * A].reshape(B, h * w * A, 4)


def logit_of(score_thresh: float) -> float:
    """logit(score_thresh) as fp32: -inf at 0, +inf at 1"""
    p = float(score_thresh)
    if p <= 0.0:
        return float("-inf")
    if p >= 1.0:
        return float("inf")
    return float(F(np.log(p / (1.0 - p))))


# ---- the contract in numpy -------------------------------------------------------------------------------------
def select_ref(x, k: int) -> np.ndarray:
    """The indices of the min(k, n) first elements of the 1-D x in rn_topk_forward's order: (v_i, i) precedes (v_j, j)
    when v_i > v_j, or v_i == v_j and i < j; -0 == +0, a NaN ranks as -inf."""
    x = np.asarray(x, dtype=F).reshape(-1)
    v = np.where(np.isnan(x), F(-np.inf), x)
    return np.argsort(-v, kind="stable")[:int(k)].astype(np.int64)


def _fmin(a, b):   # the contract's min(a, b): a NaN in a stays
    return np.where(a > b, b, a)


def _fmax(a, b):
    return np.where(a < b, b, a)


def _decode(anchors, deltas, weights, image_size, ft, exp):
    a, d = np.asarray(anchors).astype(ft).reshape(-1, 4), np.asarray(deltas).astype(ft).reshape(-1, 4)
    wx, wy, ww, wh = (ft(F(v)) for v in weights)
    H, W = ft(F(image_size[0])), ft(F(image_size[1]))
    clip, half, zero = ft(BBOX_XFORM_CLIP), ft(0.5), ft(0)
    with np.errstate(all="ignore"):
        wa, ha = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        cx, cy = a[:, 0] + half * wa, a[:, 1] + half * ha
        dx, dy = d[:, 0] / wx, d[:, 1] / wy
        dw, dh = _fmin(d[:, 2] / ww, clip), _fmin(d[:, 3] / wh, clip)
        pcx, pcy = dx * wa + cx, dy * ha + cy
        pw, ph = exp(dw).astype(ft) * wa, exp(dh).astype(ft) * ha
        hw, hh = half * pw, half * ph
        out = np.stack([_fmin(_fmax(pcx - hw, zero), W), _fmin(_fmax(pcy - hh, zero), H),
                        _fmin(_fmax(pcx + hw, zero), W), _fmin(_fmax(pcy + hh, zero), H)], axis=1)
    return out.astype(ft)


def decode_ref(anchors, deltas, weights=(1.0, 1.0, 1.0, 1.0), image_size=(np.inf, np.inf)) -> np.ndarray:
    """BoxCoder.decode_single + clip_boxes_to_image in fp32, operation by operation; np.exp stands for the device's
    expf, so the result is the contract up to that one operation."""
    return _decode(anchors, deltas, weights, image_size, F, np.exp)


def decode_f64(anchors, deltas, weights=(1.0, 1.0, 1.0, 1.0), image_size=(np.inf, np.inf)) -> np.ndarray:
    """The same expressions in float64 on the fp32 inputs (the clip constant is the fp32 one)."""
    return _decode(anchors, deltas, weights, image_size, np.float64, np.exp)


def valid_ref(boxes, logits, min_size: float, logit_thresh: float) -> np.ndarray:
    """(x2 - x1 >= min_size) && (y2 - y1 >= min_size) && (logit >= logit_thresh) in fp32; a NaN anywhere fails"""
    b, lg = np.asarray(boxes, dtype=F).reshape(-1, 4), np.asarray(logits, dtype=F).reshape(-1)
    with np.errstate(all="ignore"):
        return (b[:, 2] - b[:, 0] >= F(min_size)) & (b[:, 3] - b[:, 1] >= F(min_size)) & (lg >= F(logit_thresh))


def iou_ref(box, boxes) -> np.ndarray:
    """inter / (area_i + area_j - inter) of one box against [n,4] boxes, fp32, the contract's order"""
    b, o = np.asarray(box, dtype=F), np.asarray(boxes, dtype=F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        area, areas = (b[2] - b[0]) * (b[3] - b[1]), (o[:, 2] - o[:, 0]) * (o[:, 3] - o[:, 1])
        iw = np.where(b[2] < o[:, 2], b[2], o[:, 2]) - np.where(b[0] > o[:, 0], b[0], o[:, 0])
        ih = np.where(b[3] < o[:, 3], b[3], o[:, 3]) - np.where(b[1] > o[:, 1], b[1], o[:, 1])
        inter = np.where(iw > 0, iw, F(0)) * np.where(ih > 0, ih, F(0))
        return (inter / (area + areas - inter)).astype(F)


def nms_ref(boxes, iou_threshold: float, valid=None) -> np.ndarray:
    """Greedy NMS of [n,4] fp32 boxes in their given order -> keep, bool [n].  An invalid box neither survives nor
    suppresses; box i survives if no surviving j < i has IoU > iou_threshold; 0/0 is a NaN and does not suppress."""
    b = np.asarray(boxes, dtype=F).reshape(-1, 4)
    n = b.shape[0]
    removed = np.zeros(n, bool) if valid is None else ~np.asarray(valid).reshape(-1).astype(bool)
    keep = np.zeros(n, bool)
    thr = F(iou_threshold)
    for i in range(n):
        if removed[i]:
            continue
        keep[i] = True
        if i + 1 < n:
            removed[i + 1:] |= iou_ref(b[i], b[i + 1:]) > thr
    return keep


def merge_ref(cand_logit, cand_box, keep, post_nms_top_n: int):
    """One image: cand_logit [L,pre], cand_box [L,pre,4], keep [L,pre] -> (boxes [post,4], logits [post], levels
    [post] int32, count): the survivors in the order of (logit, position = level * pre + rank), the first
    post_nms_top_n; rows at or past count hold boxes 0, logit -inf, level -1."""
    lg, bx, kp = np.asarray(cand_logit, dtype=F), np.asarray(cand_box, dtype=F), np.asarray(keep).astype(bool)
    L, pre = lg.shape
    pos = np.flatnonzero(kp.reshape(-1))
    order = pos[select_ref(lg.reshape(-1)[pos], post_nms_top_n)]
    post, cnt = int(post_nms_top_n), order.size
    boxes, logits, levels = np.zeros((post, 4), F), np.full(post, -np.inf, F), np.full(post, -1, np.int32)
    boxes[:cnt], logits[:cnt], levels[:cnt] = bx.reshape(-1, 4)[order], lg.reshape(-1)[order], (order // pre).astype(np.int32)
    return boxes, logits, levels, cnt


def rois_ref(boxes, count) -> np.ndarray:
    """[B*post, 5] in the pooler's format from boxes [B,post,4] and count [B]: the image index first, -1 on the rows
    at or past an image's count"""
    boxes = np.asarray(boxes, dtype=F)
    B, post, _ = boxes.shape
    idx = np.where(np.arange(post)[None, :] < np.asarray(count).reshape(B, 1), np.arange(B, dtype=F)[:, None], F(-1))
    return np.concatenate([idx.astype(F)[..., None], boxes], axis=2).reshape(B * post, 5)


def select_decode_ref(heads, base, image_size, pre_nms_top_n: int, min_size: float = 1e-3,
                      logit_thresh: float = -np.inf, boxes=None) -> dict:
    """rn_rpn_select_decode_forward's outputs from the heads [B,h,w,P] of L levels: index, logit, box, valid, count,
    padded like the device's.  boxes: [B,L,pre,4] to take in place of decode_ref's (the device's own, for a bit-for-bit
    check of valid)."""
    base = np.asarray(base, dtype=F)
    L, A = base.shape[:2]
    B, pre = heads[0].shape[0], int(pre_nms_top_n)
    anchors = grid_anchors(base, [hd.shape[1:3] for hd in heads], image_size)
    out = {"index": np.full((B, L, pre), -1, np.int32), "logit": np.full((B, L, pre), -np.inf, F),
           "box": np.zeros((B, L, pre, 4), F), "valid": np.zeros((B, L, pre), np.uint8), "count": np.zeros((B, L), np.int32)}
    for l, hd in enumerate(heads):
        logits, deltas = unpack_head(hd, A)
        for b in range(B):
            idx = select_ref(logits[b], pre)
            k = idx.size
            bx = decode_ref(anchors[l][idx], deltas[b][idx], image_size=image_size) if boxes is None else boxes[b, l, :k]
            out["index"][b, l, :k], out["logit"][b, l, :k], out["box"][b, l, :k] = idx, logits[b][idx], bx
            out["valid"][b, l, :k] = valid_ref(bx, logits[b][idx], min_size, logit_thresh)
            out["count"][b, l] = k
    return out


def nms_merge_ref(cand: dict, post_nms_top_n: int, nms_thresh: float) -> dict:
    """rn_rpn_nms_merge_forward's outputs from candidates (select_decode_ref's or the device's), bit-defined"""
    B, L, pre = cand["logit"].shape
    post = int(post_nms_top_n)
    out = {"boxes": np.zeros((B, post, 4), F), "logits": np.zeros((B, post), F), "levels": np.zeros((B, post), np.int32),
           "count": np.zeros(B, np.int32), "cand_keep": np.zeros((B, L, pre), np.uint8)}
    for b in range(B):
        for l in range(L):
            k = int(cand["count"][b, l])
            out["cand_keep"][b, l, :k] = nms_ref(cand["box"][b, l, :k], nms_thresh, cand["valid"][b, l, :k])
        out["boxes"][b], out["logits"][b], out["levels"][b], out["count"][b] = merge_ref(
            cand["logit"][b], cand["box"][b], out["cand_keep"][b], post)
    out["rois"] = rois_ref(out["boxes"], out["count"])
    return out


def filter_proposals_ref(heads, base, image_size, pre_nms_top_n: int = 1000, post_nms_top_n: int = 1000,
                         nms_thresh: float = 0.7, score_thresh: float = 0.0, min_size: float = 1e-3) -> dict:
    """torchvision's filter_proposals in the contract's fp32 (np.exp for expf): the candidates and the proposals"""
    cand = select_decode_ref(heads, base, image_size, pre_nms_top_n, min_size, logit_of(score_thresh))
    out = nms_merge_ref(cand, post_nms_top_n, nms_thresh)
    out["cand"] = cand
    return out


# ---- the head's state ------------------------------------------------------------------------------------------
HEAD_KEYS = ("head.conv.0.0.weight", "head.conv.0.0.bias", "head.cls_logits.weight", "head.cls_logits.bias",
             "head.bbox_pred.weight", "head.bbox_pred.bias")


def head_shapes(in_channels: int, A: int) -> dict:
    C = int(in_channels)
    return dict(zip(HEAD_KEYS, ((C, C, 3, 3), (C,), (A, C, 1, 1), (A,), (4 * A, C, 1, 1), (4 * A,))))


def split_state(state) -> tuple:
    """(the head's tensors under HEAD_KEYS, the rest): takes "rpn.head.*" with or without the "rpn." prefix and the
    older spelling "head.conv.weight|bias" of the 3x3"""
    mine, rest = {}, {}
    for k, v in state.items():
        key = k[4:] if k.startswith("rpn.") else k
        key = key.replace("head.conv.weight", "head.conv.0.0.weight").replace("head.conv.bias", "head.conv.0.0.bias")
        if key in HEAD_KEYS:
            mine[key] = v
        else:
            rest[k] = v
    return mine, rest


def generate_rpn_state(in_channels: int, A: int, seed: int = 0, std: float = 0.01) -> dict:
    """a seeded head: N(0, std) weights (torchvision's initialisation is std = 0.01) and small biases"""
    g = np.random.default_rng([seed, 0x52504E])
    out = {}
    for k, shape in head_shapes(in_channels, A).items():
        out[k] = (g.standard_normal(shape) * (std if k.endswith("weight") else 0.1)).astype(F)
    return out


def rpn_head_ref(features_nchw, state, A: int) -> list:
    """RPNHead in float64 on [B,C,h,w] levels: one [B,h,w,P] array per level in the launches' layout"""
    st, _ = split_state(state)
    w3, b3 = st[HEAD_KEYS[0]].astype(np.float64), st[HEAD_KEYS[1]].astype(np.float64)
    wp = np.concatenate([st[HEAD_KEYS[2]].reshape(A, -1), st[HEAD_KEYS[4]].reshape(4 * A, -1)]).astype(np.float64)
    bp = np.concatenate([st[HEAD_KEYS[3]], st[HEAD_KEYS[5]]]).astype(np.float64)
    out = []
    for x in features_nchw:
        x = np.asarray(x, dtype=np.float64)
        B, C, h, w = x.shape
        xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
        t = np.zeros((B, w3.shape[0], h, w))
        for dy in range(3):
            for dx in range(3):
                t += np.einsum("oc,bchw->bohw", w3[:, :, dy, dx], xp[:, :, dy:dy + h, dx:dx + w])
        t = np.maximum(t + b3[None, :, None, None], 0.0)
        hd = np.zeros((B, h, w, head_channels(A)))
        hd[..., :5 * A] = np.einsum("oc,bchw->bhwo", wp, t) + bp
        out.append(hd)
    return out


# ---- on the device -------------------------------------------------------------------------------------------
def sigmoid(x) -> np.ndarray:
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))).astype(F)


def filter_proposals(heads, anchor_generator, image_size, pre_nms_top_n: int = 1000, post_nms_top_n: int = 1000,
                     nms_thresh: float = 0.7, score_thresh: float = 0.0, min_size: float = 1e-3,
                     return_candidates: bool = False) -> dict:
    """The three launches behind an RPN head: heads is one host array [B,h,w,P] per level (pack_head), finest first;
    anchor_generator an AnchorGenerator or a base-anchor table [L,A,4]; image_size (H, W).  Returns per image
    "boxes" ([count_i, 4]), "scores" (the sigmoid of the logits, applied on the host), "logits", "levels"; "rois"
    [B*post, 5] as the pooler takes it; with return_candidates also "cand", the pre-NMS candidates."""
    from . import ops
    base = anchor_generator.base_anchors() if isinstance(anchor_generator, AnchorGenerator) else anchor_generator
    cand, out = ops.rpn_proposals(heads, base, image_size, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size,
                                  logit_of(score_thresh))
    cnt = out["count"]
    res = {"boxes": [out["boxes"][b, :c] for b, c in enumerate(cnt)], "logits": [out["logits"][b, :c] for b, c in enumerate(cnt)],
           "levels": [out["levels"][b, :c] for b, c in enumerate(cnt)], "rois": out["rois"], "count": cnt}
    res["scores"] = [sigmoid(v) for v in res["logits"]]
    if return_candidates:
        cand["keep"] = out["cand_keep"]
        res["cand"] = cand
    return res


class RegionProposalNetwork(Handle):
    """rn_rpn_*: torchvision's RegionProposalNetwork in eval mode on the device: RPNHead's two contractions per level,
    then select + decode, the IoU mask and scan + merge -- 2 L + 3 launches.  state holds the head's tensors
    (split_state normalises the keys); the anchor generator has one entry per level the network reads."""
    DESTROY = "rn_rpn_destroy"

    def __init__(self, in_channels: int, anchor_generator: AnchorGenerator, state, pre_nms_top_n: int = 1000,
                 post_nms_top_n: int = 1000, nms_thresh: float = 0.7, score_thresh: float = 0.0, min_size: float = 1e-3,
                 ctx=None):
        import ctypes
        from . import _lib as L
        from .tensor import get_ctx
        self.ctx = ctx or get_ctx()
        self.in_channels, self.anchors = int(in_channels), anchor_generator
        self.base = np.ascontiguousarray(anchor_generator.base_anchors())
        self.n_levels, self.A = self.base.shape[:2]
        self.pre, self.post = int(pre_nms_top_n), int(post_nms_top_n)
        self.nms_thresh, self.score_thresh, self.min_size = float(nms_thresh), float(score_thresh), float(min_size)
        self.handle = None
        self.poison = False   # buffers() fills every output with 0xA5 bytes first (tests: a row never written shows)
        h = ctypes.c_void_p()
        L.check(L.lib().rn_rpn_create(self.ctx.handle, ctypes.byref(h), self.in_channels, self.n_levels, self.A,
                                      self.base.ctypes.data_as(ctypes.POINTER(ctypes.c_float))), "rn_rpn_create", self.ctx.handle)
        self.handle = h
        mine, _ = split_state(state)
        L.set_tensors(h, "rn_rpn", self.ctx, head_shapes(self.in_channels, self.A), mine)

    def buffers(self, B: int, candidates: bool = False):
        """device buffers of a forward of B images: (spec, buffers) with spec name -> (dtype, shape)"""
        from .tensor import _DeviceBuffer
        n, pre, post = self.n_levels, self.pre, self.post
        spec = {"boxes": (F, (B, post, 4)), "logits": (F, (B, post)), "levels": (np.int32, (B, post)),
                "count": (np.int32, (B,)), "rois": (F, (B * post, 5)), "cand_keep": (np.uint8, (B, n, pre))}
        if candidates:
            spec.update({"cand_index": (np.int32, (B, n, pre)), "cand_logit": (F, (B, n, pre)), "cand_box": (F, (B, n, pre, 4)),
                         "cand_valid": (np.uint8, (B, n, pre)), "cand_count": (np.int32, (B, n))})
        bufs = {k: _DeviceBuffer(self.ctx, max(int(np.prod(sh)) * np.dtype(t).itemsize, 16)) for k, (t, sh) in spec.items()}
        if self.poison:
            from . import _lib as L
            for k, (t, sh) in spec.items():
                L.check(L.lib().rn_memset(self.ctx.handle, bufs[k].ptr, 0xA5, int(np.prod(sh)) * np.dtype(t).itemsize), "rn_memset",
                        self.ctx.handle)
        return spec, bufs

    def request(self, bufs):
        """the rn_rpn_request over buffers() (or any mapping name -> object with .ptr; missing names are NULL)"""
        from . import _lib as L
        p = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
        return L.RpnRequest(self.pre, self.post, self.nms_thresh, logit_of(self.score_thresh), self.min_size,
                            L.RpnProposals(p("boxes"), p("logits"), p("levels"), p("count"), p("rois"), p("cand_keep")),
                            L.RpnCandidates(p("cand_index"), p("cand_logit"), p("cand_box"), p("cand_valid"), p("cand_count")))

    def collect(self, spec, bufs) -> dict:
        """downloads: per-image "proposals", "scores" (the sigmoid, on the host), "proposal_levels"; "rois", "count",
        "logits" padded as the device wrote them; the candidates under "cand" when they were asked for"""
        from .ops import _down_raw
        raw = {k: _down_raw(bufs[k], t, int(np.prod(sh))).reshape(sh) for k, (t, sh) in spec.items()}
        cnt = raw["count"]
        out = {"proposals": [raw["boxes"][b, :c] for b, c in enumerate(cnt)],
               "scores": [sigmoid(raw["logits"][b, :c]) for b, c in enumerate(cnt)],
               "proposal_levels": [raw["levels"][b, :c] for b, c in enumerate(cnt)], "raw": raw}
        if "cand_index" in raw:
            out["cand"] = {k[5:]: raw[k] for k in raw if k.startswith("cand_") and k != "cand_keep"}
            out["cand"]["keep"] = raw["cand_keep"]
        return out

    def __call__(self, features, image_size, return_candidates: bool = False) -> dict:
        """features: name -> [B,C,h,w] fp32 host arrays (in the levels' order, finest first); the stand-alone run"""
        import ctypes
        from . import _lib as L
        from .ops import _up_raw
        maps = [np.ascontiguousarray(np.asarray(v, dtype=F).transpose(0, 2, 3, 1)) for v in features.values()]
        assert len(maps) == self.n_levels, (len(maps), self.n_levels)
        B, n = maps[0].shape[0], self.n_levels
        dx = [_up_raw(m) for m in maps]
        spec, bufs = self.buffers(B, return_candidates)
        req = self.request(bufs)
        L.check(L.lib().rn_rpn_forward(self.handle, (ctypes.c_void_p * n)(*[d.ptr for d in dx]), B,
                                       (ctypes.c_uint64 * n)(*[m.shape[1] for m in maps]),
                                       (ctypes.c_uint64 * n)(*[m.shape[2] for m in maps]), int(image_size[0]), int(image_size[1]),
                                       ctypes.byref(req)), "rn_rpn_forward", self.ctx.handle)
        self.ctx.sync()
        return self.collect(spec, bufs)
