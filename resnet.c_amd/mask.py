"""The mask head behind the box head (rn_mask.hip): torchvision's MaskRCNNHeads, MaskRCNNPredictor, maskrcnn_inference
and paste_masks_in_image in eval mode.

The contracts are those of include/rn_hip.h ("The mask head behind the box head").  Two of them are bit-defined and
restated here in numpy, every operation in fp32 and rounded on its own: the RoI former (detection_rois_ref) and the
paste (expand_boxes_ref, paste_masks_ref).  The predictor's sum and its expf are not: mask_head_ref and predict_ref are
float64 statements a test holds the device to within a derived bound, and the model route is compared bit for bit with
the stand-alone run of the same device code.

The *_ref functions are pure numpy and need no device.
"""
from __future__ import annotations

import numpy as np

from . import roi

F = np.float32
PREDICTOR_KEYS = ("mask_predictor.conv5_mask.weight", "mask_predictor.conv5_mask.bias",
                  "mask_predictor.mask_fcn_logits.weight", "mask_predictor.mask_fcn_logits.bias")


# ---- the head's state ------------------------------------------------------------------------------------------
def _stem(i: int) -> str:
    return f"mask_head.{i}.0."


def layer_keys(n_layers: int, old: bool = False) -> tuple:
    """(weight key, bias key) of every 3x3 layer: torchvision's spelling since 0.13 ("mask_head.{i}.0.") or the one
    before it ("mask_head.mask_fcn{i+1}.")"""
    stem = (lambda i: f"mask_head.mask_fcn{i + 1}.") if old else _stem
    return tuple((stem(i) + "weight", stem(i) + "bias") for i in range(int(n_layers)))


def head_shapes(in_channels: int, layers, dim_reduced: int, classes: int, old: bool = False) -> dict:
    """key -> shape of every tensor of MaskRCNNHeads(in_channels, layers, dilation 1) and MaskRCNNPredictor"""
    out, cin = {}, int(in_channels)
    for (kw, kb), c in zip(layer_keys(len(layers), old), layers):
        out[kw], out[kb] = (int(c), cin, 3, 3), (int(c),)
        cin = int(c)
    Cr, C = int(dim_reduced), int(classes)
    out.update(zip(PREDICTOR_KEYS, ((cin, Cr, 2, 2), (Cr,), (C, Cr, 1, 1), (C,))))
    return out


def _normal_key(key: str):
    """a mask key without the "roi_heads." prefix and in the new spelling, or None for any other key"""
    import re
    k = key[len("roi_heads."):] if key.startswith("roi_heads.") else key
    if k in PREDICTOR_KEYS or re.fullmatch(r"mask_head\.\d+\.0\.(weight|bias)", k):
        return k
    m = re.fullmatch(r"mask_head\.mask_fcn(\d+)\.(weight|bias)", k)
    return f"mask_head.{int(m.group(1)) - 1}.0.{m.group(2)}" if m and int(m.group(1)) >= 1 else None


def split_state(state) -> tuple:
    """(the mask head's tensors under the new spelling's keys, the rest): takes both spellings, with or without the
    "roi_heads." prefix"""
    return roi.split_state(state, _normal_key)


def layers_of(state) -> tuple:
    """the layers' channel counts a state holds, from its 3x3 weights in order"""
    return roi.layer_widths(split_state(state)[0], _stem)


def generate_mask_head_state(in_channels: int, layers=(256,) * 4, dim_reduced: int = 256, classes: int = 91, seed: int = 0,
                             old: bool = False, prefix: str = "") -> dict:
    """a seeded head: N(0, sqrt(2 / fan_in)) weights (the activations keep their scale through the ReLUs) and small
    biases; the logits' weights N(0, 4 / sqrt(Cr)) so that the probabilities spread over (0, 1)"""
    g = np.random.default_rng([seed, 0x4D41534B])
    out = {}
    for k, shape in head_shapes(in_channels, layers, dim_reduced, classes, old).items():
        if k.endswith("bias"):
            v = g.standard_normal(shape) * 0.1
        elif "conv5_mask" in k:
            v = g.standard_normal(shape) * np.sqrt(2.0 / shape[0])
        elif "mask_fcn_logits" in k:
            v = g.standard_normal(shape) * 4.0 / np.sqrt(shape[1])
        else:
            v = g.standard_normal(shape) * np.sqrt(2.0 / (shape[1] * 9))
        out[prefix + k] = v.astype(F)
    return out


# ---- float64 references ----------------------------------------------------------------------------------------
def deconv_panel(weight, bias):
    """ConvTranspose2d(Cin, Cr, 2, 2) as ONE 1x1 panel: (rows [4*Cr, Cin], shift [4*Cr]) with row (dy*2+dx)*Cr + co =
    W[:, co, dy, dx] and the bias four times -- exact, kernel 2 at stride 2 overlaps nothing"""
    w = np.asarray(weight)
    cin, Cr = w.shape[:2]
    return np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(4 * Cr, cin)), np.tile(np.asarray(bias), 4)


def panel_to_nchw(t):
    """the panel's output t [K, M, M, 4*Cr] (channel (dy*2+dx)*Cr + c) as the transposed convolution's [K, Cr, 2M, 2M]"""
    t = np.asarray(t)
    K, M, _, c4 = t.shape
    Cr = c4 // 4
    return np.ascontiguousarray(t.reshape(K, M, M, 2, 2, Cr).transpose(0, 5, 1, 3, 2, 4).reshape(K, Cr, 2 * M, 2 * M))


def nchw_to_panel(x):
    """the inverse of panel_to_nchw: [K, Cr, 2M, 2M] -> [K, M, M, 4*Cr]"""
    x = np.asarray(x)
    K, Cr, Mo, _ = x.shape
    M = Mo // 2
    return np.ascontiguousarray(x.reshape(K, Cr, M, 2, M, 2).transpose(0, 2, 4, 3, 5, 1).reshape(K, M, M, 4 * Cr))


def mask_head_ref(pooled_nchw, state, layers: bool = False):
    """MaskRCNNHeads and conv5_mask with its ReLU in float64 on pooled [K,a,M,M]: [K,Cr,2M,2M], what mask_fcn_logits
    reads.  layers=True: the list of every layer's output instead (the 3x3s, then the transposed convolution)"""
    st, _ = split_state(state)
    outs = roi.tower_f64(pooled_nchw, st, _stem)
    rows, shift = deconv_panel(np.asarray(st[PREDICTOR_KEYS[0]], dtype=np.float64), np.asarray(st[PREDICTOR_KEYS[1]], dtype=np.float64))
    t = np.maximum(np.einsum("kchw,oc->khwo", outs[-1], rows, optimize=True) + shift, 0.0)
    outs.append(panel_to_nchw(t))
    return outs if layers else outs[-1]


def predict_ref(x_nchw, labels, weight, bias, return_logits: bool = False):
    """mask_fcn_logits, the sigmoid and maskrcnn_inference's gather in float64: x [K,Cr,Mo,Mo], labels [K], weight
    [C,Cr(,1,1)], bias [C] -> probs [K,Mo,Mo]; a row whose label is outside [1, C) is zeros (and its logits are)"""
    x = np.asarray(x_nchw, dtype=np.float64)
    w = np.asarray(weight, dtype=np.float64).reshape(np.shape(weight)[0], -1)
    b = np.asarray(bias, dtype=np.float64)
    lab = np.asarray(labels).astype(np.int64)
    ok = (lab >= 1) & (lab < w.shape[0])
    lc = np.clip(lab, 0, w.shape[0] - 1)
    z = np.einsum("kchw,kc->khw", x, w[lc], optimize=True) + b[lc][:, None, None]
    z[~ok] = 0.0
    p = 1.0 / (1.0 + np.exp(-z))
    p[~ok] = 0.0
    return (p, z) if return_logits else p


# ---- the bit-defined contracts in numpy ------------------------------------------------------------------------
def detection_rois_ref(boxes, labels) -> np.ndarray:
    """rn_detection_rois_forward: boxes [B,D,4], labels [B,D] -> rois [B*D,5]: (b, box) where label >= 1, else
    (-1, 0, 0, 0, 0)"""
    bx, lab = np.asarray(boxes, dtype=F), np.asarray(labels)
    B, D = lab.shape
    out = np.zeros((B, D, 5), F)
    real = lab >= 1
    out[..., 0] = np.where(real, np.arange(B, dtype=F)[:, None], F(-1.0))
    out[..., 1:] = np.where(real[..., None], bx.reshape(B, D, 4), F(0.0))
    return out.reshape(B * D, 5)


def expand_boxes_ref(boxes, Mo: int, labels=None):
    """torchvision's expand_boxes (scale (Mo + 2) / Mo) and the truncation to integers, in the contract's fp32:
    (int64 [K,4] of (bx0, by0, bx1, by1), live [K]); a dead row -- label < 1, a non-finite coordinate or expansion --
    has a box of zeros and pastes nothing"""
    b = np.asarray(boxes, dtype=F).reshape(-1, 4)
    s = F(float(Mo + 2) / float(Mo))
    with np.errstate(all="ignore"):
        wh = ((b[:, 2] - b[:, 0]) * F(0.5)) * s
        hh = ((b[:, 3] - b[:, 1]) * F(0.5)) * s
        xc = (b[:, 2] + b[:, 0]) * F(0.5)
        yc = (b[:, 3] + b[:, 1]) * F(0.5)
        e = np.stack([xc - wh, yc - hh, xc + wh, yc + hh], axis=1).astype(F)
    live = np.isfinite(b).all(axis=1) & np.isfinite(e).all(axis=1)
    if labels is not None:
        live &= np.asarray(labels).reshape(-1) >= 1
    e = np.where(live[:, None], np.clip(e, F(-2.0 ** 30), F(2.0 ** 30)), F(0.0))
    return np.trunc(e).astype(np.int64), live


def _paste_axis(lo: int, hi: int, origin: int, n_in: int, n_out: int):
    """rn_upsample_bilinear_forward's per-axis rule for the output indices lo - origin .. hi - origin - 1 of an axis
    resized from n_in to n_out: fp32 operations, each rounded on its own"""
    scale = F(n_in) / F(n_out)
    o = (np.arange(lo, hi, dtype=np.int64) - origin).astype(F)
    src = np.maximum(scale * (o + F(0.5)) - F(0.5), F(0.0)).astype(F)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(F)).astype(F)
    return i0, i1, (F(1.0) - l1).astype(F), l1


def paste_masks_ref(probs, boxes, image_size, labels=None) -> np.ndarray:
    """rn_paste_masks_forward's contract: probs [K,Mo,Mo] fp32, boxes [K,4] -> masks [K,H,W] fp32, torchvision's
    paste_masks_in_image with padding 1, every fp32 operation rounded on its own"""
    p = np.asarray(probs, dtype=F)
    K, Mo = p.shape[0], p.shape[1]
    H, W = int(image_size[0]), int(image_size[1])
    ib, live = expand_boxes_ref(boxes, Mo, labels)
    out = np.zeros((K, H, W), F)
    n = Mo + 2
    for k in range(K):
        if not live[k]:
            continue
        bx0, by0, bx1, by1 = (int(v) for v in ib[k])
        w, h = max(bx1 - bx0 + 1, 1), max(by1 - by0 + 1, 1)
        xs, xe, ys, ye = max(bx0, 0), min(bx1 + 1, W), max(by0, 0), min(by1 + 1, H)
        if xs >= xe or ys >= ye:
            continue
        pad = np.zeros((n, n), F)
        pad[1:-1, 1:-1] = p[k]
        y0, y1, a0, a1 = _paste_axis(ys, ye, by0, n, h)
        x0, x1, b0, b1 = _paste_axis(xs, xe, bx0, n, w)
        r0, r1 = pad[y0], pad[y1]
        top = (b0 * r0[:, x0]).astype(F) + (b1 * r0[:, x1]).astype(F)
        bot = (b0 * r1[:, x0]).astype(F) + (b1 * r1[:, x1]).astype(F)
        out[k, ys:ye, xs:xe] = (a0[:, None] * top).astype(F) + (a1[:, None] * bot).astype(F)
    return out


# ---- on the device -------------------------------------------------------------------------------------------
MASK_OUTPUTS = ("probs", "image", "bits")


def output_spec(B: int, D: int, M: int, a: int, image_size, masks=("probs",), rois: bool = False, pooled: bool = False) -> dict:
    """name -> (dtype, shape) of the outputs of rn_mask_request a call wants"""
    for m in masks:
        if m not in MASK_OUTPUTS:
            raise ValueError(f"unknown mask output {m!r}: any of {MASK_OUTPUTS}")
    if not masks:
        raise ValueError(f"masks must name at least one of {MASK_OUTPUTS}")
    spec = {}
    if rois:
        spec["mask_rois"] = (F, (B * D, 5))
    if pooled:
        spec["mask_pooled"] = (F, (B * D, M, M, a))
    if "probs" in masks:
        spec["mask_probs"] = (F, (B, D, 2 * M, 2 * M))
    if "image" in masks:
        spec["masks"] = (F, (B, D, int(image_size[0]), int(image_size[1])))
    if "bits" in masks:
        spec["mask_bits"] = (np.uint8, (B, D, int(image_size[0]), int(image_size[1])))
    return spec


class MaskHead(roi.RoIHead):
    """rn_mask_head_*: MaskRCNNHeads (3x3 convolutions with bias and ReLU), MaskRCNNPredictor's transposed convolution as
    one 1x1 panel, then the class-selected predict launch and the paste.  state holds the head's tensors in either
    spelling (split_state normalises the keys).  featmap_names, sampling_ratio: the mask pooler of a forward behind a
    neck."""
    NAME, DESTROY = "rn_mask_head", "rn_mask_head_destroy"

    def __init__(self, in_channels: int, layers=(256,) * 4, dim_reduced: int = 256, classes: int = 91, state=None,
                 resolution: int = 14, featmap_names=("0", "1", "2", "3"), sampling_ratio: int = 2, threshold: float = 0.5,
                 ctx=None):
        self.dim_reduced, self.classes, self.threshold = int(dim_reduced), int(classes), float(threshold)
        super().__init__(in_channels, layers, (self.dim_reduced, self.classes), resolution, featmap_names, sampling_ratio,
                         head_shapes, split_state(state)[0], ctx)

    def buffers(self, B: int, D: int, image_size, masks=("probs",), rois: bool = False, pooled: bool = False):
        """device buffers of a forward of B images of D detections: (spec, buffers)"""
        return self.alloc(output_spec(B, D, self.resolution, self.in_channels, image_size, masks, rois, pooled))

    def request(self, bufs, names=None):
        """the rn_mask_request over a mapping name -> object with .ptr (missing names are NULL); names: the level names
        of the neck the pooler reads (None: a stand-alone forward, which has no pooler)"""
        from . import _lib as L
        p = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
        return L.MaskRequest(*self.pool_fields(names), self.threshold, p("mask_rois"), p("mask_pooled"), p("mask_probs"), p("masks"),
                             p("mask_bits"))

    def __call__(self, pooled_nhwc, labels, boxes=None, image_size=None, masks=("probs",)) -> dict:
        """pooled_nhwc [K,M,M,a], labels [K] and boxes [K,4] host arrays: the stand-alone run.  Returns "mask_probs"
        [1,K,2M,2M] and, with boxes and image_size, "masks" / "mask_bits" [1,K,H,W] as `masks` names them."""
        import ctypes
        from . import _lib as L
        from .ops import _up_raw
        x = np.ascontiguousarray(pooled_nhwc, dtype=F)
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        K = x.shape[0]
        assert x.shape == (K, self.resolution, self.resolution, self.in_channels) and lab.size == K, (x.shape, lab.shape)
        dx, dl = _up_raw(x), _up_raw(lab)
        db = _up_raw(np.ascontiguousarray(boxes, dtype=F).reshape(K, 4)) if boxes is not None else None
        size = image_size if image_size is not None else (1, 1)
        spec, bufs = self.buffers(1, K, size, masks)
        req = self.request(bufs)
        L.check(L.lib().rn_mask_head_forward(self.handle, dx.ptr, dl.ptr, db.ptr if db else None, K, int(size[0]), int(size[1]),
                                             ctypes.byref(req)), "rn_mask_head_forward", self.ctx.handle)
        self.ctx.sync()
        return self.collect(spec, bufs)
