"""The keypoint head behind the box head (rn_keypoint.hip): torchvision's KeypointRCNNHeads, KeypointRCNNPredictor,
keypointrcnn_inference and heatmaps_to_keypoints in eval mode.

The contracts are those of include/rn_hip.h ("The keypoint head behind the box head").  Both halves of the predict
launch are bit-defined and restated here in numpy, every operation in fp32 and rounded on its own: the overlap-add of
the transposed convolution's panel with the 2x bilinear resize (heatmaps_ref) and the bicubic resize into the box with
its argmax (heatmaps_to_keypoints_ref).  The convolutions' sums are not: keypoint_head_ref is a float64 statement a
test holds the device to within a derived bound.

The *_ref functions are pure numpy and need no device.
"""
from __future__ import annotations

import numpy as np

from . import roi

F = np.float32
PREDICTOR_KEYS = ("keypoint_predictor.kps_score_lowres.weight", "keypoint_predictor.kps_score_lowres.bias")


# ---- the head's state ------------------------------------------------------------------------------------------
def _stem(i: int) -> str:
    return f"keypoint_head.{2 * i}."


def layer_keys(n_layers: int) -> tuple:
    """(weight key, bias key) of every 3x3 layer: KeypointRCNNHeads is a Sequential of (conv, ReLU) pairs, so layer i
    is "keypoint_head.{2i}." """
    return tuple((_stem(i) + "weight", _stem(i) + "bias") for i in range(int(n_layers)))


def head_shapes(in_channels: int, layers, keypoints: int) -> dict:
    """key -> shape of every tensor of KeypointRCNNHeads(in_channels, layers) and KeypointRCNNPredictor"""
    out, cin = {}, int(in_channels)
    for (kw, kb), c in zip(layer_keys(len(layers)), layers):
        out[kw], out[kb] = (int(c), cin, 3, 3), (int(c),)
        cin = int(c)
    out.update(zip(PREDICTOR_KEYS, ((cin, int(keypoints), 4, 4), (int(keypoints),))))
    return out


def _normal_key(key: str):
    """a keypoint key without the "roi_heads." prefix, or None for any other key"""
    import re
    k = key[len("roi_heads."):] if key.startswith("roi_heads.") else key
    if k in PREDICTOR_KEYS:
        return k
    m = re.fullmatch(r"keypoint_head\.(\d+)\.(weight|bias)", k)
    return k if m and int(m.group(1)) % 2 == 0 else None


def split_state(state) -> tuple:
    """(the keypoint head's tensors without the "roi_heads." prefix, the rest): takes both spellings"""
    return roi.split_state(state or {}, _normal_key)


def layers_of(state) -> tuple:
    """the layers' channel counts a state holds, from its 3x3 weights in order"""
    return roi.layer_widths(split_state(state)[0], _stem)


def generate_keypoint_head_state(in_channels: int, layers=(512,) * 8, keypoints: int = 17, seed: int = 0, prefix: str = "") -> dict:
    """a seeded head: N(0, sqrt(2 / fan_in)) weights (the activations keep their scale through the ReLUs) and small
    biases; the transposed convolution's weights N(0, 2 / sqrt(4 * Cin)) (an output sums at most four taps of Cin
    products each), so that the heat maps spread over a few units"""
    g = np.random.default_rng([seed, 0x4B5054])
    out = {}
    for k, shape in head_shapes(in_channels, layers, keypoints).items():
        if k.endswith("bias"):
            v = g.standard_normal(shape) * 0.1
        elif "kps_score_lowres" in k:
            v = g.standard_normal(shape) * 2.0 / np.sqrt(4.0 * shape[0])
        else:
            v = g.standard_normal(shape) * np.sqrt(2.0 / (shape[1] * 9))
        out[prefix + k] = v.astype(F)
    return out


# ---- the panel, the overlap-add and the 2x resize ----------------------------------------------------------------
def deconv_panel(weight) -> np.ndarray:
    """ConvTranspose2d(Cin, Kp, 4, stride 2, padding 1) as ONE 1x1 panel: rows [16*Kp, Cin] with row k*16 + ky*4 + kx =
    W[:, k, ky, kx].  The panel holds the products only; output (oy, ox) adds the taps with 2 iy = oy + 1 - ky and
    2 ix = ox + 1 - kx (heatmaps_ref)."""
    w = np.asarray(weight)
    cin, Kp = w.shape[:2]
    return np.ascontiguousarray(w.transpose(1, 2, 3, 0).reshape(16 * Kp, cin))


def _overlap_add(t, bias, dtype):
    """low [K, Kp, 2M, 2M] of `dtype` from the panel's output t [K, M, M, 16*Kp]: bias, then the valid taps in ascending
    ky, then ascending kx, each sum rounded on its own"""
    t = np.asarray(t, dtype=dtype)
    K, M = t.shape[0], t.shape[1]
    Kp = t.shape[3] // 16
    taps = t.reshape(K, M, M, Kp, 4, 4)
    low = np.empty((K, Kp, 2 * M, 2 * M), dtype)
    low[...] = np.asarray(bias, dtype=dtype).reshape(1, Kp, 1, 1)
    for ky in range(4):
        iy = np.array([i for i in range(M) if 0 <= 2 * i - 1 + ky < 2 * M], dtype=np.int64)
        for kx in range(4):
            ix = np.array([i for i in range(M) if 0 <= 2 * i - 1 + kx < 2 * M], dtype=np.int64)
            if iy.size == 0 or ix.size == 0:
                continue
            oy, ox = 2 * iy - 1 + ky, 2 * ix - 1 + kx
            v = taps[:, iy][:, :, ix][..., ky, kx].transpose(0, 3, 1, 2)  # [K, Kp, |iy|, |ix|]
            low[:, :, oy[:, None], ox[None, :]] = low[:, :, oy[:, None], ox[None, :]] + v
    return low


def _linear_axis(n_in: int, n_out: int, dtype):
    """rn_upsample_bilinear_forward's per-axis rule in `dtype`"""
    scale = dtype(n_in) / dtype(n_out)
    o = np.arange(n_out, dtype=np.int64).astype(dtype)
    src = np.maximum(scale * (o + dtype(0.5)) - dtype(0.5), dtype(0.0)).astype(dtype)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(dtype)).astype(dtype)
    return i0, i1, (dtype(1.0) - l1).astype(dtype), l1


def _resize2x(low, dtype):
    """[.., n, n] -> [.., 2n, 2n] by rn_upsample_bilinear_forward's rule and sum order in `dtype`"""
    n = low.shape[-1]
    y0, y1, a0, a1 = _linear_axis(n, 2 * n, dtype)
    x0, x1, b0, b1 = y0, y1, a0, a1
    r0, r1 = low[..., y0, :], low[..., y1, :]
    top = (b0 * r0[..., x0]).astype(dtype) + (b1 * r0[..., x1]).astype(dtype)
    bot = (b0 * r1[..., x0]).astype(dtype) + (b1 * r1[..., x1]).astype(dtype)
    out = (a0[:, None] * top).astype(dtype) + (a1[:, None] * bot).astype(dtype)
    assert out.dtype == dtype
    return out


def heatmaps_ref(t, bias, dtype=F) -> np.ndarray:
    """The first half of rn_keypoint_predict_forward's contract: the panel's output t [K, M, M, 16*Kp] and bias [Kp] ->
    heat [K, Kp, 4M, 4M]: the overlap-add of the transposed convolution, then interpolate(scale_factor=2, "bilinear",
    align_corners=False), every fp32 operation rounded on its own (dtype=np.float64: the same statement in float64)"""
    return np.ascontiguousarray(_resize2x(_overlap_add(t, bias, dtype), dtype))


# ---- the search ----------------------------------------------------------------------------------------------------
def _cubic_axis(n_in: int, n_out: int, dtype=F):
    """torch's cubic rule (A = -0.75) per axis n_in -> n_out in `dtype`: taps [n_out, 4] clamped to [0, n_in) and
    coefficients [n_out, 4]"""
    A = dtype(-0.75)
    scale = dtype(n_in) / dtype(n_out)
    o = np.arange(n_out, dtype=np.int64).astype(dtype)
    src = ((scale * (o + dtype(0.5))).astype(dtype) - dtype(0.5)).astype(dtype)
    fl = np.floor(src)
    tt = (src - fl).astype(dtype)
    i = fl.astype(np.int64)
    idx = np.clip(i[:, None] + np.arange(-1, 3, dtype=np.int64)[None, :], 0, n_in - 1)

    def outer(x):  # ((A*x - 5A)*x + 8A)*x - 4A
        return (((A * x - dtype(5.0) * A) * x + dtype(8.0) * A) * x - dtype(4.0) * A).astype(dtype)

    def inner(x):  # ((A+2)*x - (A+3))*x*x + 1
        return (((A + dtype(2.0)) * x - (A + dtype(3.0))) * x * x + dtype(1.0)).astype(dtype)

    cf = np.stack([outer(tt + dtype(1.0)), inner(tt), inner(dtype(1.0) - tt), outer(dtype(2.0) - tt)], axis=1)
    assert cf.dtype == dtype
    return idx, cf


def box_sizes_ref(boxes, max_size, labels=None):
    """(w, h fp32 [K], Wr, Hr int64 [K], live [K]): the contract's box sizes; a row that is OUT (a non-finite coordinate,
    a side over max_size = (max_h, max_w), a label below 1) has live False and sizes of 1"""
    b = np.asarray(boxes, dtype=F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        w = np.maximum(b[:, 2] - b[:, 0], F(1.0)).astype(F)
        h = np.maximum(b[:, 3] - b[:, 1], F(1.0)).astype(F)
        cw, ch = np.ceil(w), np.ceil(h)
        live = np.isfinite(b).all(axis=1) & (cw <= F(max_size[1])) & (ch <= F(max_size[0]))
    if labels is not None:
        live &= np.asarray(labels).reshape(-1) >= 1
    one = F(1.0)
    w, h = np.where(live, w, one).astype(F), np.where(live, h, one).astype(F)
    return w, h, np.where(live, cw, one).astype(np.int64), np.where(live, ch, one).astype(np.int64), live


def bicubic_resize_ref(heat, size, dtype=F) -> np.ndarray:
    """heat [.., S, S] resized bicubically (align_corners=False, torch's rule) to size = (Hr, Wr) in `dtype`: the row
    values over the columns first, then the same expression over the four row values"""
    x = np.asarray(heat, dtype=dtype)
    S = x.shape[-1]
    Hr, Wr = int(size[0]), int(size[1])
    xi, xc = _cubic_axis(S, Wr, dtype)
    yi, yc = _cubic_axis(S, Hr, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        rv = ((xc[:, 0] * x[..., xi[:, 0]] + xc[:, 1] * x[..., xi[:, 1]]) + xc[:, 2] * x[..., xi[:, 2]]) + xc[:, 3] * x[..., xi[:, 3]]
        c = yc[:, :, None]
        out = ((c[:, 0] * rv[..., yi[:, 0], :] + c[:, 1] * rv[..., yi[:, 1], :]) + c[:, 2] * rv[..., yi[:, 2], :]) + \
            c[:, 3] * rv[..., yi[:, 3], :]
    assert out.dtype == dtype
    return out


def argmax_ref(values) -> np.ndarray:
    """the contract's argmax over the last two axes, flat: the lowest index that holds the maximum, index 0 to start with
    and replaced only where v > best -- a NaN never replaces, a NaN at index 0 stays"""
    v = np.asarray(values)
    flat = v.reshape(v.shape[:-2] + (-1,))
    idx = np.where(np.isnan(flat), -np.inf, flat).argmax(axis=-1)
    return np.where(np.isnan(flat[..., 0]), 0, idx)


def heatmaps_to_keypoints_ref(heat, boxes, max_size, labels=None):
    """rn_heatmaps_to_keypoints_forward's contract: heat [K, Kp, S, S] fp32, boxes [K, 4], max_size = (max_h, max_w) ->
    (keypoints [K, Kp, 3], scores [K, Kp]) fp32, torchvision's heatmaps_to_keypoints with every fp32 operation rounded on
    its own; an OUT row answers zeros"""
    x = np.asarray(heat, dtype=F)
    K, Kp = x.shape[:2]
    b = np.asarray(boxes, dtype=F).reshape(K, 4)
    w, h, Wr, Hr, live = box_sizes_ref(b, max_size, labels)
    kps, scores = np.zeros((K, Kp, 3), F), np.zeros((K, Kp), F)
    for k in range(K):
        if not live[k]:
            continue
        r = bicubic_resize_ref(x[k], (Hr[k], Wr[k]))
        idx = argmax_ref(r)
        yi, xi = idx // Wr[k], idx % Wr[k]
        kps[k, :, 0] = ((xi.astype(F) + F(0.5)) * (w[k] / F(Wr[k]))).astype(F) + b[k, 0]
        kps[k, :, 1] = ((yi.astype(F) + F(0.5)) * (h[k] / F(Hr[k]))).astype(F) + b[k, 1]
        kps[k, :, 2] = F(1.0)
        scores[k] = r.reshape(Kp, -1)[np.arange(Kp), idx]
    return kps, scores


# ---- the float64 reference ---------------------------------------------------------------------------------------
def keypoint_head_ref(pooled_nchw, state, layers: bool = False):
    """KeypointRCNNHeads and KeypointRCNNPredictor in float64 on pooled [K, a, M, M]: heat [K, Kp, 4M, 4M].  layers=True:
    the list of every layer's output instead (the 3x3s as NCHW, then the heat maps)"""
    st, _ = split_state(state)
    outs = roi.tower_f64(pooled_nchw, st, _stem)
    rows = deconv_panel(np.asarray(st[PREDICTOR_KEYS[0]], dtype=np.float64))
    t = np.einsum("kchw,oc->khwo", outs[-1], rows, optimize=True)
    outs.append(heatmaps_ref(t, np.asarray(st[PREDICTOR_KEYS[1]], dtype=np.float64), np.float64))
    return outs if layers else outs[-1]


# ---- on the device -------------------------------------------------------------------------------------------
KEYPOINT_OUTPUTS = ("keypoints", "heatmaps", "rois", "pooled")


def output_spec(B: int, D: int, M: int, a: int, Kp: int, keypoints=("keypoints",)) -> dict:
    """name -> (dtype, shape) of the outputs of rn_keypoint_request a call wants: "keypoints" gives "keypoints" and
    "keypoints_scores", "heatmaps" gives "keypoint_heatmaps", "rois" and "pooled" the route's "keypoint_rois" and
    "keypoint_pooled" """
    for m in keypoints:
        if m not in KEYPOINT_OUTPUTS:
            raise ValueError(f"unknown keypoint output {m!r}: any of {KEYPOINT_OUTPUTS}")
    if "keypoints" not in keypoints and "heatmaps" not in keypoints:
        raise ValueError("keypoints must name at least one of 'keypoints' and 'heatmaps'")
    spec = {}
    if "rois" in keypoints:
        spec["keypoint_rois"] = (F, (B * D, 5))
    if "pooled" in keypoints:
        spec["keypoint_pooled"] = (F, (B * D, M, M, a))
    if "heatmaps" in keypoints:
        spec["keypoint_heatmaps"] = (F, (B, D, Kp, 4 * M, 4 * M))
    if "keypoints" in keypoints:
        spec["keypoints"] = (F, (B, D, Kp, 3))
        spec["keypoints_scores"] = (F, (B, D, Kp))
    return spec


class KeypointHead(roi.RoIHead):
    """rn_keypoint_head_*: KeypointRCNNHeads (3x3 convolutions with bias and ReLU), kps_score_lowres as one 1x1 panel of
    16 * Kp channels, then ONE predict launch: overlap-add, 2x bilinear, bicubic resize into the box and argmax.  state
    holds the head's tensors with or without the "roi_heads." prefix.  featmap_names, sampling_ratio: the keypoint pooler
    of a forward behind a neck."""
    NAME, DESTROY = "rn_keypoint_head", "rn_keypoint_head_destroy"

    def __init__(self, in_channels: int, layers=(512,) * 8, keypoints: int = 17, state=None, resolution: int = 14,
                 featmap_names=("0", "1", "2", "3"), sampling_ratio: int = 2, ctx=None):
        self.keypoints = int(keypoints)
        super().__init__(in_channels, layers, (self.keypoints,), resolution, featmap_names, sampling_ratio, head_shapes,
                         split_state(state)[0], ctx)

    def buffers(self, B: int, D: int, keypoints=("keypoints",)):
        """device buffers of a forward of B images of D detections: (spec, buffers)"""
        return self.alloc(output_spec(B, D, self.resolution, self.in_channels, self.keypoints, keypoints))

    def request(self, bufs, names=None):
        """the rn_keypoint_request over a mapping name -> object with .ptr (missing names are NULL); names: the level
        names of the neck the pooler reads (None: a stand-alone forward, which has no pooler)"""
        from . import _lib as L
        p = lambda k: bufs[k].ptr if k in bufs else None  # noqa: E731
        return L.KeypointRequest(*self.pool_fields(names), p("keypoint_rois"), p("keypoint_pooled"), p("keypoint_heatmaps"),
                                 p("keypoints"), p("keypoints_scores"))

    def __call__(self, pooled_nhwc, labels=None, boxes=None, image_size=None, keypoints=("keypoints",)) -> dict:
        """pooled_nhwc [K,M,M,a], labels [K] (or None: all valid) and boxes [K,4] host arrays: the stand-alone run.
        Returns "keypoints" [1,K,Kp,3] and "keypoints_scores" [1,K,Kp] (boxes and image_size = (max_h, max_w) given)
        and / or "keypoint_heatmaps" [1,K,Kp,4M,4M] as `keypoints` names them."""
        import ctypes
        from . import _lib as L
        from .ops import _up_raw
        x = np.ascontiguousarray(pooled_nhwc, dtype=F)
        K = x.shape[0]
        assert x.shape == (K, self.resolution, self.resolution, self.in_channels), x.shape
        dx = _up_raw(x)
        dl = _up_raw(np.ascontiguousarray(labels, dtype=np.int32).reshape(K)) if labels is not None else None
        db = _up_raw(np.ascontiguousarray(boxes, dtype=F).reshape(K, 4)) if boxes is not None else None
        size = image_size if image_size is not None else (1, 1)
        spec, bufs = self.buffers(1, K, keypoints)
        req = self.request(bufs)
        L.check(L.lib().rn_keypoint_head_forward(self.handle, dx.ptr, dl.ptr if dl else None, db.ptr if db else None, K,
                                                 int(size[0]), int(size[1]), ctypes.byref(req)), "rn_keypoint_head_forward",
                self.ctx.handle)
        self.ctx.sync()
        return self.collect(spec, bufs)
