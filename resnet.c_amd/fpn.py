"""Feature pyramid on top of the backbone: torchvision's FeaturePyramidNetwork (the neck of resnet_fpn_backbone).

Key shapes (``fpn_shapes``), seeded weights (``generate_fpn_state``), the split of a torchvision detection state dict
(``split_state``), the float64 restatement of what the device computes (``fpn_ref``) and ``FeaturePyramidNetwork``,
the Python face of ``rn_fpn_*``.  ``NativeModel.forward_fpn`` runs a neck inside a forward: every lateral 1x1 right
behind its stage, the rest behind layer4.  ``ops.upsample_nearest_add`` is the top-down launch alone.  With RoIs and a
``roi.MultiScaleRoIAlign`` both forwards also pool the regions from the neck's own fp32 outputs (``rn_fpn_forward_rois``,
``rn_model_forward_rois``).
"""
from __future__ import annotations

import ctypes
import re
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from . import weights

EXTRA = {None: 0, "none": 0, "pool": 1}


def fpn_shapes(in_channels_list: Sequence[int], out_channels: int) -> Dict[str, Tuple[int, ...]]:
    """Key -> shape of torchvision's FeaturePyramidNetwork(in_channels_list, out_channels) with norm_layer=None, in
    the order of its state dict: every lateral 1x1 (inner_blocks), then every 3x3 (layer_blocks)."""
    a = int(out_channels)
    out: Dict[str, Tuple[int, ...]] = {}
    for i, c in enumerate(in_channels_list):
        out[f"inner_blocks.{i}.0.weight"] = (a, int(c), 1, 1)
        out[f"inner_blocks.{i}.0.bias"] = (a,)
    for i, _ in enumerate(in_channels_list):
        out[f"layer_blocks.{i}.0.weight"] = (a, a, 3, 3)
        out[f"layer_blocks.{i}.0.bias"] = (a,)
    return out


def generate_fpn_state(in_channels_list: Sequence[int], out_channels: int, seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded tensors of the neck under torchvision's keys, from the generator of weights.py: every convolution
    He-uniform over its fan-in, every bias uniform in +-0.1, every key with a name of its own in the generator."""
    tag = f"fpn{'_'.join(str(int(c)) for c in in_channels_list)}x{int(out_channels)}"
    out = {}
    for key, shape in fpn_shapes(in_channels_list, out_channels).items():
        if len(shape) == 4:
            bound = float(np.sqrt(6.0 / (shape[1] * shape[2] * shape[3])))
            out[key] = weights._uniform(f"{tag}.{key}", shape, -bound, bound, seed)
        else:
            out[key] = weights._uniform(f"{tag}.{key}", shape, -0.1, 0.1, seed)
    return out


_KEY = re.compile(r"^(inner_blocks|layer_blocks)\.(\d+)\.(?:0\.)?(weight|bias)$")


def split_state(state) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """A state dict that holds a torchvision FPN -> (backbone_state, fpn_state).  The neck's keys may carry the prefix
    "fpn." or "backbone.fpn." and either spelling, "inner_blocks.0.0.weight" (Conv2dNormActivation) or the older
    "inner_blocks.0.weight"; they come back as fpn_shapes spells them.  "backbone.body." / "body." keys come back
    without the prefix (the keys NativeModel reads); everything else (rpn.*, roi_heads.*, num_batches_tracked) is
    dropped.  A key that starts like a neck's and is not one raises ValueError."""
    backbone, neck = {}, {}
    for key, value in state.items():
        if key.endswith("num_batches_tracked"):
            continue
        arr = value.detach().cpu().numpy() if hasattr(value, "detach") else np.asarray(value)
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        k = key
        for prefix in ("backbone.fpn.", "fpn."):
            if k.startswith(prefix):
                k = k[len(prefix):]
                break
        if k.startswith(("inner_blocks.", "layer_blocks.")):
            m = _KEY.match(k)
            if not m:
                raise ValueError(f"{key!r}: not a key of torchvision's FeaturePyramidNetwork")
            neck[f"{m.group(1)}.{int(m.group(2))}.0.{m.group(3)}"] = arr
            continue
        for prefix in ("backbone.body.", "body."):
            if key.startswith(prefix):
                backbone[key[len(prefix):]] = arr
                break
    return backbone, neck


def fpn_ref(maps_nchw_f64, state, extra="pool", round_fn=None) -> Dict[str, np.ndarray]:
    """The neck in torch on the CPU, float64: maps [B,in_i,h_i,w_i], finest first -> {"0": [B,a,h_0,w_0], ..., "pool"}
    float64.  The top-down step gathers with ops.nearest_index, the index contract of
    rn_upsample_nearest_add_forward_dt.  round_fn (bf16 necks): applied to the maps, every convolution weight and
    every tensor the device stores in its element type -- the laterals and the merged tensors; the biases and the
    3x3 outputs (fp32 on the device) stay as they are."""
    import torch
    import torch.nn.functional as F

    from .ops import nearest_index
    rd = (lambda a: np.asarray(round_fn(np.asarray(a, dtype=np.float32)), dtype=np.float64)) if round_fn else (lambda a: a)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))  # noqa: E731
    n = len(maps_nchw_f64)
    out: Dict[str, np.ndarray] = {}
    with torch.no_grad():
        inner = []
        for i, x in enumerate(maps_nchw_f64):
            y = F.conv2d(t(rd(x)), t(rd(state[f"inner_blocks.{i}.0.weight"])), t(state[f"inner_blocks.{i}.0.bias"]))
            inner.append(rd(y.numpy()))
        for i in range(n - 2, -1, -1):
            H, W = inner[i].shape[2:]
            iy, ix = nearest_index(inner[i + 1].shape[2], H), nearest_index(inner[i + 1].shape[3], W)
            inner[i] = rd(inner[i] + inner[i + 1][:, :, iy][:, :, :, ix])
        for i in range(n):
            y = F.conv2d(t(inner[i]), t(rd(state[f"layer_blocks.{i}.0.weight"])), t(state[f"layer_blocks.{i}.0.bias"]),
                         padding=1)
            out[str(i)] = y.numpy()
    if EXTRA[extra]:
        out["pool"] = np.ascontiguousarray(out[str(n - 1)][:, :, ::2, ::2])
    return out


class NeckTail:
    """What runs behind a neck in one forward -- the pooler, the rpn, the box head, the mask head, the keypoint head --
    for both ``FeaturePyramidNetwork.forward`` and ``NativeModel.forward_fpn``.  Creating one raises the ValueErrors of
    a bad combination and touches no device; ``build`` makes the device buffers and the ctypes requests; ``entry`` names
    the entry point of the family that applies ("fpn", "rois", "proposals", "detections", "masks" or "keypoints") and
    ``requests`` what that one takes behind the levels; ``collect`` adds the results to the forward's dict once the
    context is synchronised."""

    def __init__(self, ctx, names, out_channels, B, image_size, rois, pooler, roi_levels, validate, rpn, candidates,
                 box_head, detect_intermediates, mask_head=None, masks=("probs",), mask_pooled=False, keypoint_head=None,
                 keypoints=("keypoints",)):
        if rpn is None and ((rois is None) != (pooler is None) or (rois is not None and image_size is None)):
            raise ValueError("rois, pooler and image_size go together")
        if rpn is not None and (image_size is None or (rois is not None and pooler is None)):
            raise ValueError("rpn needs image_size (and rois a pooler)")
        if box_head is not None and rpn is None:
            raise ValueError("box_head needs an rpn and a pooler")
        if box_head is not None and (pooler is None or rois is not None):
            raise ValueError("box_head needs a pooler that takes the proposals of the same call (no rois)")
        if mask_head is not None and box_head is None:
            raise ValueError("mask_head needs a box_head (and its rpn and pooler)")
        if keypoint_head is not None and box_head is None:
            raise ValueError("keypoint_head needs a box_head (and its rpn and pooler)")
        self.mask_head, self.masks, self.mask_pooled = mask_head, tuple(masks), bool(mask_pooled)
        self.keypoint_head, self.keypoints = keypoint_head, tuple(keypoints)
        self.ctx, self.names, self.a, self.B, self.image_size = ctx, names, int(out_channels), int(B), image_size
        self.rois, self.pooler, self.roi_levels, self.validate = rois, pooler, roi_levels, validate
        self.rpn, self.candidates, self.box_head, self.detect_intermediates = rpn, candidates, box_head, detect_intermediates
        self.entry = ("keypoints" if keypoint_head is not None else "masks" if mask_head is not None else
                      "detections" if box_head is not None else "proposals" if rpn is not None else
                      "rois" if pooler is not None else "fpn")
        self.req = self.rreq = self.dreq = self.mreq = self.kreq = None

    def build(self) -> None:
        from . import roi as R
        from .tensor import _DeviceBuffer
        if self.rpn is not None:
            self.rspec, self.rbufs = self.rpn.buffers(self.B, self.candidates)
            self.rreq = self.rpn.request(self.rbufs)
        if self.pooler is not None:
            if self.rois is None:  # the chain: the proposals of the same call, on the device
                self.drois, self.K = self.rbufs["rois"], self.B * self.rpn.post
            else:
                self.drois, self.K = R.upload_rois(self.rois, self.B, self.validate)
            PH, PW = self.pooler.output_size
            self.pooled = _DeviceBuffer(self.ctx, max(self.K * self.a * PH * PW * 4, 16))
            self.lv = _DeviceBuffer(self.ctx, max(self.K * 4, 16)) if self.roi_levels else None
            self.req = self.pooler.request(self.names, self.drois.ptr, self.K, self.image_size, self.pooled.ptr,
                                           self.lv.ptr if self.lv else None)
        if self.box_head is not None:
            self.dspec, self.dbufs = self.box_head.buffers(self.B, self.rpn.post, self.detect_intermediates)
            self.dreq = self.box_head.request(self.dbufs)
        if self.mask_head is not None:
            self.mspec, self.mbufs = self.mask_head.buffers(self.B, self.box_head.detections_per_img, self.image_size, self.masks,
                                                            rois=True, pooled=self.mask_pooled)
            self.mreq = self.mask_head.request(self.mbufs, self.names)
        if self.keypoint_head is not None:
            self.kspec, self.kbufs = self.keypoint_head.buffers(self.B, self.box_head.detections_per_img, self.keypoints)
            self.kreq = self.keypoint_head.request(self.kbufs, self.names)

    @property
    def requests(self) -> tuple:
        """The arguments of ``entry`` behind the levels, in the C order: req, rois, det_req, mask_req, kp_req."""
        ref = lambda r: ctypes.byref(r) if r is not None else None  # noqa: E731
        return {"fpn": (), "rois": (ref(self.req),), "proposals": (ref(self.rreq), ref(self.req)),
                "detections": (ref(self.rreq), ref(self.req), ref(self.dreq)),
                "masks": (ref(self.rreq), ref(self.req), ref(self.dreq), ref(self.mreq)),
                "keypoints": (ref(self.rreq), ref(self.req), ref(self.dreq), ref(self.mreq), ref(self.kreq))}[self.entry]

    def collect(self, out: dict) -> dict:
        from .ops import _down_raw
        if self.rpn is not None:
            got = self.rpn.collect(self.rspec, self.rbufs)
            out.update({k: got[k] for k in ("proposals", "scores", "proposal_levels", "cand") if k in got})
            out["rois"], out["proposal_count"], out["proposal_logits"] = got["raw"]["rois"], got["raw"]["count"], got["raw"]["logits"]
        if self.pooler is not None:
            PH, PW = self.pooler.output_size
            out["pooled"] = _down_raw(self.pooled, np.float32, self.K * self.a * PH * PW).reshape(self.K, self.a, PH, PW)
            if self.roi_levels:
                out["roi_levels"] = _down_raw(self.lv, np.int32, self.K)
        if self.box_head is not None:
            out["proposal_scores"] = out.pop("scores")
            out.update(self.box_head.collect(self.dspec, self.dbufs))
        if self.mask_head is not None:
            out.update(self.mask_head.collect(self.mspec, self.mbufs))
        if self.keypoint_head is not None:
            out.update(self.keypoint_head.collect(self.kspec, self.kbufs))
        return out


class FeaturePyramidNetwork(L.Handle):
    """rn_fpn_*: FeaturePyramidNetwork(in_channels_list, out_channels, extra_blocks=LastLevelMaxPool()) on the device
    (extra=None: no extra block); state holds torchvision's tensors (fpn_shapes; split_state normalises the keys).
    dtype "f32" or "bf16": storage of the input maps, the lateral tensors and the weight panels; the outputs are fp32
    either way."""
    DESTROY = "rn_fpn_destroy"

    def __init__(self, in_channels_list: Sequence[int], out_channels: int, state: Dict[str, np.ndarray],
                 extra: Optional[str] = "pool", dtype: str = "f32", ctx=None):
        from .tensor import get_ctx
        self.ctx = ctx or get_ctx()
        self.in_channels_list = tuple(int(c) for c in in_channels_list)
        self.out_channels, self.extra, self.dtype = int(out_channels), EXTRA[extra], dtype
        self.handle = None
        lib = L.lib()
        h = ctypes.c_void_p()
        cin = (ctypes.c_uint64 * max(len(self.in_channels_list), 1))(*self.in_channels_list)
        L.check(lib.rn_fpn_create(self.ctx.handle, ctypes.byref(h), len(self.in_channels_list), cin, self.out_channels,
                                  self.extra), "rn_fpn_create", self.ctx.handle)
        self.handle = h
        L.check(lib.rn_fpn_set_dtype(h, {"f32": L.RN_DTYPE_F32, "bf16": L.RN_DTYPE_BF16}[dtype]), "rn_fpn_set_dtype",
                self.ctx.handle)
        L.set_tensors(h, "rn_fpn", self.ctx, fpn_shapes(self.in_channels_list, self.out_channels), state)

    @property
    def names(self) -> Tuple[str, ...]:
        """torchvision's output names: "0" .. "n-1", then "pool" with the extra block."""
        return tuple(str(i) for i in range(len(self.in_channels_list))) + (("pool",) if self.extra else ())

    def level_shape(self, name: str, h_in: int, w_in: int) -> Tuple[int, int, int]:
        """(C, H, W) of output `name` when its level's map (for "pool": the coarsest level's) is h_in x w_in."""
        c, h, w = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        L.check(L.lib().rn_fpn_level_shape(self.handle, self.names.index(name), int(h_in), int(w_in), ctypes.byref(c),
                                           ctypes.byref(h), ctypes.byref(w)), "rn_fpn_level_shape", self.ctx.handle)
        return int(c.value), int(h.value), int(w.value)

    def forward(self, maps_nhwc, levels=None, *, rois=None, pooler=None, image_size=None, roi_levels: bool = False,
                validate: bool = True, rpn=None, candidates: bool = False, box_head=None,
                detect_intermediates: bool = False, mask_head=None, masks=("probs",),
                mask_pooled: bool = False, keypoint_head=None, keypoints=("keypoints",)) -> Dict[str, np.ndarray]:
        """maps_nhwc: one host array [B,h_i,w_i,in_i] fp32 per level, finest first (a bf16 neck rounds them on upload;
        uint16 bf16 bit patterns are taken as they are) -> {"0": [B,a,h_0,w_0] fp32, ..., "pool": ...}, the names in
        `levels` only (default: all).  With rois ([K,5] fp32: image index, x1, y1, x2, y2 in pixels of the input image),
        a pooler (roi.MultiScaleRoIAlign) and image_size (H, W): rn_fpn_forward_rois, which adds "pooled" [K,a,PH,PW]
        fp32 and, with roi_levels, "roi_levels" int32 [K]; levels may then be empty.  A RoI whose image index is no
        integer in [0, B) raises ValueError (validate=False hands it to the device, which answers zeros and level -1).
        With rpn (rpn.RegionProposalNetwork over all of the neck's outputs) and image_size: rn_fpn_forward_proposals,
        which adds per image "proposals", "scores", "proposal_levels" (and "cand" with candidates=True); with a pooler
        and no rois the pooler takes the proposals of the same call on the device: "pooled" is [B*post,a,PH,PW] and
        "rois" [B*post,5] comes with it.  With box_head (detection.BoxHead) behind that rpn and pooler (no rois):
        rn_fpn_forward_detections, which adds "boxes", "scores" (the proposals' go to "proposal_scores"), "labels",
        "detections" and "detection_rois" (and the intermediates with detect_intermediates).  With mask_head
        (mask.MaskHead) behind that box head: rn_fpn_forward_masks, which adds "mask_rois" [B*D,5] and, as `masks` names
        them ("probs", "image", "bits"), "mask_probs" [B,D,2M,2M], "masks" [B,D,H,W] fp32 and "mask_bits" [B,D,H,W] uint8
        (and "mask_pooled" [B*D,M,M,a] with mask_pooled).  With keypoint_head (keypoint.KeypointHead) behind that box
        head, with or without a mask head: rn_fpn_forward_keypoints, which adds, as `keypoints` names them ("keypoints",
        "heatmaps", "rois", "pooled"), "keypoints" [B,D,Kp,3] with "keypoints_scores" [B,D,Kp], "keypoint_heatmaps"
        [B,D,Kp,4M,4M], "keypoint_rois" [B*D,5] and "keypoint_pooled" [B*D,M,M,a].  Synchronous convenience."""
        from .ops import _down_raw, _up_raw, to_bf16_bits
        from .tensor import _DeviceBuffer
        n = len(self.in_channels_list)
        assert len(maps_nhwc) == n, (len(maps_nhwc), n)
        levels = self.names if levels is None else tuple(levels)
        for name in levels:
            if name not in self.names:
                raise ValueError(f"unknown level {name!r}: one of {self.names}")
        tail = NeckTail(self.ctx, self.names, self.out_channels, np.shape(maps_nhwc[0])[0], image_size, rois, pooler,
                        roi_levels, validate, rpn, candidates, box_head, detect_intermediates, mask_head, masks, mask_pooled,
                        keypoint_head, keypoints)
        xs = []
        for x, c in zip(maps_nhwc, self.in_channels_list):
            x = np.asarray(x)
            if self.dtype == "bf16":
                x = x if x.dtype == np.uint16 else to_bf16_bits(x).reshape(x.shape)
            else:
                x = np.ascontiguousarray(x, dtype=np.float32)
            assert x.ndim == 4 and x.shape[3] == c and x.shape[0] == np.shape(maps_nhwc[0])[0], (x.shape, c)
            xs.append(x)
        B = xs[0].shape[0]
        hs, ws = [x.shape[1] for x in xs], [x.shape[2] for x in xs]
        dx = [_up_raw(x) for x in xs]
        shapes, bufs = {}, {}
        for i, name in enumerate(self.names):
            j = min(i, n - 1)
            shapes[name] = (B,) + self.level_shape(name, hs[j], ws[j])
            if name in levels:
                bufs[name] = _DeviceBuffer(self.ctx, max(int(np.prod(shapes[name])) * 4, 16))
        xp = (ctypes.c_void_p * n)(*[d.ptr for d in dx])
        op = (ctypes.c_void_p * len(self.names))(*[bufs[name].ptr if name in bufs else None for name in self.names])
        hp, wp = (ctypes.c_uint64 * n)(*hs), (ctypes.c_uint64 * n)(*ws)
        tail.build()
        lib, size = L.lib(), tuple(int(s) for s in image_size) if image_size is not None else ()
        if tail.entry == "keypoints":
            st = lib.rn_fpn_forward_keypoints(self.handle, rpn.handle, box_head.handle, mask_head.handle if mask_head else None,
                                              keypoint_head.handle, xp, B, hp, wp, op, *size, *tail.requests)
        elif tail.entry == "masks":
            st = lib.rn_fpn_forward_masks(self.handle, rpn.handle, box_head.handle, mask_head.handle, xp, B, hp, wp, op, *size,
                                          *tail.requests)
        elif tail.entry == "detections":
            st = lib.rn_fpn_forward_detections(self.handle, rpn.handle, box_head.handle, xp, B, hp, wp, op, *size, *tail.requests)
        elif tail.entry == "proposals":
            st = lib.rn_fpn_forward_proposals(self.handle, rpn.handle, xp, B, hp, wp, op, *size, *tail.requests)
        elif tail.entry == "rois":
            st = lib.rn_fpn_forward_rois(self.handle, xp, B, hp, wp, op, *tail.requests)
        else:
            st = lib.rn_fpn_forward(self.handle, xp, B, hp, wp, op)
        L.check(st, "rn_fpn_forward" + {"fpn": ""}.get(tail.entry, "_" + tail.entry), self.ctx.handle)
        self.ctx.sync()
        out = {name: _down_raw(bufs[name], np.float32, int(np.prod(shapes[name]))).reshape(shapes[name])
               for name in self.names if name in bufs}
        return tail.collect(out)
