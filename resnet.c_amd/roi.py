"""RoIAlign over the pyramid: torchvision's MultiScaleRoIAlign on the device's own maps.

``MultiScaleRoIAlign`` holds a pooler's parameters (the names of the levels it reads, the output size, the sampling
ratio, the canonical box); a neck's or a model's forward takes it with the RoIs and pools inside the same forward
(``FeaturePyramidNetwork.forward(..., rois=, pooler=, image_size=)``, ``NativeModel.forward_fpn(..., rois=, pooler=)``),
and calling it on a dict of host maps runs the launch alone (``ops.roi_align``).  ``infer_scales`` and ``boxes_to_rois``
are torchvision's ``infer_scale`` and ``convert_to_roi_format``; ``roi_align_f64`` is the float64 reference of the
arithmetic contract (``ops.roi_align_ref`` is its fp32 statement, which the kernel matches bit for bit).
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from . import ops


def infer_scales(level_sizes: Sequence[Tuple[int, int]], image_size: Tuple[int, int]) -> Tuple[float, ...]:
    """torchvision's infer_scale for every level: 2^round(log2(h / H)), the height's (torchvision forms the width's
    too and returns the first).  level_sizes: (h, w) per level; image_size: (H, W) of the input image."""
    H = int(image_size[0])
    return tuple(2.0 ** round(math.log2(float(h) / float(H))) for h, _ in level_sizes)


def boxes_to_rois(boxes: Sequence[np.ndarray]) -> np.ndarray:
    """torchvision's convert_to_roi_format: one [k_i,4] array of (x1, y1, x2, y2) per image -> [sum k_i, 5] fp32 with
    the image's index in front."""
    rows = []
    for i, b in enumerate(boxes):
        b = np.asarray(b, dtype=np.float32).reshape(-1, 4)
        rows.append(np.concatenate([np.full((b.shape[0], 1), i, dtype=np.float32), b], axis=1))
    return np.ascontiguousarray(np.concatenate(rows, axis=0) if rows else np.zeros((0, 5), np.float32))


def roi_align_f64(maps_nchw, rois, scales, output_size, sampling_ratio: int = 2, aligned: bool = False,
                  levels=None, thresholds=None) -> np.ndarray:
    """The contract of rn_roi_align_forward_dt in float64: maps_nchw one [B,C,h,w] array per level, finest first ->
    [K,C,PH,PW] float64.  levels: the level of every RoI (default: the kernel's own choice, ops.roi_levels_ref on the
    fp32 RoIs and thresholds -- the choice is part of the contract, not of the arithmetic)."""
    maps = [np.ascontiguousarray(np.asarray(m, dtype=np.float64).transpose(0, 2, 3, 1)) for m in maps_nchw]
    r32 = np.ascontiguousarray(rois, dtype=np.float32).reshape(-1, 5)
    if levels is None:
        thr = ops.roi_level_thresholds(scales) if thresholds is None else thresholds
        levels = ops.roi_levels_ref(r32, thr, images=maps[0].shape[0])
    return ops._roi_align_host(maps, r32.astype(np.float64), np.asarray(scales, dtype=np.float64), output_size,
                               sampling_ratio, aligned, levels, np.float64)


class MultiScaleRoIAlign:
    """torchvision.ops.MultiScaleRoIAlign(featmap_names, output_size, sampling_ratio, canonical_scale=224,
    canonical_level=4): the parameters of a pooler.  sampling_ratio must be 1..4 (the adaptive grid of
    sampling_ratio <= 0 is not carried)."""

    def __init__(self, featmap_names: Sequence[str], output_size, sampling_ratio: int, *, canonical_scale: float = 224.0,
                 canonical_level: int = 4, aligned: bool = False):
        self.featmap_names = tuple(str(n) for n in featmap_names)
        self.output_size = ((int(output_size), int(output_size)) if np.ndim(output_size) == 0
                            else (int(output_size[0]), int(output_size[1])))
        self.sampling_ratio, self.aligned = int(sampling_ratio), bool(aligned)
        self.canonical_scale, self.canonical_level = float(canonical_scale), int(canonical_level)
        if not self.featmap_names or len(self.featmap_names) > 4:
            raise ValueError("a pooler reads 1..4 levels")

    def level_indices(self, names: Sequence[str]) -> Tuple[int, ...]:
        """the pooler's levels as indices into a neck's level names; a name the neck has not, "pool" or a descending
        order raises ValueError"""
        names = tuple(names)
        idx = []
        for n in self.featmap_names:
            if n not in names or n == "pool":
                raise ValueError(f"the pooler reads level {n!r}: the neck has {tuple(x for x in names if x != 'pool')}")
            idx.append(names.index(n))
        if any(b <= a for a, b in zip(idx, idx[1:])):
            raise ValueError(f"the pooler's levels must ascend without repeats: {self.featmap_names}")
        return tuple(idx)

    def request(self, names, rois_ptr, K: int, image_size, pooled_ptr, levels_ptr=None) -> "L.RoiPool":
        """the rn_roi_pool of this pooler behind a neck whose levels are `names`"""
        idx = self.level_indices(names)
        return L.RoiPool(rois_ptr, int(K), int(image_size[0]), int(image_size[1]), len(idx),
                         (ctypes.c_int * 4)(*(idx + (0,) * (4 - len(idx)))), self.output_size[0], self.output_size[1],
                         self.sampling_ratio, int(self.aligned), self.canonical_scale, self.canonical_level, pooled_ptr,
                         levels_ptr)

    def thresholds(self, scales) -> np.ndarray:
        return ops.roi_level_thresholds(scales, self.canonical_scale, self.canonical_level)

    def __call__(self, features: Dict[str, np.ndarray], boxes, image_size, return_levels: bool = False):
        """The launch alone on host maps: features name -> [B,C,h,w] fp32 (NCHW, as a forward returns them); boxes one
        [k_i,4] array per image, or a [K,5] RoI array; image_size (H, W) -> [K,C,PH,PW] fp32."""
        maps = [np.asarray(features[n], dtype=np.float32) for n in self.featmap_names]
        rois = boxes_to_rois(boxes) if isinstance(boxes, (list, tuple)) else np.asarray(boxes, dtype=np.float32)
        scales = infer_scales([m.shape[2:] for m in maps], image_size)
        return ops.roi_align([np.ascontiguousarray(m.transpose(0, 2, 3, 1)) for m in maps], rois, scales, self.output_size,
                             self.sampling_ratio, self.aligned, self.thresholds(scales), return_levels)


def upload_rois(rois, images: int, validate: bool = True):
    """host RoIs [K,5] -> (device buffer, K); a RoI whose image index is no integer in [0, images) raises ValueError
    unless validate is False (the device then answers it with zeros and level -1)"""
    rois = np.ascontiguousarray(rois, dtype=np.float32).reshape(-1, 5)
    if validate and not ops.roi_image_valid(rois, images).all():
        raise ValueError(f"a RoI's image index is no integer in [0, {images})")
    return ops._up_raw(rois), rois.shape[0]


# ---- what the RoI heads behind the box head share (mask.py, keypoint.py): the tower of 3x3 layers --------------------
def split_state(state, normal_key) -> tuple:
    """(the tensors whose key normal_key knows, under the key it returns; the rest, for which it returns None)"""
    mine, rest = {}, {}
    for k, v in state.items():
        key = normal_key(k)
        if key is None:
            rest[k] = v
        else:
            mine[key] = v
    return mine, rest


def layer_widths(mine, stem) -> tuple:
    """the layers' channel counts a head's state holds, from its 3x3 weights stem(i) + "weight" in order"""
    out = []
    while stem(len(out)) + "weight" in mine:
        out.append(int(np.shape(mine[stem(len(out)) + "weight"])[0]))
    return tuple(out)


def conv3x3_f64(x, w, b):
    """x [K,C,H,W], w [O,C,3,3], b [O]: padding 1, float64"""
    K, C, H, W = x.shape
    xp = np.zeros((K, C, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    cols = np.stack([xp[:, :, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=2)  # [K,C,9,H,W]
    y = np.einsum("kcthw,oct->kohw", cols, w.reshape(w.shape[0], C, 9), optimize=True)
    return y + b[None, :, None, None]


def tower_f64(pooled_nchw, mine, stem) -> list:
    """every 3x3 layer's output (convolution, bias, ReLU) in float64 on pooled [K,a,M,M], for as many layers stem(i) as
    the state holds; the last one is what the head's transposed convolution reads"""
    x, outs = np.asarray(pooled_nchw, dtype=np.float64), []
    while stem(len(outs)) + "weight" in mine:
        w, b = (np.asarray(mine[stem(len(outs)) + leaf], dtype=np.float64) for leaf in ("weight", "bias"))
        x = np.maximum(conv3x3_f64(x, w, b), 0.0)
        outs.append(x)
    return outs


class RoIHead(L.Handle):
    """What MaskHead and KeypointHead are both: an object of the C library (NAME: "rn_mask_head") that reads pooled
    [K, M, M, in_channels] through `layers` 3x3 convolutions, with the pooler of a forward behind a neck."""
    NAME = ""

    def __init__(self, in_channels: int, layers, own, resolution: int, featmap_names, sampling_ratio: int, shapes, mine, ctx=None):
        """own: the head's own arguments of NAME_create, between layer_channels and resolution; shapes: key -> shape of
        every tensor (own already in it); mine: the tensors"""
        from .tensor import get_ctx
        self.ctx = ctx or get_ctx()
        self.in_channels, self.layers, self.resolution = int(in_channels), tuple(int(c) for c in layers), int(resolution)
        self.pooler = MultiScaleRoIAlign(featmap_names, self.resolution, sampling_ratio)
        self.handle = None
        self.poison = False   # alloc() fills every output with 0xA5 bytes first (tests: a row never written shows)
        h = ctypes.c_void_p()
        ch = (ctypes.c_uint64 * max(len(self.layers), 1))(*self.layers)
        create = self.NAME + "_create"
        L.check(getattr(L.lib(), create)(self.ctx.handle, ctypes.byref(h), self.in_channels, len(self.layers), ch, *own,
                                         self.resolution), create, self.ctx.handle)
        self.handle = h
        L.set_tensors(h, self.NAME, self.ctx, shapes(self.in_channels, self.layers, *own), mine)

    def alloc(self, spec):
        """device buffers of an output_spec: (spec, buffers)"""
        from .tensor import _DeviceBuffer
        bufs = {k: _DeviceBuffer(self.ctx, max(int(np.prod(sh)) * np.dtype(t).itemsize, 16)) for k, (t, sh) in spec.items()}
        if self.poison:
            for k, (t, sh) in spec.items():
                L.check(L.lib().rn_memset(self.ctx.handle, bufs[k].ptr, 0xA5, int(np.prod(sh)) * np.dtype(t).itemsize), "rn_memset",
                        self.ctx.handle)
        return spec, bufs

    def pool_fields(self, names) -> tuple:
        """the pooler's six fields in front of a head's request; names: the level names of the neck the pooler reads
        (None: a stand-alone forward, which has no pooler)"""
        idx = self.pooler.level_indices(names) if names is not None else ()
        return (len(idx), (ctypes.c_int * 4)(*(idx + (0,) * (4 - len(idx)))), self.pooler.sampling_ratio, int(self.pooler.aligned),
                self.pooler.canonical_scale, self.pooler.canonical_level)

    def collect(self, spec, bufs) -> dict:
        return {k: ops._down_raw(bufs[k], t, int(np.prod(sh))).reshape(sh) for k, (t, sh) in spec.items()}
