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
