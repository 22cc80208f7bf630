"""Semantic segmentation on top of the backbone: torchvision's FCNHead, the bilinear upsample and the label map.

Pure-numpy / torch-on-CPU restatements of what the device computes (``upsample_bilinear_ref``, ``fcn_head_ref``),
seeded head weights (``generate_fcn_head_state``), the split of a torchvision ``fcn_resnet*`` state dict
(``split_state``), and ``FCNHead``, the Python face of ``rn_seg_head_*``.  ``NativeModel.forward_segment`` runs a
head right behind layer4 of a forward; ``ops.upsample_bilinear`` is the upsample launch alone.  The second half of
the file is the same for torchvision's DeepLabHead (``deeplab_head_shapes``, ``generate_deeplab_head_state``,
``deeplab_head_ref``, ``DeepLabHead``), the same device object with a longer table of convolutions.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import numpy as np

from . import _lib as L
from . import weights

HEAD_KEYS = ("classifier.0.weight", "classifier.1.weight", "classifier.1.bias", "classifier.1.running_mean",
             "classifier.1.running_var", "classifier.4.weight", "classifier.4.bias")


def head_shapes(in_channels: int, classes: int, mid_channels: Optional[int] = None) -> Dict[str, Tuple[int, ...]]:
    """Key -> shape of torchvision's FCNHead(in_channels, classes): mid_channels = in_channels // 4."""
    mid = in_channels // 4 if mid_channels is None else mid_channels
    return {"classifier.0.weight": (mid, in_channels, 3, 3), "classifier.1.weight": (mid,), "classifier.1.bias": (mid,),
            "classifier.1.running_mean": (mid,), "classifier.1.running_var": (mid,),
            "classifier.4.weight": (classes, mid, 1, 1), "classifier.4.bias": (classes,)}


# ---------------------------------------------------------------------------
# the contract of rn_upsample_bilinear_forward, in numpy
# ---------------------------------------------------------------------------
def _axis(n_in: int, n_out: int):
    """Index pair and weights of every output index along one axis: fp32 operations, each rounded on its own."""
    f32 = np.float32
    scale = f32(n_in) / f32(n_out)
    o = np.arange(n_out, dtype=np.float32)
    src = np.maximum(scale * (o + f32(0.5)) - f32(0.5), f32(0.0)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (f32(1.0) - l1).astype(np.float32)
    return i0, i1, l0, l1


def upsample_bilinear_ref(x_nhwc, size, classes: Optional[int] = None):
    """torch.nn.functional.interpolate(mode="bilinear", align_corners=False) of NHWC scores [B,h,w,C] to size =
    (H, W), with every operation rounded to fp32 on its own and no product fused into an add: the arithmetic
    rn_upsample_bilinear_forward is held to, bit for bit (include/rn_hip.h states it).  Only channels 0 ..
    classes-1 are read (classes = None: all).  Returns (scores [B,classes,H,W] fp32, labels [B,H,W] uint8): the label
    is numpy.argmax over the classes, the lowest index that holds the maximum."""
    x = np.asarray(x_nhwc, dtype=np.float32)
    B, h, w, C = x.shape
    classes = C if classes is None else int(classes)
    assert 1 <= classes <= min(C, 256), (classes, C)
    H, W = int(size[0]), int(size[1])
    y0, y1, a0, a1 = _axis(h, H)
    x0, x1, b0, b1 = _axis(w, W)
    v = x[..., :classes]
    b0, b1 = b0[None, None, :, None], b1[None, None, :, None]
    a0, a1 = a0[None, :, None, None], a1[None, :, None, None]
    r0, r1 = v[:, y0], v[:, y1]                                     # [B,H,w,classes]
    top = (b0 * r0[:, :, x0]).astype(np.float32) + (b1 * r0[:, :, x1]).astype(np.float32)
    bot = (b0 * r1[:, :, x0]).astype(np.float32) + (b1 * r1[:, :, x1]).astype(np.float32)
    out = (a0 * top).astype(np.float32) + (a1 * bot).astype(np.float32)
    assert out.dtype == np.float32
    labels = out.argmax(axis=3).astype(np.uint8)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)), labels


# ---------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------
def _draw_head_state(tag: str, shapes: Dict[str, Tuple[int, ...]], seed: int) -> Dict[str, np.ndarray]:
    """The draws of generate_fcn_head_state for every key of shapes; `{tag}.{key}` is the tensor's name in the
    generator."""
    out = {}
    for key, shape in shapes.items():
        name = f"{tag}.{key}"
        if key == "classifier.4.bias":
            out[key] = weights._uniform(name, shape, -0.02, 0.02, seed)
        elif len(shape) == 4:
            bound = float(np.sqrt(6.0 / (shape[1] * shape[2] * shape[3])))
            out[key] = weights._uniform(name, shape, -bound, bound, seed)
        elif key.endswith("running_var") or key.endswith(".weight"):
            out[key] = weights._uniform(name, shape, 0.5, 1.5, seed)
        else:
            out[key] = weights._uniform(name, shape, -0.1, 0.1, seed)
    return out


def generate_fcn_head_state(in_channels: int, classes: int, seed: int = 0,
                            mid_channels: Optional[int] = None) -> Dict[str, np.ndarray]:
    """Seeded tensors of FCNHead(in_channels, classes) under torchvision's keys, from the generator of weights.py:
    both convolutions He-uniform over their fan-in, the batch-norm as weights.generate_tensor draws one.  The
    classifier's bias is uniform in +-0.02: two orders below the spread the He-scaled 1x1 convolution gives the
    scores of an O(1) mid tensor, so that the bias never decides a label (a bias-dominated fixture makes
    every top-1 assert vacuous)."""
    return _draw_head_state(f"fcn{in_channels}x{classes}", head_shapes(in_channels, classes, mid_channels), seed)


def split_state(state) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """A torchvision fcn_resnet* or deeplabv3_resnet* state dict -> (backbone_state, head_state): "backbone." is
    stripped (the keys NativeModel reads), "classifier." is kept (the keys FCNHead or DeepLabHead reads),
    "aux_classifier." is dropped, and so are
    the batch-norms' num_batches_tracked.  A segmentation backbone has no fc: when fc.* is absent a zero classifier
    of 4 rows is supplied, so that NativeModel finalizes (its logits are then zeros)."""
    backbone, head = {}, {}
    for key, value in state.items():
        if key.endswith("num_batches_tracked") or key.startswith("aux_classifier."):
            continue
        arr = value.detach().cpu().numpy() if hasattr(value, "detach") else np.asarray(value)
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        if key.startswith("backbone."):
            backbone[key[len("backbone."):]] = arr
        elif key.startswith("classifier."):
            head[key] = arr
        else:
            raise ValueError(f"{key!r}: not a key of a torchvision fcn_resnet* state dict")
    if "fc.weight" not in backbone:
        first = "classifier.0.weight" if "classifier.0.weight" in head else "classifier.0.convs.0.0.weight"
        feat = int(head[first].shape[1])
        backbone["fc.weight"] = np.zeros((4, feat), dtype=np.float32)
        backbone["fc.bias"] = np.zeros((4,), dtype=np.float32)
    return backbone, head


def fcn_head_ref(x_nchw_f64, state, size, round_fn=None) -> np.ndarray:
    """FCNHead + interpolate in torch on the CPU, float64: x [B,in,h,w] -> scores [B,classes,H,W] float64.
    round_fn (bf16 heads): applied to the map, both convolution weights and the mid tensor, where the device
    rounds to its storage type; the batch-norm constants and the bias stay as they are."""
    import torch
    import torch.nn.functional as F

    rd = (lambda a: np.asarray(round_fn(np.asarray(a, dtype=np.float32)), dtype=np.float64)) if round_fn else (lambda a: a)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))  # noqa: E731
    with torch.no_grad():
        y = F.conv2d(t(rd(x_nchw_f64)), t(rd(state["classifier.0.weight"])), padding=1)
        y = F.batch_norm(y, t(state["classifier.1.running_mean"]), t(state["classifier.1.running_var"]),
                         t(state["classifier.1.weight"]), t(state["classifier.1.bias"]), training=False, eps=1e-5)
        y = torch.relu(y)
        if round_fn:
            y = t(rd(y.numpy()))
        y = F.conv2d(y, t(rd(state["classifier.4.weight"])), t(state["classifier.4.bias"]))
        y = F.interpolate(y, size=(int(size[0]), int(size[1])), mode="bilinear", align_corners=False)
    return y.numpy()


# ---------------------------------------------------------------------------
# the device head
# ---------------------------------------------------------------------------
class FCNHead(L.Handle):
    """rn_seg_head_*: FCNHead(in_channels, classes) with mid = in_channels // 4 on the device; state holds
    torchvision's seven tensors (HEAD_KEYS).  dtype "f32" or "bf16": storage of the input map, the mid tensor and
    the weight panels; the coarse scores and the outputs are fp32 either way.  mid_channels: another width than
    torchvision's in_channels // 4."""
    DESTROY = "rn_seg_head_destroy"

    def __init__(self, in_channels: int, classes: int, state: Dict[str, np.ndarray], dtype: str = "f32", ctx=None,
                 mid_channels: Optional[int] = None):
        mid = int(in_channels) // 4 if mid_channels is None else int(mid_channels)
        self._build(in_channels, mid, classes, dtype, ctx, state, head_shapes(in_channels, classes, mid),
                    "rn_seg_head_create", mid, int(classes))

    def _build(self, in_channels, mid_channels, classes, dtype, ctx, state, shapes, create, *create_args):
        """the head of either kind: `create`(ctx, &handle, in_channels, *create_args), its dtype, the tensors of shapes
        from state, finalize"""
        from .tensor import get_ctx
        self.handle = None                                   # close() is safe whatever fails below
        self.ctx = ctx or get_ctx()
        self.in_channels, self.mid_channels, self.classes, self.dtype = int(in_channels), int(mid_channels), int(classes), dtype
        lib = L.lib()
        h = ctypes.c_void_p()
        L.check(getattr(lib, create)(self.ctx.handle, ctypes.byref(h), self.in_channels, *create_args), create,
                self.ctx.handle)
        self.handle = h
        L.check(lib.rn_seg_head_set_dtype(h, {"f32": L.RN_DTYPE_F32, "bf16": L.RN_DTYPE_BF16}[dtype]),
                "rn_seg_head_set_dtype", self.ctx.handle)
        L.set_tensors(h, "rn_seg_head", self.ctx, shapes, state)

    def forward(self, x_nhwc, size, scores: bool = True, labels: bool = False):
        """x_nhwc: host array [B,h,w,in_channels] fp32 (a bf16 head rounds it on upload; uint16 bf16 bit patterns
        are taken as they are) -> (scores [B,classes,H,W] fp32 or None, labels [B,H,W] uint8 or None) at size =
        (H, W).  Synchronous convenience."""
        from .ops import _down_raw, _up_raw, to_bf16_bits
        from .tensor import _DeviceBuffer
        x = np.asarray(x_nhwc)
        if self.dtype == "bf16":
            x = x if x.dtype == np.uint16 else to_bf16_bits(x).reshape(x.shape)
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
        B, h, w, C = x.shape
        assert C == self.in_channels, (x.shape, self.in_channels)
        H, W = int(size[0]), int(size[1])
        dx = _up_raw(x)
        ds = _DeviceBuffer(self.ctx, max(B * self.classes * H * W * 4, 16)) if scores else None
        dl = _DeviceBuffer(self.ctx, max(B * H * W, 16)) if labels else None
        L.check(L.lib().rn_seg_head_forward(self.handle, dx.ptr, B, h, w, H, W, ds.ptr if ds else None,
                                            dl.ptr if dl else None), "rn_seg_head_forward", self.ctx.handle)
        self.ctx.sync()
        s = _down_raw(ds, np.float32, B * self.classes * H * W).reshape(B, self.classes, H, W) if scores else None
        lb = _down_raw(dl, np.uint8, B * H * W).reshape(B, H, W) if labels else None
        return s, lb


# ---------------------------------------------------------------------------
# DeepLabV3: torchvision's DeepLabHead (ASPP + Conv3x3 + Conv1x1), an rn_seg_head from rn_seg_head_create_deeplab
# ---------------------------------------------------------------------------
DEEPLAB_RATES = (12, 24, 36)
_BN = ("weight", "bias", "running_mean", "running_var")


def deeplab_head_shapes(in_channels: int, classes: int, aspp_channels: int = 256,
                        rates=DEEPLAB_RATES) -> Dict[str, Tuple[int, ...]]:
    """Key -> shape of torchvision's DeepLabHead(in_channels, classes) with ASPP(in_channels, rates, aspp_channels),
    in the order of its state dict (num_batches_tracked left out).  convs.0 is the 1x1 branch, convs.1..n the
    dilated 3x3 branches, convs.(n+1) the pooled branch, whose Sequential starts with the pool: its convolution is
    .1 and its batch-norm .2."""
    a, n = int(aspp_channels), len(rates)
    out: Dict[str, Tuple[int, ...]] = {}

    def unit(conv: str, norm: str, cin: int, k: int):
        out[f"{conv}.weight"] = (a, cin, k, k)
        for name in _BN:
            out[f"{norm}.{name}"] = (a,)

    unit("classifier.0.convs.0.0", "classifier.0.convs.0.1", in_channels, 1)
    for i in range(1, n + 1):
        unit(f"classifier.0.convs.{i}.0", f"classifier.0.convs.{i}.1", in_channels, 3)
    unit(f"classifier.0.convs.{n + 1}.1", f"classifier.0.convs.{n + 1}.2", in_channels, 1)
    unit("classifier.0.project.0", "classifier.0.project.1", (n + 2) * a, 1)
    unit("classifier.1", "classifier.2", a, 3)
    out["classifier.4.weight"] = (int(classes), a, 1, 1)
    out["classifier.4.bias"] = (int(classes),)
    return out


def generate_deeplab_head_state(in_channels: int, classes: int, aspp_channels: int = 256, rates=DEEPLAB_RATES,
                                seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded tensors of DeepLabHead under torchvision's keys: the draws of generate_fcn_head_state (convolutions
    He-uniform over their fan-in, batch-norms as there, the classifier's bias in +-0.02), every key with a name of
    its own in the generator."""
    tag = f"deeplab{in_channels}x{aspp_channels}x{classes}r{'_'.join(str(int(r)) for r in rates)}"
    return _draw_head_state(tag, deeplab_head_shapes(in_channels, classes, aspp_channels, rates), seed)


def deeplab_head_ref(x_nchw_f64, state, size, rates=DEEPLAB_RATES, round_fn=None) -> np.ndarray:
    """DeepLabHead + interpolate in torch on the CPU, float64: x [B,in,h,w] -> scores [B,classes,H,W] float64.  The
    pooled branch is broadcast (what bilinear interpolation from a 1x1 map gives).  round_fn (bf16 heads): applied
    to the map, every convolution weight and every tensor the device stores in its element type -- the branch
    outputs, the pooled mean, the pooled branch, the projected tensor and the 3x3's output; the batch-norm constants
    and the bias stay as they are."""
    import torch
    import torch.nn.functional as F

    rd = (lambda a: np.asarray(round_fn(np.asarray(a, dtype=np.float32)), dtype=np.float64)) if round_fn else (lambda a: a)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))  # noqa: E731
    n = len(rates)

    def unit(y, conv, norm, **kw):
        """convolution + batch-norm + ReLU, stored"""
        y = F.conv2d(y, t(rd(state[f"{conv}.weight"])), **kw)
        y = F.batch_norm(y, t(state[f"{norm}.running_mean"]), t(state[f"{norm}.running_var"]), t(state[f"{norm}.weight"]),
                         t(state[f"{norm}.bias"]), training=False, eps=1e-5)
        y = torch.relu(y)
        return t(rd(y.numpy())) if round_fn else y

    with torch.no_grad():
        x = t(rd(x_nchw_f64))
        outs = [unit(x, "classifier.0.convs.0.0", "classifier.0.convs.0.1")]
        for i, r in enumerate(rates, start=1):
            outs.append(unit(x, f"classifier.0.convs.{i}.0", f"classifier.0.convs.{i}.1", padding=int(r), dilation=int(r)))
        pooled = x.mean(dim=(2, 3), keepdim=True)
        if round_fn:
            pooled = t(rd(pooled.numpy()))
        pooled = unit(pooled, f"classifier.0.convs.{n + 1}.1", f"classifier.0.convs.{n + 1}.2")
        outs.append(pooled.expand(-1, -1, x.shape[2], x.shape[3]))
        y = unit(torch.cat(outs, dim=1), "classifier.0.project.0", "classifier.0.project.1")
        y = unit(y, "classifier.1", "classifier.2", padding=1)
        y = F.conv2d(y, t(rd(state["classifier.4.weight"])), t(state["classifier.4.bias"]))
        y = F.interpolate(y, size=(int(size[0]), int(size[1])), mode="bilinear", align_corners=False)
    return y.numpy()


class DeepLabHead(FCNHead):
    """rn_seg_head_create_deeplab: DeepLabHead(in_channels, classes) with ASPP(in_channels, rates, aspp_channels) on
    the device; state holds torchvision's tensors (deeplab_head_shapes).  forward, close and the attributes are
    FCNHead's (mid_channels is the ASPP width); dtype "f32" or "bf16" as there.  center_tap(on) switches the
    centre-tap plan (default on): a dilated branch whose rate is at least the map's height and width runs as the 1x1
    contraction on its centre tap -- the same bits, a ninth of the FLOPs (every bf16 head; an fp32 head only at
    in_channels == 64, see include/rn_hip.h)."""

    def __init__(self, in_channels: int, classes: int, state: Dict[str, np.ndarray], aspp_channels: int = 256,
                 rates=DEEPLAB_RATES, dtype: str = "f32", ctx=None):
        self.aspp_channels, self.rates = int(aspp_channels), tuple(int(r) for r in rates)
        rates_c = (ctypes.c_uint64 * len(self.rates))(*self.rates)
        self._build(in_channels, self.aspp_channels, classes, dtype, ctx, state,
                    deeplab_head_shapes(in_channels, classes, self.aspp_channels, self.rates),
                    "rn_seg_head_create_deeplab", self.aspp_channels, int(classes), len(self.rates), rates_c)

    def center_tap(self, on: bool) -> None:
        L.check(L.lib().rn_seg_head_set_center_tap(self.handle, int(bool(on))), "rn_seg_head_set_center_tap", self.ctx.handle)
