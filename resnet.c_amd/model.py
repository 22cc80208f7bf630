"""The model graph, twice.

``ResnetModel`` / ``createResnet`` / ``resnetForward`` mirror the reference
driver cuda/inference/main.cu:7-226 object for object on top of the nn layer
wrappers (one C-ABI call per reference op, NCHW tensors, lazily cached
activations) -- the literal drop-in for code written against ops/nn/tensor.

``NativeModel`` wraps the plain-C driver inside librn_hip.so (rn_model.c): NHWC
engine layout, packed weights, optional fused epilogues, no Python in the loop.
It is what bench.py times.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib as L
from . import nn, weights
from .tensor import Context, Device, FloatTensor, Shape, get_ctx

# names the C driver takes (rn_model_create): the bottleneck networks, and the basic-block
# ResNet-18/34 (NativeModel / ShardedModel only: the reference-shaped graph below is bottleneck-only,
# like the reference)
ARCH_ID = {"resnet18": 18, "resnet34": 34, "resnet50": 50, "resnet101": 101, "resnet152": 152}


# ---------------------------------------------------------------------------
# reference-shaped graph (main.cu)
# ---------------------------------------------------------------------------
class Downsample:  # main.cu:7-16
    def __init__(self, conv: nn.Conv2d, bn: nn.BatchNorm2d):
        self.conv, self.bn = conv, bn
        self.act = FloatTensor(Device.GPU)


class ResnetBlock:  # main.cu:18-46
    def __init__(self, conv1, bn1, conv2, bn2, conv3, bn3, downsample: Optional[Downsample],
                 in_channels, inter_channels, out_channels, stride):
        self.conv1, self.bn1 = conv1, bn1
        self.conv2, self.bn2 = conv2, bn2
        self.conv3, self.bn3 = conv3, bn3
        self.downsample = downsample
        self.in_channels, self.inter_channels = in_channels, inter_channels
        self.out_channels, self.stride = out_channels, stride
        self.act1_out = FloatTensor(Device.GPU)
        self.act2_out = FloatTensor(Device.GPU)
        self.act3_out = FloatTensor(Device.GPU)


class Layer:  # main.cu:48-51
    def __init__(self, blocks: List[ResnetBlock]):
        self.blocks = blocks


class _Loader:
    """Where layer weights come from: a weights_bin/ directory (the reference's only
    source, nn.cuh:18-25) or an in-memory state dict."""

    def __init__(self, state: Optional[Dict[str, np.ndarray]] = None):
        self.state = state

    def tensor(self, key: str, shape) -> FloatTensor:
        if self.state is None:
            return FloatTensor.loadToCuda(nn.WEIGHTS_DIR + key).view(Shape(shape))
        return FloatTensor.from_numpy(self.state[key], Device.GPU).view(Shape(shape))

    def conv(self, name, cin, cout, k, stride=1, padding=0) -> nn.Conv2d:
        return nn.Conv2d(self.tensor(name + ".weight", (cout, cin, k, k)), cin, cout, k, stride,
                         padding)

    def bn(self, name, c) -> nn.BatchNorm2d:
        return nn.BatchNorm2d(*(self.tensor(f"{name}.{f}", (c,)) for f in weights.BN_FIELDS), c)

    def linear(self, name, fin, fout) -> nn.Linear:
        return nn.Linear(self.tensor(name + ".weight", (fout, fin)),
                         self.tensor(name + ".bias", (fout,)), fin, fout)


def createLayer(ld: _Loader, layer_id: int, in_channels: int, inter_channels: int,
                out_channels: int, n_blocks: int, stride: int = 1) -> Layer:
    """main.cu:53-89."""

    def load_block(block_id, cin, mid, cout, s) -> ResnetBlock:
        pre = f"layer{layer_id}.{block_id}."
        ds = None
        if block_id == 0 and (s != 1 or cin != cout):  # main.cu:71
            ds = Downsample(ld.conv(pre + "downsample.0", cin, cout, 1, s),
                            ld.bn(pre + "downsample.1", cout))
        return ResnetBlock(ld.conv(pre + "conv1", cin, mid, 1), ld.bn(pre + "bn1", mid),
                           ld.conv(pre + "conv2", mid, mid, 3, s, 1), ld.bn(pre + "bn2", mid),
                           ld.conv(pre + "conv3", mid, cout, 1), ld.bn(pre + "bn3", cout),
                           ds, cin, mid, cout, s)

    blocks = [load_block(0, in_channels, inter_channels, out_channels, stride)]
    for i in range(1, n_blocks):
        blocks.append(load_block(i, out_channels, inter_channels, out_channels, 1))
    return Layer(blocks)


class ResnetModel:  # main.cu:91-107
    def __init__(self, ld: _Loader, arch: str):
        d = weights.depths_of(arch)
        self.arch = arch
        self.conv1 = ld.conv("conv1", 3, 64, 7, 2, 3)
        self.bn1 = ld.bn("bn1", 64)
        self.act1_out = FloatTensor(Device.GPU)
        self.maxpool = nn.Pool2d(64, 3, 2, 1)
        self.maxpool_out = FloatTensor(Device.GPU)
        self.layer1 = createLayer(ld, 1, 64, 64, 256, d[0])
        self.layer2 = createLayer(ld, 2, 256, 128, 512, d[1], 2)
        self.layer3 = createLayer(ld, 3, 512, 256, 1024, d[2], 2)
        self.layer4 = createLayer(ld, 4, 1024, 512, 2048, d[3], 2)
        self.avgpool = nn.Pool2d(2048, 7)
        self.avgpool_out = FloatTensor(Device.GPU)
        self.fc = ld.linear("fc", 2048, 1000)
        self.fc_out = FloatTensor(Device.GPU)


def createResnet(arch: str = "resnet152", state: Optional[Dict[str, np.ndarray]] = None):
    """createResnet152 (main.cu:109-125) for any depth; weights from ``weights_bin/``
    (state=None, like the reference) or from a dict."""
    return ResnetModel(_Loader(state), arch)


def createResnet152(state=None) -> ResnetModel:
    return createResnet("resnet152", state)


def _ensure(holder, attr: str, shape: Shape) -> FloatTensor:
    """`if (!act) act = FloatTensor(shape, GPU)` (main.cu:141-143 and friends)."""
    t = getattr(holder, attr)
    if not t or t.shape() != shape:
        t = FloatTensor(shape, Device.GPU)
        setattr(holder, attr, t)
    return t


def layerForward(layer: Layer, x: FloatTensor) -> FloatTensor:
    """main.cu:127-166."""
    y = x
    for block in layer.blocks:
        if block.downsample:
            ds = block.downsample
            _ensure(ds, "act", ds.conv.getOutShape(y.shape()))
            ds.conv.forward(y, ds.act)
            ds.bn.forward(ds.act, ds.act)
        _ensure(block, "act1_out", block.conv1.getOutShape(y.shape()))
        block.conv1.forward(y, block.act1_out)
        block.bn1.forward(block.act1_out, block.act1_out)
        nn.reluForward(block.act1_out, block.act1_out)

        _ensure(block, "act2_out", block.conv2.getOutShape(block.act1_out.shape()))
        block.conv2.forward(block.act1_out, block.act2_out)
        block.bn2.forward(block.act2_out, block.act2_out)
        nn.reluForward(block.act2_out, block.act2_out)

        _ensure(block, "act3_out", block.conv3.getOutShape(block.act2_out.shape()))
        block.conv3.forward(block.act2_out, block.act3_out)
        block.bn3.forward(block.act3_out, block.act3_out)
        nn.addForward(block.act3_out, block.downsample.act if block.downsample else y,
                      block.act3_out)
        nn.reluForward(block.act3_out, block.act3_out)
        y = block.act3_out
    return y


def resnetForward(model: ResnetModel, x: FloatTensor) -> FloatTensor:
    """resnet152Forward (main.cu:168-226) without the progress prints and without the
    unused D2H copy of the layer4 activation (main.cu:207).  Returns model.fc_out."""
    assert x.device == Device.GPU
    x.shape().as_tuple(4)
    conv1_out_shape = model.conv1.getOutShape(x.shape())
    _ensure(model, "act1_out", conv1_out_shape)
    model.conv1.forward(x, model.act1_out)
    model.bn1.forward(model.act1_out, model.act1_out)
    nn.reluForward(model.act1_out, model.act1_out)
    _ensure(model, "maxpool_out", model.maxpool.getOutShape(conv1_out_shape))
    model.maxpool.maxforward(model.act1_out, model.maxpool_out)
    y = layerForward(model.layer1, model.maxpool_out)
    y = layerForward(model.layer2, y)
    y = layerForward(model.layer3, y)
    y = layerForward(model.layer4, y)
    _ensure(model, "avgpool_out", model.avgpool.getOutShape(y.shape()))
    model.avgpool.avgforward(y, model.avgpool_out)
    s = model.avgpool_out.shape()
    flat = model.avgpool_out.view(Shape((s[0], s[1] * s[2] * s[3])))
    _ensure(model, "fc_out", Shape((flat.shape()[0], model.fc.out_features)))
    model.fc.forward(flat, model.fc_out)
    return model.fc_out


def argmax(logits: np.ndarray) -> np.ndarray:
    """Host argmax of main.cu:243-251: strict '<', first maximum wins."""
    out = np.zeros(logits.shape[0], dtype=np.int64)
    for b in range(logits.shape[0]):
        mx = 0
        row = logits[b]
        for i in range(1, row.shape[0]):
            if row[mx] < row[i]:
                mx = i
        out[b] = mx
    return out


# ---------------------------------------------------------------------------
# the C driver
# ---------------------------------------------------------------------------
class NativeModel:
    def __init__(self, arch: str = "resnet50", state: Optional[Dict[str, np.ndarray]] = None,
                 weights_dir: Optional[str] = None, ctx: Optional[Context] = None,
                 dtype: str = "f32", classes: Optional[int] = None,
                 input_size: Optional[Tuple[int, int]] = None,
                 replace_stride_with_dilation: Optional[Tuple[bool, bool, bool]] = None):
        """classes: rows of the classifier; None = state["fc.weight"].shape[0] when a state is given,
        otherwise the library's 1000.  input_size: (H, W) of the images every forward reads, 32..2048 each;
        None = the library's 224 x 224 (set_input_size changes it later: the weights do not depend on it).
        replace_stride_with_dilation: torchvision's three flags (layer2, layer3, layer4), see set_dilation."""
        self.ctx = ctx or get_ctx()
        self.arch = arch
        lib = L.lib()
        h = ctypes.c_void_p()
        if arch in weights.FAMILY:  # ResNeXt / Wide ResNet: torchvision's (depth, groups, width_per_group)
            L.check(lib.rn_model_create_ex(self.ctx.handle, ctypes.byref(h), *weights.FAMILY[arch]),
                    "rn_model_create_ex", self.ctx.handle)
        else:
            L.check(lib.rn_model_create(self.ctx.handle, ctypes.byref(h), ARCH_ID[arch]),
                    "rn_model_create", self.ctx.handle)
        self.handle = h
        if (state is None) == (weights_dir is None):
            raise ValueError("give exactly one of state / weights_dir")
        if classes is None and state is not None:
            classes = int(np.shape(state["fc.weight"])[0])
        if classes is not None:  # before the first tensor: fc.* take their size from it
            L.check(lib.rn_model_set_classes(h, int(classes)), "rn_model_set_classes: 1..65536", self.ctx.handle)
        if weights_dir is not None:
            L.check(lib.rn_model_load_dir(h, weights_dir.encode()), "rn_model_load_dir",
                    self.ctx.handle)
        else:
            for key, numel in self.tensor_keys():
                arr = np.ascontiguousarray(state[key], dtype=np.float32)
                assert arr.size == numel, (key, arr.size, numel)
                L.check(lib.rn_model_set_tensor(h, key.encode(), arr.ctypes.data, numel),
                        f"rn_model_set_tensor({key})", self.ctx.handle)
        self.dtype = dtype
        L.check(lib.rn_model_set_dtype(h, {"f32": L.RN_DTYPE_F32, "bf16": L.RN_DTYPE_BF16}[dtype]),
                "rn_model_set_dtype", self.ctx.handle)
        L.check(lib.rn_model_finalize(h), "rn_model_finalize", self.ctx.handle)
        if input_size is not None:
            self.set_input_size(*input_size)
        if replace_stride_with_dilation is not None:
            self.set_dilation(*replace_stride_with_dilation)

    def set_dilation(self, layer2, layer3, layer4) -> None:
        """torchvision's replace_stride_with_dilation from the next forward on (rn_model_set_dilation): a
        flagged stage keeps its resolution and dilates its 3x3 convolutions.  Bottleneck networks only
        (RnError with RN_ERR_UNSUPPORTED on resnet18/34); refused, nothing changed, while a Graph or a Pipeline
        of this model lives.  Frees the activation arenas and drops the tuned tiles."""
        L.check(L.lib().rn_model_set_dilation(self.handle, int(bool(layer2)), int(bool(layer3)), int(bool(layer4))),
                "rn_model_set_dilation: bottleneck networks, no live Graph or Pipeline", self.ctx.handle)

    @property
    def dilation(self) -> Tuple[bool, bool, bool]:
        """The three flags (layer2, layer3, layer4): (False, False, False) unless set otherwise."""
        out = (ctypes.c_int * 3)()
        L.check(L.lib().rn_model_dilation(self.handle, out), "rn_model_dilation")
        return tuple(bool(v) for v in out)

    @property
    def output_stride(self) -> int:
        """Input pixels per pixel of the final map: 32, or 16 / 8 / 4 with dilated stages."""
        return int(L.lib().rn_model_output_stride(self.handle))

    def set_input_size(self, H: int, W: int) -> None:
        """Images of H x W from the next forward on (rn_model_set_input_size): 32..2048 each.  Refused
        (RnError, nothing changed) out of range and while a Graph or a Pipeline of this model lives.  Frees
        the activation arenas and drops the tuned tiles."""
        L.check(L.lib().rn_model_set_input_size(self.handle, int(H), int(W)),
                "rn_model_set_input_size: sides 32..2048, no live Graph or Pipeline", self.ctx.handle)

    @property
    def input_size(self) -> Tuple[int, int]:
        """(H, W) of the images the forwards read: (224, 224) unless set otherwise."""
        h, w = ctypes.c_uint64(), ctypes.c_uint64()
        L.check(L.lib().rn_model_input_size(self.handle, ctypes.byref(h), ctypes.byref(w)), "rn_model_input_size")
        return int(h.value), int(w.value)

    def max_sub_batch(self) -> int:
        """Images per launch batch at the model's input size (rn_model_max_sub_batch): 512 at 224 x 224, a
        smaller power of two for larger images; a larger batch runs as sub-batches, same bits."""
        return int(L.lib().rn_model_max_sub_batch(self.handle))

    def _check_input(self, x: np.ndarray, u8: bool = False) -> None:
        H, W = self.input_size
        want = (H, W, 3) if u8 else (3, H, W)
        assert x.ndim == 4 and tuple(x.shape[1:]) == want, (x.shape, "the model's input_size is", (H, W))

    @property
    def classes(self) -> int:
        return int(L.lib().rn_model_classes(self.handle))

    @property
    def features(self) -> int:
        """Width of the pooled feature vector: 512 (ResNet-18/34) or 2048."""
        return int(L.lib().rn_model_features(self.handle))

    def forward_outputs(self, x: np.ndarray, *, logits: bool = True, features: bool = False, probs: bool = False,
                        topk: int = 0, fused: bool = True) -> dict:
        """One forward, several outputs (rn_model_forward_outputs): a dict with the requested of
        "logits" [B,classes], "features" [B,features], "probs" [B,classes], "topk_prob" / "topk_idx" [B,topk].
        x: fp32 NCHW [B,3,H,W], or uint8 NHWC [B,H,W,3] (normalised on the device), H x W = input_size."""
        from .ops import _down_raw, _up_raw
        from .tensor import _DeviceBuffer
        x = np.asarray(x)
        u8 = x.dtype == np.uint8
        x = np.ascontiguousarray(x, dtype=np.uint8 if u8 else np.float32)
        self._check_input(x, u8)
        B, C, F, k = x.shape[0], self.classes, self.features, int(topk)
        xin = _up_raw(x)
        bufs = {}

        def buf(name, want, nbytes):
            if want:
                bufs[name] = _DeviceBuffer(self.ctx, max(nbytes, 16))
            return bufs[name].ptr if want else None

        o = L.ModelOutputs(buf("logits", logits, B * C * 4), buf("features", features, B * F * 4),
                           buf("probs", probs, B * C * 4), buf("topk_prob", k > 0, B * k * 4),
                           buf("topk_idx", k > 0, B * k * 8), k)
        fn = L.lib().rn_model_forward_outputs_u8 if u8 else L.lib().rn_model_forward_outputs
        L.check(fn(self.handle, xin.ptr, B, ctypes.byref(o), L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS),
                "rn_model_forward_outputs", self.ctx.handle)
        self.ctx.sync()
        shapes = {"logits": (B, C), "features": (B, F), "probs": (B, C), "topk_prob": (B, k), "topk_idx": (B, k)}
        out = {}
        for name, b in bufs.items():
            if name == "topk_idx":
                out[name] = _down_raw(b, np.uint64, B * k).astype(np.int64).reshape(B, k)
            else:
                out[name] = _down_raw(b, np.float32, int(np.prod(shapes[name]))).reshape(shapes[name])
        return out

    STAGES = ("layer1", "layer2", "layer3", "layer4")

    @property
    def stage_shapes(self) -> Dict[str, Tuple[int, int, int]]:
        """"layerN" -> (C, H, W) of the map behind that stage (rn_model_stage_shape): follows the architecture,
        input_size and dilation.  ResNet-50 at 224 x 224: (256, 56, 56) .. (2048, 7, 7)."""
        out = {}
        for i, name in enumerate(self.STAGES):
            c, h, w = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            L.check(L.lib().rn_model_stage_shape(self.handle, i + 1, ctypes.byref(c), ctypes.byref(h), ctypes.byref(w)),
                    "rn_model_stage_shape")
            out[name] = (int(c.value), int(h.value), int(w.value))
        return out

    def forward_maps(self, x: np.ndarray, stages=STAGES, *, logits: bool = False, features: bool = False,
                     probs: bool = False, topk: int = 0, fused: bool = True) -> dict:
        """One forward, the feature maps behind the named stages (rn_model_forward_maps; torchvision's
        IntermediateLayerGetter): a dict "layerN" -> [B,C,H,W] fp32 (stage_shapes) in the order of `stages`, then
        the head outputs asked for, as forward_outputs returns them.  bf16 models: the stored values, widened
        exactly.  x: fp32 NCHW [B,3,H,W], or uint8 NHWC [B,H,W,3] (normalised on the device).  An unknown or
        repeated stage name raises ValueError."""
        from .ops import _down_raw, _up_raw
        from .tensor import _DeviceBuffer
        stages = tuple(stages)
        for s in stages:
            if s not in self.STAGES:
                raise ValueError(f"unknown stage {s!r}: one of {self.STAGES}")
        if len(set(stages)) != len(stages):
            raise ValueError(f"repeated stage in {stages}")
        x = np.asarray(x)
        u8 = x.dtype == np.uint8
        x = np.ascontiguousarray(x, dtype=np.uint8 if u8 else np.float32)
        self._check_input(x, u8)
        B, C, F, k = x.shape[0], self.classes, self.features, int(topk)
        xin = _up_raw(x)
        shapes = {name: (B,) + chw for name, chw in self.stage_shapes.items()}
        mbufs = {s: _DeviceBuffer(self.ctx, max(int(np.prod(shapes[s])) * 4, 16)) for s in stages}
        maps = L.ModelMaps()
        for s in stages:
            maps.layer[self.STAGES.index(s)] = mbufs[s].ptr
        bufs = {}

        def buf(name, want, nbytes):
            if want:
                bufs[name] = _DeviceBuffer(self.ctx, max(nbytes, 16))
            return bufs[name].ptr if want else None

        o = L.ModelOutputs(buf("logits", logits, B * C * 4), buf("features", features, B * F * 4),
                           buf("probs", probs, B * C * 4), buf("topk_prob", k > 0, B * k * 4),
                           buf("topk_idx", k > 0, B * k * 8), k)
        fn = L.lib().rn_model_forward_maps_u8 if u8 else L.lib().rn_model_forward_maps
        L.check(fn(self.handle, xin.ptr, B, ctypes.byref(o), ctypes.byref(maps),
                   L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS), "rn_model_forward_maps", self.ctx.handle)
        self.ctx.sync()
        shapes.update({"logits": (B, C), "features": (B, F), "probs": (B, C), "topk_prob": (B, k), "topk_idx": (B, k)})
        out = {s: _down_raw(mbufs[s], np.float32, int(np.prod(shapes[s]))).reshape(shapes[s]) for s in stages}
        for name, b in bufs.items():
            if name == "topk_idx":
                out[name] = _down_raw(b, np.uint64, B * k).astype(np.int64).reshape(B, k)
            else:
                out[name] = _down_raw(b, np.float32, int(np.prod(shapes[name]))).reshape(shapes[name])
        return out

    def forward_maps_u8(self, px: np.ndarray, stages=STAGES, **kw) -> dict:
        """forward_maps from 8-bit RGB [B,H,W,3] (rn_model_forward_maps_u8): the same maps as forward_maps on
        preprocess.normalize_u8 of the bytes, bit for bit."""
        return self.forward_maps(np.ascontiguousarray(px, dtype=np.uint8), stages, **kw)

    def forward_segment(self, x: np.ndarray, head, labels: bool = True, scores: bool = False, *, logits: bool = False,
                        features: bool = False, probs: bool = False, topk: int = 0, fused: bool = True) -> dict:
        """One forward with a segmentation head behind layer4 (rn_model_forward_segment): a dict with "labels"
        [B,H,W] uint8 and / or "scores" [B,classes,H,W] fp32 at the model's input_size, then the head outputs
        asked for, as forward_outputs returns them.  head: a segmentation.FCNHead or segmentation.DeepLabHead of this
        model's feature width and dtype, on this model's context.  x: fp32 NCHW [B,3,H,W], or uint8 NHWC [B,H,W,3]."""
        from .ops import _down_raw, _up_raw
        from .tensor import _DeviceBuffer
        x = np.asarray(x)
        u8 = x.dtype == np.uint8
        x = np.ascontiguousarray(x, dtype=np.uint8 if u8 else np.float32)
        self._check_input(x, u8)
        (H, W), K = self.input_size, head.classes
        B, C, F, k = x.shape[0], self.classes, self.features, int(topk)
        xin = _up_raw(x)
        bufs = {}

        def buf(name, want, nbytes):
            if want:
                bufs[name] = _DeviceBuffer(self.ctx, max(nbytes, 16))
            return bufs[name].ptr if want else None

        seg = L.SegOutputs(buf("labels", labels, B * H * W), buf("scores", scores, B * K * H * W * 4))
        o = L.ModelOutputs(buf("logits", logits, B * C * 4), buf("features", features, B * F * 4),
                           buf("probs", probs, B * C * 4), buf("topk_prob", k > 0, B * k * 4),
                           buf("topk_idx", k > 0, B * k * 8), k)
        fn = L.lib().rn_model_forward_segment_u8 if u8 else L.lib().rn_model_forward_segment
        L.check(fn(self.handle, head.handle, xin.ptr, B, ctypes.byref(o), ctypes.byref(seg),
                   L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS), "rn_model_forward_segment", self.ctx.handle)
        self.ctx.sync()
        shapes = {"scores": (B, K, H, W), "logits": (B, C), "features": (B, F), "probs": (B, C), "topk_prob": (B, k),
                  "topk_idx": (B, k)}
        out = {}
        for name, b in bufs.items():
            if name == "labels":
                out[name] = _down_raw(b, np.uint8, B * H * W).reshape(B, H, W)
            elif name == "topk_idx":
                out[name] = _down_raw(b, np.uint64, B * k).astype(np.int64).reshape(B, k)
            else:
                out[name] = _down_raw(b, np.float32, int(np.prod(shapes[name]))).reshape(shapes[name])
        return out

    def forward_segment_u8(self, px: np.ndarray, head, **kw) -> dict:
        """forward_segment from 8-bit RGB [B,H,W,3] (rn_model_forward_segment_u8): the same scores and labels as
        forward_segment on preprocess.normalize_u8 of the bytes, bit for bit."""
        return self.forward_segment(np.ascontiguousarray(px, dtype=np.uint8), head, **kw)

    def forward_fpn(self, x: np.ndarray, neck, stages=STAGES, levels=None, *, logits: bool = False,
                    features: bool = False, probs: bool = False, topk: int = 0, fused: bool = True, rois=None,
                    pooler=None, roi_levels: bool = False, validate: bool = True, rpn=None, candidates: bool = False,
                    box_head=None, detect_intermediates: bool = False, mask_head=None, masks=("probs",),
                    mask_pooled: bool = False, keypoint_head=None, keypoints=("keypoints",)) -> dict:
        """One forward with a feature pyramid neck (rn_model_forward_fpn; torchvision's resnet_fpn_backbone): an
        ordered dict "0", "1", .. (one per stage in `stages`, finest first), then "pool" when the neck has the extra
        block -> [B,a,H,W] fp32; then the head outputs asked for, as forward_outputs returns them.  neck: an
        fpn.FeaturePyramidNetwork of this model's dtype on this model's context whose in_channels_list is the
        channels of `stages`.  levels: the names wanted (default: all).  x: fp32 NCHW [B,3,H,W], or uint8 NHWC
        [B,H,W,3].  An unknown, repeated or descending stage, a stage count that is not the neck's, or an unknown
        level raises ValueError.
        With rois ([K,5] fp32: image index, x1, y1, x2, y2 in pixels of the model's input) and a pooler
        (roi.MultiScaleRoIAlign): rn_model_forward_rois, the same launches plus the pooler's behind the neck, which
        adds "pooled" [K,a,PH,PW] fp32 and, with roi_levels, "roi_levels" int32 [K]; levels may then be empty.  A RoI
        whose image index is no integer in [0, B) raises ValueError (validate=False hands it to the device: zeros
        and level -1).
        With rpn (rpn.RegionProposalNetwork over all of the neck's outputs): rn_model_forward_proposals, which adds per
        image "proposals" ([count_i, 4]), "scores" and "proposal_levels" (and "cand" with candidates=True); with a
        pooler and no rois the pooler takes the proposals of the same forward on the device: "pooled" is
        [B*post,a,PH,PW] and "rois" [B*post,5] is returned with it.
        With box_head (detection.BoxHead) behind that rpn and pooler (no rois): rn_model_forward_detections, which adds
        "boxes" [B,D,4], "scores" [B,D] (in place of the proposals' scores, which stay under "proposal_scores"), "labels",
        "detections" (the counts [B]) and "detection_rois" (the proposal row of every detection), padded as the device
        wrote them; with detect_intermediates also "probs", "class_boxes", "valid" and "keep".
        With mask_head (mask.MaskHead) behind that box head: rn_model_forward_masks, which adds "mask_rois" [B*D,5] and,
        as `masks` names them ("probs", "image", "bits"), "mask_probs" [B,D,2M,2M], "masks" [B,D,H,W] fp32 and
        "mask_bits" [B,D,H,W] uint8 at the model's input size (and "mask_pooled" [B*D,M,M,a] with mask_pooled).
        With keypoint_head (keypoint.KeypointHead) behind that box head, with or without a mask head:
        rn_model_forward_keypoints, which adds, as `keypoints` names them ("keypoints", "heatmaps", "rois", "pooled"),
        "keypoints" [B,D,Kp,3] with "keypoints_scores" [B,D,Kp], "keypoint_heatmaps" [B,D,Kp,4M,4M], "keypoint_rois"
        [B*D,5] and "keypoint_pooled" [B*D,M,M,a]."""
        from .fpn import NeckTail
        from .ops import _down_raw, _up_raw
        from .tensor import _DeviceBuffer
        stages = tuple(stages)
        for s in stages:
            if s not in self.STAGES:
                raise ValueError(f"unknown stage {s!r}: one of {self.STAGES}")
        idx = [self.STAGES.index(s) + 1 for s in stages]
        if any(b <= a for a, b in zip(idx, idx[1:])):
            raise ValueError(f"stages must ascend without repeats: {stages}")
        if len(stages) != len(neck.in_channels_list):
            raise ValueError(f"{len(stages)} stages for a neck of {len(neck.in_channels_list)} levels")
        names = neck.names
        levels = names if levels is None else tuple(levels)
        for name in levels:
            if name not in names:
                raise ValueError(f"unknown level {name!r}: one of {names}")
        x = np.asarray(x)
        tail = NeckTail(self.ctx, names, neck.out_channels, x.shape[0], self.input_size, rois, pooler, roi_levels, validate,
                        rpn, candidates, box_head, detect_intermediates, mask_head, masks, mask_pooled, keypoint_head, keypoints)
        u8 = x.dtype == np.uint8
        x = np.ascontiguousarray(x, dtype=np.uint8 if u8 else np.float32)
        self._check_input(x, u8)
        B, C, F, k = x.shape[0], self.classes, self.features, int(topk)
        xin = _up_raw(x)
        stage_shapes = self.stage_shapes
        shapes, lbufs = {}, {}
        fo = L.FpnOutputs()
        for i, name in enumerate(names):
            _, h, w = stage_shapes[stages[min(i, len(stages) - 1)]]
            shapes[name] = (B,) + neck.level_shape(name, h, w)
            if name in levels:
                lbufs[name] = _DeviceBuffer(self.ctx, max(int(np.prod(shapes[name])) * 4, 16))
                fo.level[i] = lbufs[name].ptr
        bufs = {}

        def buf(name, want, nbytes):
            if want:
                bufs[name] = _DeviceBuffer(self.ctx, max(nbytes, 16))
            return bufs[name].ptr if want else None

        o = L.ModelOutputs(buf("logits", logits, B * C * 4), buf("features", features, B * F * 4),
                           buf("probs", probs, B * C * 4), buf("topk_prob", k > 0, B * k * 4),
                           buf("topk_idx", k > 0, B * k * 8), k)
        tail.build()
        mode = L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS
        stage_arr = (ctypes.c_int * len(idx))(*idx)
        objs = {"fpn": (), "rois": (), "proposals": (rpn,), "detections": (rpn, box_head),
                "masks": (rpn, box_head, mask_head), "keypoints": (rpn, box_head, mask_head, keypoint_head)}[tail.entry]
        name = "rn_model_forward_" + tail.entry
        fn = getattr(L.lib(), name + ("_u8" if u8 else ""))
        L.check(fn(self.handle, neck.handle, *[obj.handle if obj is not None else None for obj in objs], xin.ptr, B, ctypes.byref(o), stage_arr,
                   ctypes.byref(fo), *tail.requests, mode), name, self.ctx.handle)
        self.ctx.sync()
        shapes.update({"logits": (B, C), "features": (B, F), "probs": (B, C), "topk_prob": (B, k), "topk_idx": (B, k)})
        out = {name: _down_raw(lbufs[name], np.float32, int(np.prod(shapes[name]))).reshape(shapes[name])
               for name in names if name in lbufs}
        for name, b in bufs.items():
            if name == "topk_idx":
                out[name] = _down_raw(b, np.uint64, B * k).astype(np.int64).reshape(B, k)
            else:
                out[name] = _down_raw(b, np.float32, int(np.prod(shapes[name]))).reshape(shapes[name])
        return tail.collect(out)

    def forward_fpn_u8(self, px: np.ndarray, neck, stages=STAGES, levels=None, **kw) -> dict:
        """forward_fpn from 8-bit RGB [B,H,W,3] (rn_model_forward_fpn_u8): the same pyramid as forward_fpn on
        preprocess.normalize_u8 of the bytes, bit for bit."""
        return self.forward_fpn(np.ascontiguousarray(px, dtype=np.uint8), neck, stages, levels, **kw)

    def tensor_keys(self) -> List[Tuple[str, int]]:
        out, i, n = [], 0, ctypes.c_uint64()
        while True:
            k = L.lib().rn_model_tensor_key(self.handle, i, ctypes.byref(n))
            if k is None:
                return out
            out.append((k.decode(), n.value))
            i += 1

    def forward_ptr(self, input_ptr: int, B: int, logits_ptr: int, fused: bool = True) -> None:
        """Queue one forward on the context's stream (asynchronous)."""
        L.check(L.lib().rn_model_forward(self.handle, input_ptr, B, logits_ptr,
                                         L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS),
                "rn_model_forward", self.ctx.handle)

    def forward(self, x: np.ndarray, fused: bool = True) -> np.ndarray:
        """NCHW host array [B,3,H,W] of the model's input_size -> logits host array (synchronous convenience)."""
        self._check_input(np.asarray(x))
        xin = FloatTensor.from_numpy(x, Device.GPU)
        B = x.shape[0]
        out = FloatTensor((B, self.classes), Device.GPU)
        self.forward_ptr(xin.data(), B, out.data(), fused)
        self.ctx.sync()
        return out.numpy()

    def forward_u8_ptr(self, input_ptr: int, B: int, logits_ptr: int, fused: bool = True) -> None:
        """Queue one forward from 8-bit RGB [B,H,W,3] (input_size) on the device (asynchronous): the first
        launch normalises the bytes (rn_model_forward_u8); same logits as forward_ptr on
        preprocess.normalize_u8 of them, bit for bit."""
        L.check(L.lib().rn_model_forward_u8(self.handle, input_ptr, B, logits_ptr,
                                            L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS),
                "rn_model_forward_u8", self.ctx.handle)

    def forward_u8(self, px: np.ndarray, fused: bool = True) -> np.ndarray:
        """uint8 RGB host array [B,H,W,3] of the model's input_size -> logits host array (synchronous
        convenience)."""
        from .ops import _up_raw
        px = np.ascontiguousarray(px, dtype=np.uint8)
        self._check_input(px, True)
        B = px.shape[0]
        xin = _up_raw(px)
        out = FloatTensor((B, self.classes), Device.GPU)
        self.forward_u8_ptr(xin.ptr, B, out.data(), fused)
        self.ctx.sync()
        return out.numpy()

    def forward_images(self, images, fused: bool = True) -> np.ndarray:
        """A list of decoded [H,W,3] uint8 RGB arrays of any sizes -> logits host array: the device
        resizes (short side 256) and centre-crops (224) them to PIL's bytes, then runs forward_u8's
        launches (rn_model_forward_images_u8).  Synchronous convenience.  Only at input_size (224, 224):
        RnError (RN_ERR_UNSUPPORTED) otherwise."""
        from .ops import _u64p, _up_raw, pack_images
        packed, offsets, heights, widths = pack_images(images)
        B = len(heights)
        xin = _up_raw(packed)
        out = FloatTensor((B, self.classes), Device.GPU)
        L.check(L.lib().rn_model_forward_images_u8(self.handle, xin.ptr, _u64p(offsets), _u64p(heights), _u64p(widths),
                                                   B, out.data(), L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS),
                "rn_model_forward_images_u8", self.ctx.handle)
        self.ctx.sync()
        return out.numpy()

    def tune(self, input_ptr: int, B: int, logits_ptr: int, fused: bool = True) -> None:
        """Pick the fastest contraction tile per layer for batch B (results unchanged)."""
        L.check(L.lib().rn_model_tune(self.handle, input_ptr, B, logits_ptr,
                                      L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS),
                "rn_model_tune", self.ctx.handle)

    def export_tuning(self) -> np.ndarray:
        """The tile table of the last tune() as uint64 words (rn_model_export_tuning): for a model of the
        same architecture, element type and settings on an identical device, or a later process."""
        n = ctypes.c_uint64()
        L.check(L.lib().rn_model_export_tuning(self.handle, None, 0, ctypes.byref(n)), "rn_model_export_tuning")
        words = np.zeros(n.value, dtype=np.uint64)
        L.check(L.lib().rn_model_export_tuning(self.handle, words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                               n.value, ctypes.byref(n)), "rn_model_export_tuning: not tuned")
        return words

    def import_tuning(self, words: np.ndarray) -> None:
        """Take over another model's tile table; refused (RnError) when it was measured for another
        architecture, element type, fusion setting or build.  Tiles change speed only."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        L.check(L.lib().rn_model_import_tuning(self.handle, words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                               words.size), "rn_model_import_tuning: table of another model or build")

    def set_pair_fusion(self, on: bool) -> None:
        """Fused mode: conv3 + downsample of a stage's first block as one contraction (default
        on) or as two launches with the downsample tensor as the residual."""
        L.check(L.lib().rn_model_set_pair_fusion(self.handle, int(on)), "rn_model_set_pair_fusion")

    def set_streams(self, streams: int) -> None:
        """2 (default): batches of >= 128 images (fp32 at the default: >= 256) run as two halves on two
        streams; 1: one stream."""
        L.check(L.lib().rn_model_set_streams(self.handle, int(streams)), "rn_model_set_streams")

    def streams(self) -> int:
        return int(L.lib().rn_model_get_streams(self.handle))

    def parts(self, B: int) -> int:
        """Streams a forward of B images actually runs on: the configured count, halved while a part
        would be smaller than 64 images (128 for an fp32 model left at the library default)."""
        return int(L.lib().rn_model_parts(self.handle, int(B)))

    def set_chain(self, on: bool) -> None:
        """Fused mode: conv3 of a bottleneck block + conv1 of the next block as one launch wherever
        a chain kernel exists (fp32: the 64-channel blocks of stage 1; bf16: those and the
        128-channel blocks of stage 2; rn_model.c chain_applies).  Default on.  The same bits
        whatever the setting."""
        L.check(L.lib().rn_model_set_chain(self.handle, int(on)), "rn_model_set_chain")

    def set_stem_pool_fusion(self, on) -> None:
        """Fused mode: conv1 + bn1 + relu + maxpool as one launch (default on); 2 = that launch
        reads the NCHW input itself, no layout launch in front of it."""
        L.check(L.lib().rn_model_set_stem_pool_fusion(self.handle, int(on)), "rn_model_set_stem_pool_fusion")

    def set_front_parts(self, parts: int) -> None:
        """Stem, max-pool and first stage in `parts` slices of the batch (Infinity-Cache reuse)."""
        L.check(L.lib().rn_model_set_front_parts(self.handle, int(parts)), "rn_model_set_front_parts")

    def set_stem_exact(self, on: bool) -> None:
        """fp32: stem in the exact-K form (K = 160, default) or the 4-channel slot form (224)."""
        L.check(L.lib().rn_model_set_stem_exact(self.handle, int(on)), "rn_model_set_stem_exact")

    def set_profiling(self, on: bool) -> None:
        L.check(L.lib().rn_model_set_profiling(self.handle, int(on)), "rn_model_set_profiling")

    def profile(self) -> List[dict]:
        """Per-op records of the last profiled forward (after a sync)."""
        lib = L.lib()
        self.ctx.sync()
        recs = []
        op, layer = ctypes.c_char_p(), ctypes.c_char_p()
        ms, fl, by = ctypes.c_float(), ctypes.c_double(), ctypes.c_double()
        for i in range(lib.rn_model_profile_count(self.handle)):
            L.check(lib.rn_model_profile_get(self.handle, i, ctypes.byref(op), ctypes.byref(layer),
                                             ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)),
                    "rn_model_profile_get")
            recs.append({"op": op.value.decode(), "layer": layer.value.decode(), "ms": ms.value,
                         "flops": fl.value, "bytes": by.value})
        return recs

    def activation_bytes(self) -> int:
        return int(L.lib().rn_model_activation_bytes(self.handle))

    def close(self) -> None:
        if self.handle:
            # refused (nothing freed) while a graph captured from this model lives: close those first
            L.check(L.lib().rn_model_destroy(self.handle), "rn_model_destroy: graphs captured from the model "
                    "are still alive")
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardedModel:
    """One batch over several devices of a node (rn_shard_*): the multi-device form of the
    reference's main() (main.cu:228-254).  Contiguous batch split, weights replicated, no data
    moves between devices; one host thread + context + model per listed device inside the
    library.  A device may be listed twice (how a one-GPU box exercises the sharding)."""

    def __init__(self, devices, arch: str = "resnet50", state: Optional[Dict[str, np.ndarray]] = None,
                 weights_dir: Optional[str] = None, dtype: str = "f32"):
        lib = L.lib()
        if (state is None) == (weights_dir is None):
            raise ValueError("give exactly one of state / weights_dir")
        dev = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        if arch in weights.FAMILY:
            L.check(lib.rn_shard_create_ex(ctypes.byref(h), dev, len(devices), *weights.FAMILY[arch]),
                    "rn_shard_create_ex")
        else:
            L.check(lib.rn_shard_create(ctypes.byref(h), dev, len(devices), ARCH_ID[arch]), "rn_shard_create")
        self.handle, self.n = h, len(devices)
        self._stream_B = 0
        self._stream_input = "f32"
        if weights_dir is not None:
            self._check(lib.rn_shard_load_dir(h, weights_dir.encode()), "rn_shard_load_dir")
        else:
            for key, arr in state.items():
                if key.endswith("num_batches_tracked"):
                    continue
                a = np.ascontiguousarray(arr, dtype=np.float32)
                self._check(lib.rn_shard_set_tensor(h, key.encode(), a.ctypes.data, a.size),
                            f"rn_shard_set_tensor({key})")
        self._check(lib.rn_shard_set_dtype(h, {"f32": L.RN_DTYPE_F32, "bf16": L.RN_DTYPE_BF16}[dtype]),
                    "rn_shard_set_dtype")
        self._check(lib.rn_shard_finalize(h), "rn_shard_finalize")

    def _check(self, status: int, where: str) -> None:
        if status != L.RN_OK:
            msg = L.lib().rn_shard_last_error(self.handle)
            raise L.RnError(status, where, msg.decode() if msg else "")

    @staticmethod
    def bounds(B: int, rank: int, world: int) -> Tuple[int, int]:
        lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
        L.lib().rn_shard_bounds(B, rank, world, ctypes.byref(lo), ctypes.byref(hi))
        return lo.value, hi.value

    def forward(self, x: np.ndarray, fused: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """NCHW host array -> (logits [B,1000], top-1 [B]) host arrays, image order."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        B = x.shape[0]
        logits = np.empty((B, 1000), dtype=np.float32)
        top1 = np.empty(B, dtype=np.uint64)
        self._check(L.lib().rn_shard_forward(self.handle, x.ctypes.data, B, logits.ctypes.data,
                                             top1.ctypes.data,
                                             L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS),
                    "rn_shard_forward")
        return logits, top1

    def forward_u8(self, px: np.ndarray, fused: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """uint8 RGB host array [B,224,224,3] -> (logits [B,1000], top-1 [B]), image order."""
        px = np.ascontiguousarray(px, dtype=np.uint8)
        assert px.ndim == 4 and px.shape[1:] == (224, 224, 3), px.shape
        B = px.shape[0]
        logits = np.empty((B, 1000), dtype=np.float32)
        top1 = np.empty(B, dtype=np.uint64)
        self._check(L.lib().rn_shard_forward_u8(self.handle, px.ctypes.data, B, logits.ctypes.data,
                                                top1.ctypes.data,
                                                L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS),
                    "rn_shard_forward_u8")
        return logits, top1

    def tune(self, x: np.ndarray, fused: bool = True) -> None:
        x = np.ascontiguousarray(x, dtype=np.float32)
        self._check(L.lib().rn_shard_tune(self.handle, x.ctypes.data, x.shape[0],
                                          L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS),
                    "rn_shard_tune")

    def tuning_of(self, rank: int) -> np.ndarray:
        """The tile table shard `rank` runs with (rn_shard_model + rn_model_export_tuning)."""
        lib = L.lib()
        mh = lib.rn_shard_model(self.handle, rank)
        n = ctypes.c_uint64()
        self._check(lib.rn_model_export_tuning(mh, None, 0, ctypes.byref(n)), "rn_model_export_tuning")
        words = np.zeros(n.value, dtype=np.uint64)
        self._check(lib.rn_model_export_tuning(mh, words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n.value,
                                               ctypes.byref(n)), "rn_model_export_tuning: shard not tuned")
        return words

    def placement(self, rank: int):
        """(device, NUMA node of the device's slot or -1, the CPUs shard `rank`'s host thread is bound to or '')."""
        dev, node, buf = ctypes.c_int(), ctypes.c_int(), ctypes.create_string_buffer(256)
        self._check(L.lib().rn_shard_placement(self.handle, rank, ctypes.byref(dev), ctypes.byref(node), buf, 256),
                    "rn_shard_placement")
        return dev.value, node.value, buf.value.decode()

    # streaming form: consecutive batches of B images, two in flight on every device
    def stream_open(self, B: int, fused: bool = True, input: str = "f32") -> None:
        """input: "f32" (NCHW floats: submit) or "u8" (RGB bytes [B,224,224,3]: submit_u8)."""
        if input not in ("f32", "u8"):
            raise ValueError(f"input must be 'f32' or 'u8', not {input!r}")
        lib = L.lib()
        opener = lib.rn_shard_stream_open_u8 if input == "u8" else lib.rn_shard_stream_open
        self._check(opener(self.handle, B, L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS),
                    "rn_shard_stream_open_u8" if input == "u8" else "rn_shard_stream_open")
        self._stream_B = B
        self._stream_input = input

    def stream_buffer(self, rank: int):
        """(pinned staging of shard `rank` for the next submit as [hi-lo,3,224,224] floats, or in a
        byte stream as [hi-lo,224,224,3] uint8, lo, hi)."""
        u8 = self._stream_input == "u8"
        ptr, lo, hi = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        fn = L.lib().rn_shard_stream_buffer_u8 if u8 else L.lib().rn_shard_stream_buffer
        self._check(fn(self.handle, rank, ctypes.byref(ptr), ctypes.byref(lo), ctypes.byref(hi)),
                    "rn_shard_stream_buffer_u8" if u8 else "rn_shard_stream_buffer")
        n = hi.value - lo.value
        if n == 0:
            return None, lo.value, hi.value
        if u8:
            buf = (ctypes.c_uint8 * (n * 224 * 224 * 3)).from_address(ptr.value)
            return np.frombuffer(buf, dtype=np.uint8).reshape(n, 224, 224, 3), lo.value, hi.value
        buf = (ctypes.c_float * (n * 3 * 224 * 224)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=np.float32).reshape(n, 3, 224, 224), lo.value, hi.value

    def submit(self, x: Optional[np.ndarray] = None) -> None:
        ptr = None
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.float32)
            assert self._stream_B == 0 or x.shape == (self._stream_B, 3, 224, 224)
            ptr = x.ctypes.data
        self._check(L.lib().rn_shard_submit(self.handle, ptr), "rn_shard_submit")

    def submit_u8(self, px: Optional[np.ndarray] = None) -> None:
        """px: [B,224,224,3] uint8, or None when the staging buffers were filled in place."""
        ptr = None
        if px is not None:
            px = np.ascontiguousarray(px, dtype=np.uint8)
            assert self._stream_B == 0 or px.shape == (self._stream_B, 224, 224, 3)
            ptr = px.ctypes.data
        self._check(L.lib().rn_shard_submit_u8(self.handle, ptr), "rn_shard_submit_u8")

    def collect(self) -> Tuple[np.ndarray, np.ndarray]:
        logits = np.empty((self._stream_B, 1000), dtype=np.float32)
        top1 = np.empty(self._stream_B, dtype=np.uint64)
        self._check(L.lib().rn_shard_collect(self.handle, logits.ctypes.data, top1.ctypes.data), "rn_shard_collect")
        return logits, top1

    def in_flight(self) -> int:
        return int(L.lib().rn_shard_in_flight(self.handle))

    def stream_close(self) -> None:
        self._check(L.lib().rn_shard_stream_close(self.handle), "rn_shard_stream_close")

    def close(self) -> None:
        if self.handle:
            L.lib().rn_shard_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Graph:
    """A captured forward (rn_model_capture) of `batch` images of the model's input_size: launch() replays it
    on the context's stream.  While it lives the model refuses set_input_size."""

    def __init__(self, model: NativeModel, input_ptr, batch: int, logits_ptr, fused: bool = True):
        self.model = model
        h = ctypes.c_void_p()
        L.check(L.lib().rn_model_capture(model.handle, input_ptr, batch, logits_ptr,
                                         L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS,
                                         ctypes.byref(h)), "rn_model_capture", model.ctx.handle)
        self.handle = h

    def launch(self) -> None:
        L.check(L.lib().rn_graph_launch(self.handle), "rn_graph_launch", self.model.ctx.handle)

    def node_count(self) -> int:
        return int(L.lib().rn_graph_node_count(self.handle))

    def close(self) -> None:
        if self.handle:
            L.lib().rn_graph_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipeline:
    """Stream of host batches through a NativeModel with the upload of the next batch
    overlapped with the forward of the current one (rn_pipeline_*, two slots)."""

    def __init__(self, model: NativeModel, batch: int, fused: bool = True, input: str = "f32",
                 max_batch_bytes: Optional[int] = None):
        """input: "f32" (NCHW floats, submit), "u8" (RGB bytes [n,H,W,3], submit_u8: a
        quarter of the upload, normalised on the device) or "images" (decoded RGB images of any
        size, submit_images: resized and cropped on the device, models of input_size (224, 224) only;
        ``max_batch_bytes`` is the room for one batch's pixels, default 1 MB per image).  The buffers
        are sized for the model's input_size at creation; while the pipeline lives the model refuses
        set_input_size."""
        if input not in ("f32", "u8", "images"):
            raise ValueError(f"input must be 'f32', 'u8' or 'images', not {input!r}")
        self.model, self.batch, self.input = model, batch, input
        self.classes = model.classes  # the row length of what collect() returns
        self.input_size = model.input_size  # (H, W) of the staging buffers
        h = ctypes.c_void_p()
        mode = L.RN_FWD_FUSED if fused else L.RN_FWD_REFERENCE_OPS
        if input == "images":
            self.max_batch_bytes = int(max_batch_bytes) if max_batch_bytes is not None else batch << 20
            L.check(L.lib().rn_pipeline_create_images_u8(model.handle, ctypes.byref(h), batch, mode, self.max_batch_bytes),
                    "rn_pipeline_create_images_u8", model.ctx.handle)
        else:
            create = L.lib().rn_pipeline_create_u8 if input == "u8" else L.lib().rn_pipeline_create
            L.check(create(model.handle, ctypes.byref(h), batch, mode),
                    "rn_pipeline_create_u8" if input == "u8" else "rn_pipeline_create", model.ctx.handle)
        self.handle = h

    def input_buffer(self) -> np.ndarray:
        """The pinned staging buffer of the next slot as a [B,3,H,W] float array (a byte
        pipeline: [B,H,W,3] uint8), H x W the model's input_size: fill it in place, then submit without
        an argument."""
        ptr = ctypes.c_void_p()
        H, W = self.input_size
        if self.input == "u8":
            L.check(L.lib().rn_pipeline_input_buffer_u8(self.handle, ctypes.byref(ptr)),
                    "rn_pipeline_input_buffer_u8", self.model.ctx.handle)
            buf = (ctypes.c_uint8 * (self.batch * H * W * 3)).from_address(ptr.value)
            return np.frombuffer(buf, dtype=np.uint8).reshape(self.batch, H, W, 3)
        L.check(L.lib().rn_pipeline_input_buffer(self.handle, ctypes.byref(ptr)),
                "rn_pipeline_input_buffer", self.model.ctx.handle)
        n = self.batch * 3 * H * W
        buf = (ctypes.c_float * n).from_address(ptr.value)
        return np.frombuffer(buf, dtype=np.float32).reshape(self.batch, 3, H, W)

    def submit(self, x: np.ndarray | None = None) -> None:
        """x: [n,3,H,W] (the model's input_size) with n <= batch (a ragged last batch), or None when the staging
        buffer was filled in place (a whole batch)."""
        ptr, n = None, self.batch
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.float32)
            assert x.shape[1:] == (3,) + self.input_size, (x.shape, self.input_size)
            ptr, n = x.ctypes.data, x.shape[0]
        L.check(L.lib().rn_pipeline_submit_n(self.handle, ptr, n), "rn_pipeline_submit_n",
                self.model.ctx.handle)

    def submit_u8(self, px: np.ndarray | None = None) -> None:
        """px: [n,H,W,3] uint8 (the model's input_size) with n <= batch, or None when the staging buffer was filled in
        place (a whole batch).  Only on a pipeline created with input="u8"."""
        ptr, n = None, self.batch
        if px is not None:
            px = np.ascontiguousarray(px, dtype=np.uint8)
            assert px.shape[1:] == self.input_size + (3,), (px.shape, self.input_size)
            ptr, n = px.ctypes.data, px.shape[0]
        L.check(L.lib().rn_pipeline_submit_u8_n(self.handle, ptr, n), "rn_pipeline_submit_u8_n",
                self.model.ctx.handle)

    def submit_images(self, images) -> None:
        """images: a list of n <= batch decoded [H,W,3] uint8 arrays of any sizes (pageable memory: the
        library packs them into its pinned staging).  Only on a pipeline created with input="images"."""
        imgs = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
        for a in imgs:
            assert a.ndim == 3 and a.shape[2] == 3, a.shape
        n = len(imgs)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in imgs])
        heights = np.array([a.shape[0] for a in imgs], dtype=np.uint64)
        widths = np.array([a.shape[1] for a in imgs], dtype=np.uint64)
        u64p = ctypes.POINTER(ctypes.c_uint64)
        L.check(L.lib().rn_pipeline_submit_images_u8_n(self.handle, ptrs, heights.ctypes.data_as(u64p),
                                                       widths.ctypes.data_as(u64p), n),
                "rn_pipeline_submit_images_u8_n", self.model.ctx.handle)

    def collect(self) -> np.ndarray:
        return self.collect_top1()[0]

    def collect_top1(self):
        """(logits [n,classes], class indices [n]) of the oldest batch in flight."""
        out = np.empty((self.batch, self.classes), dtype=np.float32)
        idx = np.empty(self.batch, dtype=np.uint64)
        n = ctypes.c_uint64()
        L.check(L.lib().rn_pipeline_collect_n(self.handle, out.ctypes.data, idx.ctypes.data, ctypes.byref(n)),
                "rn_pipeline_collect_n", self.model.ctx.handle)
        return out[:n.value], idx[:n.value]

    def in_flight(self) -> int:
        return int(L.lib().rn_pipeline_in_flight(self.handle))

    def run(self, batches):
        """Yield logits for an iterable of host batches, keeping two in flight."""
        for x in batches:
            if self.in_flight() == 2:
                yield self.collect()
            {"u8": self.submit_u8, "images": self.submit_images}.get(self.input, self.submit)(x)
        while self.in_flight():
            yield self.collect()

    def close(self) -> None:
        if self.handle:
            L.lib().rn_pipeline_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
