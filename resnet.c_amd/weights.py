"""Weight files either side of the forward path.

Two things live here:

* the on-disk format the reference's tools write and its loader reads:
  one headerless native-endian fp32 file per ``state_dict`` key inside a
  ``weights_bin/`` directory (reference ``save_weights.py:8-12`` writes them,
  ``cuda/tensor.cuh:126-147`` reads ``file_size / 4`` floats back,
  ``cuda/nn.cuh:21,58-61,113,117`` builds the file names);
* a deterministic synthetic generator.  Pretrained weights cannot be fetched
  offline, so parity and throughput runs use weights produced from a
  counter-based hash: the value of element ``i`` of tensor ``name`` depends on
  ``(seed, name, i)`` only, is computed in float64 and rounded once to fp32,
  so every host produces bit-identical tensors.

The layer table follows the reference's model factory
(``cuda/inference/main.cu:53-89,109-125``): bottleneck blocks with the stride
on the 3x3 convolution and a projection shortcut on block 0 of every stage.
ResNet-18/34, which the reference does not ship, follow torchvision's
``BasicBlock``: two 3x3 convolutions (the stride on the first), expansion 1,
stage widths 64/128/256/512, a projection shortcut on block 0 of stages 2-4.
"""
from __future__ import annotations

import os
from typing import Dict, Iterator, List, Tuple

import numpy as np

# stage widths (in, mid, out) and strides are the same for every depth
# (main.cu:116-119); only the block counts differ.
STAGE_WIDTHS = ((64, 64, 256), (256, 128, 512), (512, 256, 1024), (1024, 512, 2048))
STAGE_STRIDES = (1, 2, 2, 2)
DEPTHS = {
    "resnet50": (3, 4, 6, 3),
    "resnet101": (3, 4, 23, 3),
    "resnet152": (3, 8, 36, 3),  # main.cu:116-119
}
# torchvision's other bottleneck networks: name -> (depth, groups, width_per_group).  The bottleneck's middle
# width is planes * width_per_group // 64 * groups and conv2 is a 3x3 convolution with `groups` groups
# (weight [width, width // groups, 3, 3]); everything else is the ResNet of that depth.
FAMILY = {
    "resnext50_32x4d": (50, 32, 4),
    "resnext101_32x8d": (101, 32, 8),
    "resnext101_64x4d": (101, 64, 4),
    "wide_resnet50_2": (50, 1, 128),
    "wide_resnet101_2": (101, 1, 128),
}
# basic-block networks: not in DEPTHS, whose names are the bottleneck networks (depths_of)
BASIC_DEPTHS = {
    "resnet18": (2, 2, 2, 2),
    "resnet34": (3, 4, 6, 3),
}
BASIC_WIDTHS = (64, 128, 256, 512)
NUM_CLASSES = 1000
BN_FIELDS = ("weight", "bias", "running_mean", "running_var")


def depths_of(arch: str) -> Tuple[int, int, int, int]:
    try:
        return DEPTHS[f"resnet{FAMILY[arch][0]}"] if arch in FAMILY else DEPTHS[arch]
    except KeyError:
        raise ValueError(f"unknown arch {arch!r}; expected one of {sorted(list(DEPTHS) + list(FAMILY))}") from None


def family_of(arch: str) -> Tuple[int, int, int]:
    """(depth, groups, width_per_group) of a bottleneck network: (50, 1, 64) for resnet50,
    (50, 32, 4) for resnext50_32x4d, (50, 1, 128) for wide_resnet50_2."""
    if arch in FAMILY:
        return FAMILY[arch]
    depths_of(arch)  # raises for an unknown name
    return (int(arch[len("resnet"):]), 1, 64)


def stage_widths(arch: str) -> Tuple[Tuple[int, int, int], ...]:
    """(in, mid, out) per stage; mid = planes * width_per_group // 64 * groups."""
    _d, groups, wpg = family_of(arch)
    return tuple((cin, mid * wpg // 64 * groups, cout) for cin, mid, cout in STAGE_WIDTHS)


def conv_groups(arch: str, conv_name: str) -> int:
    """groups of a convolution: the family's for a bottleneck's conv2, 1 everywhere else."""
    if arch in FAMILY and conv_name.startswith("layer") and conv_name.endswith(".conv2"):
        return FAMILY[arch][1]
    return 1


def block_kind(arch: str) -> str:
    """"bottleneck" (ResNet-50/101/152) or "basic" (ResNet-18/34)."""
    if arch in BASIC_DEPTHS:
        return "basic"
    depths_of(arch)  # raises for an unknown name
    return "bottleneck"


def feature_width(arch: str) -> int:
    """Channels of the last stage, the input width of fc: 2048 or 512."""
    return BASIC_WIDTHS[-1] if block_kind(arch) == "basic" else STAGE_WIDTHS[-1][2]


def conv_specs(arch: str, replace_stride_with_dilation=(False, False, False)) -> List[Tuple[str, int, int, int, int, int]]:
    """(name, cin, cout, k, stride, pad) for every convolution, in forward order (conv_groups() gives
    the groups of a ResNeXt's conv2: its weight is [cout, cin // groups, k, k]).  With
    replace_stride_with_dilation (bottleneck networks) the strides are the dilated network's and a conv2's
    pad is its dilation (iter_blocks_dilated yields it by name)."""
    out = [("conv1", 3, 64, 7, 2, 3)]
    if any(replace_stride_with_dilation):
        for pre, b_in, mid, cout, b_stride, has_ds, dil in iter_blocks_dilated(arch, replace_stride_with_dilation):
            if has_ds:
                out.append((f"{pre}.downsample.0", b_in, cout, 1, b_stride, 0))
            out.append((f"{pre}.conv1", b_in, mid, 1, 1, 0))
            out.append((f"{pre}.conv2", mid, mid, 3, b_stride, dil))
            out.append((f"{pre}.conv3", mid, cout, 1, 1, 0))
        return out
    if block_kind(arch) == "basic":
        for pre, cin, cout, stride, has_ds in iter_basic_blocks(arch):
            if has_ds:
                out.append((f"{pre}.downsample.0", cin, cout, 1, stride, 0))
            out.append((f"{pre}.conv1", cin, cout, 3, stride, 1))
            out.append((f"{pre}.conv2", cout, cout, 3, 1, 1))
        return out
    for li, ((cin, mid, cout), stride, n) in enumerate(
        zip(stage_widths(arch), STAGE_STRIDES, depths_of(arch)), start=1
    ):
        for bi in range(n):
            pre = f"layer{li}.{bi}"
            b_in = cin if bi == 0 else cout
            b_stride = stride if bi == 0 else 1
            if bi == 0 and (b_stride != 1 or b_in != cout):
                out.append((f"{pre}.downsample.0", b_in, cout, 1, b_stride, 0))
            out.append((f"{pre}.conv1", b_in, mid, 1, 1, 0))
            out.append((f"{pre}.conv2", mid, mid, 3, b_stride, 1))
            out.append((f"{pre}.conv3", mid, cout, 1, 1, 0))
    return out


def bn_of(conv_name: str) -> str:
    """Name of the batch-norm that follows a convolution (main.cu:59-75,111-112)."""
    if conv_name.endswith("downsample.0"):
        return conv_name[:-1] + "1"
    head, _, tail = conv_name.rpartition("conv")
    return f"{head}bn{tail}"


def tensor_specs(arch: str) -> List[Tuple[str, Tuple[int, ...]]]:
    """Every file the loader reads: (state_dict key, shape)."""
    specs: List[Tuple[str, Tuple[int, ...]]] = []
    for name, cin, cout, k, _s, _p in conv_specs(arch):
        specs.append((f"{name}.weight", (cout, cin // conv_groups(arch, name), k, k)))
        bn = bn_of(name)
        for f in BN_FIELDS:
            specs.append((f"{bn}.{f}", (cout,)))
    specs.append(("fc.weight", (NUM_CLASSES, feature_width(arch))))
    specs.append(("fc.bias", (NUM_CLASSES,)))
    return specs


def param_count(arch: str) -> int:
    """Learnable parameters (running stats excluded), e.g. 25,557,032 for resnet50, 11,689,512 for
    resnet18."""
    n = 0
    for key, shape in tensor_specs(arch):
        if key.endswith("running_mean") or key.endswith("running_var"):
            continue
        n += int(np.prod(shape))
    return n


# --------------------------------------------------------------------------
# counter-based generator
# --------------------------------------------------------------------------
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _fnv1a64(text: str) -> int:
    h = 0xCBF29CE484222325
    for ch in text.encode("utf-8"):
        h ^= ch
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def uniform01(name: str, n: int, seed: int, offset: int = 0) -> np.ndarray:
    """n float64 values in [0,1) with 24 random bits each (exact in fp32)."""
    key = (_fnv1a64(name) ^ ((seed * 0xD1342543DE82EF95) & 0xFFFFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF
    idx = np.arange(offset, offset + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(key)
    bits = _splitmix64(ctr) >> np.uint64(40)
    return bits.astype(np.float64) * (1.0 / 16777216.0)


def _uniform(name: str, shape, lo: float, hi: float, seed: int) -> np.ndarray:
    n = int(np.prod(shape))
    u = uniform01(name, n, seed)
    return (lo + (hi - lo) * u).astype(np.float32).reshape(shape)


def generate_tensor(key: str, shape, seed: int = 0) -> np.ndarray:
    """Synthetic tensor for one state_dict key.

    conv: He-uniform over fan_in; BN gamma in [0.5,1.5), beta and running mean in
    [-0.1,0.1), running var in [0.5,1.5); fc uniform(+-1/sqrt(in)).  The last
    batch-norm of every block (bn3) gets a smaller gamma so the residual stream
    of the 50-block network stays O(1).  The fc bound stays 1/sqrt(2048) for every
    architecture.  Basic blocks: see generate_state.
    """
    if key.endswith("running_var"):
        return _uniform(key, shape, 0.5, 1.5, seed)
    if key.endswith("running_mean"):
        return _uniform(key, shape, -0.1, 0.1, seed)
    if key.startswith("fc."):
        bound = 1.0 / np.sqrt(2048.0)
        return _uniform(key, shape, -bound, bound, seed)
    if key.endswith(".bias"):
        return _uniform(key, shape, -0.1, 0.1, seed)
    if len(shape) == 4:
        fan_in = shape[1] * shape[2] * shape[3]
        bound = float(np.sqrt(6.0 / fan_in))
        return _uniform(key, shape, -bound, bound, seed)
    if ".bn3." in key:
        return _uniform(key, shape, 0.02, 0.1, seed)
    return _uniform(key, shape, 0.5, 1.5, seed)


def _basic_last_bn(key: str) -> bool:
    """gamma of a basic block's last batch-norm (layerX.Y.bn2.weight)"""
    return key.startswith("layer") and key.endswith(".bn2.weight")


def generate_state(arch: str, seed: int = 0) -> Dict[str, np.ndarray]:
    """Every tensor of `arch` from generate_tensor.  In a basic-block network the block's last
    batch-norm is bn2: its gamma gets the damping bn3's gets (generate_tensor itself, and with it
    every tensor of the bottleneck networks, is unchanged)."""
    basic = block_kind(arch) == "basic"
    out = {}
    for k, s in tensor_specs(arch):
        if basic and _basic_last_bn(k):
            out[k] = _uniform(k, s, 0.02, 0.1, seed)
        else:
            out[k] = generate_tensor(k, s, seed)
    return out


def _hw_pair(hw) -> Tuple[int, int]:
    """hw: one side (square) or (H, W)."""
    if isinstance(hw, (tuple, list)):
        h, w = hw
        return int(h), int(w)
    return int(hw), int(hw)


def generate_input(batch: int, seed: int = 0, hw=224, name: str = "input") -> np.ndarray:
    """[batch,3,H,W] NCHW fp32, uniform in [-2,2): image i depends on (seed, i) and the size only.
    hw: one side, or (H, W)."""
    h, w = _hw_pair(hw)
    per = 3 * h * w
    out = np.empty((batch, 3, h, w), dtype=np.float32)
    for i in range(batch):
        u = uniform01(name, per, seed, offset=i * per)
        out[i] = (-2.0 + 4.0 * u).astype(np.float32).reshape(3, h, w)
    return out


# --------------------------------------------------------------------------
# weights_bin/ directory format
# --------------------------------------------------------------------------
def save_weights_bin(state: Dict[str, np.ndarray], dir_name: str) -> None:
    """Write one raw fp32 file per key, like reference save_weights.py:8-12."""
    os.makedirs(dir_name, exist_ok=True)
    for key, arr in state.items():
        np.ascontiguousarray(arr, dtype=np.float32).tofile(os.path.join(dir_name, key))


def load_weights_bin(arch: str, dir_name: str) -> Dict[str, np.ndarray]:
    """Read the files the reference loader reads; other files (e.g.
    ``*.num_batches_tracked``, which an export contains) are ignored."""
    state = {}
    for key, shape in tensor_specs(arch):
        path = os.path.join(dir_name, key)
        arr = np.fromfile(path, dtype=np.float32)
        want = int(np.prod(shape))
        if arr.size != want:
            raise ValueError(f"{path}: {arr.size} floats on disk, expected {want} for {shape}")
        state[key] = arr.reshape(shape)
    return state


def iter_blocks(arch: str, replace_stride_with_dilation=(False, False, False)
                ) -> Iterator[Tuple[str, int, int, int, int, bool]]:
    """(prefix, cin, mid, cout, stride, has_downsample) per bottleneck block."""
    for blk in iter_blocks_dilated(arch, replace_stride_with_dilation):
        yield blk[:6]


def iter_blocks_dilated(arch: str, replace_stride_with_dilation=(False, False, False)
                        ) -> Iterator[Tuple[str, int, int, int, int, bool, int]]:
    """(prefix, cin, mid, cout, stride, has_downsample, dilation) per bottleneck block: torchvision's
    _make_layer.  A running dilation starts at 1; a flagged stage (layer2, layer3, layer4) doubles it and
    takes stride 1.  Block 0 of a stage runs conv2 at the stage's stride with the dilation from before the
    stage (and keeps its downsample: the widths differ), blocks 1.. with the current one; conv2's padding
    is its dilation."""
    flags = tuple(bool(f) for f in replace_stride_with_dilation)
    if len(flags) != 3:
        raise ValueError("replace_stride_with_dilation takes three flags: layer2, layer3, layer4")
    if any(flags) and block_kind(arch) == "basic":
        raise NotImplementedError("replace_stride_with_dilation is defined for bottleneck networks only")
    dilation = 1
    for li, ((cin, mid, cout), stride, n) in enumerate(
        zip(stage_widths(arch), STAGE_STRIDES, depths_of(arch)), start=1
    ):
        previous = dilation
        if li > 1 and flags[li - 2]:
            dilation *= 2
            stride = 1
        for bi in range(n):
            b_in = cin if bi == 0 else cout
            b_stride = stride if bi == 0 else 1
            # (torchvision: stride != 1 or inplanes != planes * expansion -- with the stage's stride)
            yield (f"layer{li}.{bi}", b_in, mid, cout, b_stride,
                   bi == 0 and (b_stride != 1 or b_in != cout), previous if bi == 0 else dilation)


def iter_basic_blocks(arch: str) -> Iterator[Tuple[str, int, int, int, bool]]:
    """(prefix, cin, cout, stride, has_downsample) per basic block of ResNet-18/34."""
    try:
        depths = BASIC_DEPTHS[arch]
    except KeyError:
        raise ValueError(f"{arch!r} is not a basic-block network; expected one of {sorted(BASIC_DEPTHS)}") from None
    prev = 64
    for li, (cout, stride, n) in enumerate(zip(BASIC_WIDTHS, STAGE_STRIDES, depths), start=1):
        for bi in range(n):
            b_in = prev if bi == 0 else cout
            b_stride = stride if bi == 0 else 1
            yield (f"layer{li}.{bi}", b_in, cout, b_stride, b_stride != 1 or b_in != cout)
        prev = cout


def forward_flops(arch: str, hw=224, replace_stride_with_dilation=(False, False, False)) -> int:
    """Algorithmic FLOPs of one image: 2 x MACs of every convolution (output sizes tracked through
    the network) and of fc.  8,178,368,512 for resnet50, 3,628,146,688 for resnet18 at 224 x 224.
    hw: one side (a square image) or (H, W).  replace_stride_with_dilation: the dilated network's (a
    dilated stage keeps its map, so everything behind it costs four times as much)."""
    dil = {}
    if any(replace_stride_with_dilation):
        dil = {f"{blk[0]}.conv2": blk[6] for blk in iter_blocks_dilated(arch, replace_stride_with_dilation)}

    def out2(n, k, s, p, d=1):
        return tuple((x + 2 * p - d * (k - 1) - 1) // s + 1 for x in n)
    size = _hw_pair(hw)
    total, block_in, last = 0, {}, size
    for name, cin, cout, k, s, p in conv_specs(arch, replace_stride_with_dilation):
        if name == "conv1":
            n_in = size
        else:
            pre = name.rsplit(".", 2)[0] if name.endswith("downsample.0") else name.rsplit(".", 1)[0]
            if pre not in block_in:   # first convolution of a block: the previous block's output
                block_in[pre] = last if len(block_in) else out2(last, 3, 2, 1)  # max-pool after the stem
            first = name.endswith(("downsample.0", ".conv1"))
            n_in = block_in[pre] if first else last
        n_out = out2(n_in, k, s, p, dil.get(name, 1))
        total += 2 * n_out[0] * n_out[1] * cout * (cin // conv_groups(arch, name)) * k * k
        last = n_out
    return total + 2 * feature_width(arch) * NUM_CLASSES
