"""DeepLabV3 head on the host: torchvision's keys and arithmetic, the references the GPU tests hold the device to.

torchvision is not installed where the suite runs, so its DeepLabHead is assembled here from torch.nn exactly as its
source does (ASPPConv, ASPPPooling, ASPP, DeepLabHead under the name `classifier`); the state dict that
segmentation.generate_deeplab_head_state draws must load into it strictly, and segmentation.deeplab_head_ref must be
its arithmetic in float64 -- which also pins "the pooled branch is broadcast" against "bilinear from a 1x1 map".
The cases (H1, H2, the model-sized head) and seeds are the ones tests/test_deeplab_gpu.py runs; it imports them.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from resnet_c_amd import _lib as L
from resnet_c_amd import ops
from resnet_c_amd import segmentation as S
from test_dilation_gpu import tol_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (in_channels, aspp_channels, classes, (B, h, w), size, rates)
H1 = (128, 64, 21, (2, 6, 5), (24, 20), (2, 3, 6))       # rates 2 and 3 reach inside the map, rate 6 is centre-only
H2 = (512, 64, 7, (1, 4, 4), (32, 32), (12, 24, 36))     # all three centre-only; the pooled 1x1 has M = 1
MODEL = (2048, 256, 21, (3, 8, 8), (64, 64), (2, 4, 12))  # the head of the model tests, on a random 8 x 8 map here
CASES = {"H1": H1, "H2": H2, "model": MODEL}
HEAD_SEED = 0   # the float64 reference labels of this seed hold 10 (H1), 4 (H2) and 12 (model) distinct classes

# the concat cases of the GPU test: (channels of the sources, broadcast channels or 0, B, pixels) in elements of 4 bytes;
# the bf16 runs double every count (the same bytes)
CONCAT_CASES = {"aspp": ((64, 64, 128), 64, 3, 30), "one_chunk": ((4,), 0, 1, 1), "eight": ((8,) * 8, 0, 2, 257),
                "broadcast": ((8,), 12, 2, 7)}


# ---------------------------------------------------------------------------------------------------------------------
# torchvision.models.segmentation.deeplabv3, restated
# ---------------------------------------------------------------------------------------------------------------------
class ASPPConv(nn.Sequential):
    def __init__(self, cin, cout, dilation):
        super().__init__(nn.Conv2d(cin, cout, 3, padding=dilation, dilation=dilation, bias=False), nn.BatchNorm2d(cout),
                         nn.ReLU())


class ASPPPooling(nn.Sequential):
    def __init__(self, cin, cout):
        super().__init__(nn.AdaptiveAvgPool2d(1), nn.Conv2d(cin, cout, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU())

    def forward(self, x):
        size = x.shape[-2:]
        for mod in self:
            x = mod(x)
        return F.interpolate(x, size=size, mode="bilinear", align_corners=False)


class ASPP(nn.Module):
    def __init__(self, cin, rates, cout=256):
        super().__init__()
        mods = [nn.Sequential(nn.Conv2d(cin, cout, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU())]
        mods += [ASPPConv(cin, cout, r) for r in rates]
        mods.append(ASPPPooling(cin, cout))
        self.convs = nn.ModuleList(mods)
        self.project = nn.Sequential(nn.Conv2d(len(self.convs) * cout, cout, 1, bias=False), nn.BatchNorm2d(cout),
                                     nn.ReLU(), nn.Dropout(0.5))

    def forward(self, x):
        return self.project(torch.cat([conv(x) for conv in self.convs], dim=1))


class TorchvisionDeepLab(nn.Module):
    """DeepLabHead(in_channels, classes) as the `classifier` of a deeplabv3 model"""

    def __init__(self, cin, classes, rates, a=256):
        super().__init__()
        self.classifier = nn.Sequential(ASPP(cin, rates, a), nn.Conv2d(a, a, 3, padding=1, bias=False), nn.BatchNorm2d(a),
                                        nn.ReLU(), nn.Conv2d(a, classes, 1))

    def forward(self, x, size):
        return F.interpolate(self.classifier(x), size=size, mode="bilinear", align_corners=False)


def module_of(cin, a, classes, rates, state):
    mod = TorchvisionDeepLab(cin, classes, rates, a)
    missing, unexpected = mod.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith("num_batches_tracked") for k in missing), missing
    return mod.double().eval()


# ---------------------------------------------------------------------------------------------------------------------
# the shared references: computed once, read-only
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_state(case):
    cin, a, classes, _bhw, _size, rates = CASES[case]
    st = S.generate_deeplab_head_state(cin, classes, a, rates, seed=HEAD_SEED)
    for v in st.values():
        v.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def head_map(case):
    """the NHWC fp32 map of a head-alone case"""
    cin, _a, classes, (B, h, w), _size, _rates = CASES[case]
    x = np.random.default_rng(cin + classes).standard_normal((B, h, w, cin), dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def head_ref(case, bf16=False):
    """float64 scores of the case (bf16: rounded where a bf16 head stores)"""
    _cin, _a, _classes, _bhw, size, rates = CASES[case]
    ref = S.deeplab_head_ref(head_map(case).transpose(0, 3, 1, 2).astype(np.float64), head_state(case), size, rates,
                             round_fn=ops.bf16_round if bf16 else None)
    ref.setflags(write=False)
    return ref


def concat_sources(case, bf16, special=False):
    """(sources [B, pixels, C_i], per_image [B, C_p] or None) of a concat case as the bit patterns the device copies:
    uint32 words for fp32, uint16 for bf16.  special: NaN payloads, infinities and both zeros among them."""
    chans, cp, B, pixels = CONCAT_CASES[case]
    mul, dt = (2, np.uint16) if bf16 else (1, np.uint32)
    rng = np.random.default_rng(len(chans) * 100 + cp + B + pixels)

    def draw(shape):
        f = rng.standard_normal(shape, dtype=np.float32)
        v = ops.to_bf16_bits(f).reshape(shape) if bf16 else f.view(np.uint32).copy()
        if special:  # quiet and signalling NaNs with payloads, -0, +0, +inf, -inf
            pats = np.array([0x7FC1, 0xFFD2, 0x7F81, 0x8000, 0x0000, 0x7F80, 0xFF80] if bf16 else
                            [0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000], dtype=dt)
            flat = v.reshape(-1)
            flat[::3] = pats[np.arange(flat[::3].size) % pats.size]
        return v.astype(dt)

    srcs = [draw((B, pixels, c * mul)) for c in chans]
    per = draw((B, cp * mul)) if cp else None
    return srcs, per


# ---------------------------------------------------------------------------------------------------------------------
# keys, shapes, arithmetic
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rates", [(5,), (12, 24, 36), (1, 2, 3, 4)], ids=["n1", "n3", "n4"])
def test_state_loads_into_torchvisions_module(rates):
    cin, a, classes = 64, 64, 5
    st = S.generate_deeplab_head_state(cin, classes, a, rates, seed=3)
    mod = TorchvisionDeepLab(cin, classes, rates, a)
    want = {k: tuple(v.shape) for k, v in mod.state_dict().items() if not k.endswith("num_batches_tracked")}
    shapes = S.deeplab_head_shapes(cin, classes, a, rates)
    assert shapes == want and list(shapes) == list(want)
    assert {k: v.shape for k, v in st.items()} == want
    # strict: nothing unexpected, nothing missing but the counters
    full = dict(mod.state_dict())
    full.update({k: torch.from_numpy(v.copy()) for k, v in st.items()})
    mod.load_state_dict(full, strict=True)
    assert set(full) - set(st) == {k for k in full if k.endswith("num_batches_tracked")}
    # every key draws its own numbers
    flat = [v.reshape(-1)[:4].tobytes() for v in st.values()]
    assert len(set(flat)) == len(flat)


def test_default_shapes_are_torchvisions():
    mod = TorchvisionDeepLab(2048, 21, (12, 24, 36))
    want = {k: tuple(v.shape) for k, v in mod.state_dict().items() if not k.endswith("num_batches_tracked")}
    assert S.deeplab_head_shapes(2048, 21) == want


@pytest.mark.parametrize("case", ["H1", "H2"])
def test_reference_is_torchvisions_arithmetic(case):
    cin, a, classes, _bhw, size, rates = CASES[case]
    mod = module_of(cin, a, classes, rates, head_state(case))
    x = torch.from_numpy(head_map(case).transpose(0, 3, 1, 2).astype(np.float64))
    with torch.no_grad():
        want = mod(x, size).numpy()
    got = head_ref(case)
    err = float(np.abs(got - want).max())
    assert got.shape == want.shape and err <= 1e-12 * float(np.abs(want).max()), err


def test_split_state_takes_a_deeplab_state():
    cin, a, classes, rates = 64, 64, 3, (2, 4)
    head = S.generate_deeplab_head_state(cin, classes, a, rates, seed=1)
    state = dict(head)
    state["backbone.conv1.weight"] = np.ones((64, 3, 7, 7), np.float32)
    state["backbone.bn1.num_batches_tracked"] = np.zeros((), np.int64)
    state["classifier.0.convs.0.1.num_batches_tracked"] = np.zeros((), np.int64)
    state["aux_classifier.0.weight"] = np.ones((16, 32, 3, 3), np.float32)
    state["aux_classifier.4.bias"] = np.ones((3,), np.float32)
    backbone, got = S.split_state(state)
    assert set(got) == set(head) and all(np.array_equal(got[k], head[k]) for k in head)
    assert set(backbone) == {"conv1.weight", "fc.weight", "fc.bias"}
    assert backbone["fc.weight"].shape == (4, cin) and not backbone["fc.weight"].any() and not backbone["fc.bias"].any()


def test_centre_tap_premise_in_float64():
    """H2: every rate is at least the map's height and width, so each dilated branch is the 1x1 convolution with
    weight[:, :, 1, 1]"""
    cin, _a, _classes, (_B, h, w), _size, rates = H2
    st = head_state("H2")
    x = torch.from_numpy(head_map("H2").transpose(0, 3, 1, 2).astype(np.float64))
    for i, r in enumerate(rates, start=1):
        assert r >= h and r >= w
        wt = torch.from_numpy(st[f"classifier.0.convs.{i}.0.weight"].astype(np.float64))
        full = F.conv2d(x, wt, padding=r, dilation=r)
        centre = F.conv2d(x, wt[:, :, 1:2, 1:2].contiguous())
        assert float((full - centre).abs().max()) <= 1e-12 * float(full.abs().max())


@pytest.mark.parametrize("case", ["H1", "H2", "model"])
def test_reference_labels_are_diverse(case):
    labels = head_ref(case).argmax(axis=1)
    assert len(np.unique(labels)) >= 3, np.unique(labels)


@pytest.mark.parametrize("case", ["H1", "H2", "model"])
def test_fp32_yardstick(case):
    """torch float32 on the CPU against float64: at most a tenth of the bound the GPU test gives the fp32 head, so
    the bound of the single convolutions covers the deeper chain"""
    cin, a, classes, _bhw, size, rates = CASES[case]
    mod = module_of(cin, a, classes, rates, head_state(case)).float()
    with torch.no_grad():
        got = mod(torch.from_numpy(head_map(case).transpose(0, 3, 1, 2).copy()), size).numpy().astype(np.float64)
    ref = head_ref(case)
    err, tol = float(np.abs(got - ref).max()), tol_f32(ref, 9 * cin)
    print(f"\n  DeepLabHead {case}: max|torch fp32 - fp64| = {err:.3e}, a tenth of the bound {tol / 10:.3e}")
    assert err <= tol / 10


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(CONCAT_CASES))
def test_concat_reference(case, bf16):
    """ops.concat_channels_ref is numpy.concatenate plus numpy.broadcast_to, on the bit patterns themselves"""
    srcs, per = concat_sources(case, bf16, special=True)
    chans, cp, B, pixels = CONCAT_CASES[case]
    mul = 2 if bf16 else 1
    want = ops.concat_channels_ref(srcs, per)
    assert want.dtype == srcs[0].dtype and want.shape == (B, pixels, (sum(chans) + cp) * mul)
    assert all(s.shape[2] * s.dtype.itemsize % 16 == 0 for s in srcs)
    at = 0
    for s in srcs:
        assert np.array_equal(want[:, :, at:at + s.shape[2]], s)
        at += s.shape[2]
    if per is not None:
        for p in range(pixels):
            assert np.array_equal(want[:, p, at:], per)
    else:
        assert at == want.shape[2]


def test_surface():
    text = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    declared = set(re.findall(r"RN_API[^;(]*?\b(rn_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rn_[a-z0-9_]+)", out))
    lib = L.lib()
    for name in ("rn_concat_channels_forward_dt", "rn_seg_head_create_deeplab", "rn_seg_head_set_center_tap"):
        assert name in declared and name in exported and name in L.SIGNATURES and hasattr(lib, name), name
