"""Segmentation, the parts that need no GPU: the numpy restatement of the upsample's contract against torch, the
float64 head reference against a hand-built torch module, the seeded head weights, the state-dict split, and the
new symbols.

OP_SHAPES is the op list of tests/test_segmentation_gpu.py: (B, h, w, classes, src_channels, H, W)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import segmentation as S

SYMBOLS = ("rn_upsample_bilinear_forward", "rn_seg_head_create", "rn_seg_head_set_dtype", "rn_seg_head_set_tensor",
           "rn_seg_head_finalize", "rn_seg_head_destroy", "rn_seg_head_forward", "rn_model_forward_segment",
           "rn_model_forward_segment_u8")

OP_SHAPES = [(2, 7, 7, 21, 24, 56, 56), (1, 28, 28, 21, 24, 224, 224), (2, 3, 5, 21, 24, 37, 50), (1, 1, 1, 5, 8, 9, 9),
             (1, 9, 12, 8, 8, 5, 7), (1, 7, 7, 21, 24, 7, 7), (2, 4, 6, 150, 152, 32, 48), (1, 2, 9, 256, 256, 16, 18),
             (1, 2, 2, 1, 4, 8, 8)]
PAD = np.float32(1e30)  # what the padding channels hold: reading one would win every argmax


@functools.lru_cache(maxsize=None)
def op_source(shape):
    """seeded N(0,1) scores [B,h,w,src_channels], the padding channels +1e30; with 256 classes channel 255 is the
    largest at source pixel (0, 0), so that label 255 occurs.  Read-only, shared."""
    B, h, w, classes, cs, H, W = shape
    x = np.random.default_rng(sum(shape)).standard_normal((B, h, w, cs), dtype=np.float32)
    x[..., classes:] = PAD
    if classes == 256:
        x[0, 0, 0, 255] = 9.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def op_reference(shape):
    B, h, w, classes, cs, H, W = shape
    s, lb = S.upsample_bilinear_ref(op_source(shape), (H, W), classes)
    s.setflags(write=False), lb.setflags(write=False)
    return s, lb


def test_symbols_are_declared_exported_and_typed():
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rn_hip.h")).read()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None and name in L.SIGNATURES, name
        assert re.search(r"RN_API int " + name + r"\(", header), name
        assert getattr(lib, name).restype is ctypes.c_int and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert re.search(r"typedef struct rn_seg_outputs \{ uint8_t \*labels; float \*scores; \} rn_seg_outputs;", header)
    assert [f[0] for f in L.SegOutputs._fields_] == ["labels", "scores"]
    assert ctypes.sizeof(L.SegOutputs) == 2 * ctypes.sizeof(ctypes.c_void_p)
    assert callable(R.ops.upsample_bilinear) and callable(R.NativeModel.forward_segment)
    assert callable(R.NativeModel.forward_segment_u8) and callable(S.FCNHead.forward) and callable(S.FCNHead.close)


@pytest.mark.parametrize("shape", OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_contract_is_torchs_interpolate(shape):
    """upsample_bilinear_ref against F.interpolate(bilinear, align_corners=False) in float64:
    max|diff| <= (8 + 4 max(h, w)) 2^-24 max|x| (the rounding of src, of the weights and of the three sums); the
    source's bits where the sizes are equal; torch's argmax wherever float64's top-two gap exceeds twice that bound,
    at most 0.1 % of the pixels left out."""
    B, h, w, classes, cs, H, W = shape
    x = op_source(shape)
    got, labels = op_reference(shape)
    assert got.shape == (B, classes, H, W) and got.dtype == np.float32
    assert labels.shape == (B, H, W) and labels.dtype == np.uint8
    v = np.ascontiguousarray(x[..., :classes].transpose(0, 3, 1, 2))
    assert np.abs(v).max() < 100.0                                   # no padding channel among them
    want = F.interpolate(torch.from_numpy(v.astype(np.float64)), size=(H, W), mode="bilinear", align_corners=False).numpy()
    bound = (8 + 4 * max(h, w)) * 2.0 ** -24 * float(np.abs(v).max())
    err = float(np.abs(got - want).max())
    print(f"\n  upsample_bilinear_ref {shape}: max|ref - torch f64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if (h, w) == (H, W):
        assert np.array_equal(got.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(labels, got.argmax(axis=1))
    if classes == 1:
        assert not labels.any()
        return
    if classes == 256:
        assert (labels == 255).any()
    top2 = np.sort(want, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * bound
    left_out = 1.0 - clear.mean()
    print(f"  labels: {100 * left_out:.3f} % of the pixels inside twice the bound")
    assert left_out <= 1e-3
    assert np.array_equal(labels[clear], want.argmax(axis=1)[clear])


def test_contract_ties_take_the_lowest_index():
    x = np.random.default_rng(3).integers(-4, 4, (1, 3, 4, 12)).astype(np.float32)
    x[..., 3] = 9.0
    x[..., 7] = 9.0
    _, labels = S.upsample_bilinear_ref(x, (11, 13), 10)
    assert (labels == 3).all()


def test_generated_head_state():
    st = S.generate_fcn_head_state(128, 21, seed=1)
    assert tuple(st) == S.HEAD_KEYS
    assert {k: v.shape for k, v in st.items()} == S.head_shapes(128, 21)
    assert st["classifier.0.weight"].shape == (32, 128, 3, 3) and st["classifier.4.weight"].shape == (21, 32, 1, 1)
    assert all(v.dtype == np.float32 for v in st.values())
    again, other = S.generate_fcn_head_state(128, 21, seed=1), S.generate_fcn_head_state(128, 21, seed=2)
    assert all(np.array_equal(st[k], again[k]) for k in st)
    assert not np.array_equal(st["classifier.0.weight"], other["classifier.0.weight"])
    assert (st["classifier.1.running_var"] > 0).all()
    # not bias-dominated: on a random map the scores spread far wider than the bias, the bias's favourite class
    # does not win everywhere, and several classes win somewhere
    x = np.random.default_rng(11).standard_normal((2, 128, 6, 5))
    scores = S.fcn_head_ref(x, st, (6, 5))
    bias = st["classifier.4.bias"]
    spread = float((scores - bias[None, :, None, None]).std())
    assert np.abs(bias).max() <= 0.05 * spread, (np.abs(bias).max(), spread)
    labels = scores.argmax(axis=1)
    assert len(np.unique(labels)) >= 3
    assert (labels == int(bias.argmax())).mean() < 0.5
    nobias = dict(st, **{"classifier.4.bias": np.zeros_like(bias)})
    assert (S.fcn_head_ref(x, nobias, (6, 5)).argmax(axis=1) == labels).mean() > 0.9


def test_split_state():
    head = S.generate_fcn_head_state(512, 7, seed=0)
    full = {"backbone.conv1.weight": np.ones((64, 3, 7, 7), np.float32),
            "backbone.bn1.num_batches_tracked": np.array(5),
            "backbone.layer4.1.bn2.weight": torch.ones(512),
            "aux_classifier.0.weight": np.ones((64, 256, 3, 3), np.float32),
            "aux_classifier.4.bias": np.ones(7, np.float32)}
    full.update(head)
    full["classifier.1.num_batches_tracked"] = np.array(5)
    backbone, got = S.split_state(full)
    assert set(got) == set(S.HEAD_KEYS) and all(np.array_equal(got[k], head[k]) for k in head)
    assert set(backbone) == {"conv1.weight", "layer4.1.bn2.weight", "fc.weight", "fc.bias"}
    assert backbone["layer4.1.bn2.weight"].dtype == np.float32
    assert backbone["fc.weight"].shape == (4, 512) and not backbone["fc.weight"].any()
    assert backbone["fc.bias"].shape == (4,) and not backbone["fc.bias"].any()
    # an fc that is there stays
    full["backbone.fc.weight"], full["backbone.fc.bias"] = np.ones((10, 512), np.float32), np.ones(10, np.float32)
    backbone, _ = S.split_state(full)
    assert backbone["fc.weight"].shape == (10, 512) and backbone["fc.weight"].all()
    with pytest.raises(ValueError):
        S.split_state({"something.else": np.zeros(1)})


def test_head_reference_is_torchs_module():
    """fcn_head_ref against torchvision's FCNHead layers built by hand: Conv3x3 (no bias), BatchNorm, ReLU,
    Dropout, Conv1x1, in eval mode and float64, then interpolate"""
    cin, classes = 64, 5
    st = S.generate_fcn_head_state(cin, classes, seed=4)
    mod = torch.nn.Sequential(torch.nn.Conv2d(cin, cin // 4, 3, padding=1, bias=False), torch.nn.BatchNorm2d(cin // 4),
                              torch.nn.ReLU(), torch.nn.Dropout(0.1), torch.nn.Conv2d(cin // 4, classes, 1)).double().eval()
    mod.load_state_dict({k[len("classifier."):]: torch.from_numpy(v.astype(np.float64)) for k, v in st.items()},
                        strict=False)
    x = np.random.default_rng(8).standard_normal((2, cin, 5, 4))
    with torch.no_grad():
        want = F.interpolate(mod(torch.from_numpy(x)), size=(17, 9), mode="bilinear", align_corners=False).numpy()
    got = S.fcn_head_ref(x, st, (17, 9))
    assert got.dtype == np.float64 and got.shape == (2, classes, 17, 9)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the rounding hook touches the map, the weights and the mid tensor
    rounded = S.fcn_head_ref(x, st, (17, 9), round_fn=R.ops.bf16_round)
    assert 0 < np.abs(rounded - got).max() < 0.1 * np.abs(got).max()
