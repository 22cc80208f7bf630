"""Stage feature maps (rn_model_forward_maps), the parts that need no GPU: the four symbols, rn_model_stage_shape,
and the float64 reference of tests/test_stage_maps_gpu.py held to the references the project already has.

`stage_maps_f64` is dilated_features_f64 (tests/test_dilation_host.py) and netref's basic-block forward with the
block output kept at the end of every stage: torch functional on the CPU, float64, nothing of the code under test.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_c_amd as R
from oracle import netref as N
from resnet_c_amd import _lib as L
from resnet_c_amd import weights as W
from test_dilation_host import dilated_features_f64

SYMBOLS = ("rn_nhwc_to_nchw_dt", "rn_model_stage_shape", "rn_model_forward_maps", "rn_model_forward_maps_u8")


@torch.no_grad()
def stage_maps_f64(arch, state, x, flags=(0, 0, 0)):
    """the four maps [B,C,H,W] behind layer1..layer4, float64"""
    t = lambda k: torch.from_numpy(np.asarray(state[k], dtype=np.float64))
    bn = lambda name, y: F.batch_norm(y, t(f"{name}.running_mean"), t(f"{name}.running_var"), t(f"{name}.weight"),
                                      t(f"{name}.bias"), False, 0.0, 1e-5)
    h = torch.from_numpy(np.asarray(x, dtype=np.float64))
    h = F.max_pool2d(F.relu(bn("bn1", F.conv2d(h, t("conv1.weight"), stride=2, padding=3))), 3, 2, 1)
    maps = {}
    if W.block_kind(arch) == "basic":
        assert not any(flags)
        for pre, _cin, _cout, stride, has_ds in W.iter_basic_blocks(arch):
            y = F.relu(bn(f"{pre}.bn1", F.conv2d(h, t(f"{pre}.conv1.weight"), stride=stride, padding=1)))
            y = bn(f"{pre}.bn2", F.conv2d(y, t(f"{pre}.conv2.weight"), stride=1, padding=1))
            sc = bn(f"{pre}.downsample.1", F.conv2d(h, t(f"{pre}.downsample.0.weight"), stride=stride)) if has_ds else h
            h = F.relu(y + sc)
            maps[pre.split(".")[0]] = h        # the last block of a stage wins
    else:
        groups = W.family_of(arch)[1]
        for pre, _cin, _mid, _cout, stride, has_ds, d in W.iter_blocks_dilated(arch, flags):
            y = F.relu(bn(f"{pre}.bn1", F.conv2d(h, t(f"{pre}.conv1.weight"))))
            y = F.relu(bn(f"{pre}.bn2", F.conv2d(y, t(f"{pre}.conv2.weight"), stride=stride, padding=d, dilation=d,
                                                 groups=groups)))
            y = bn(f"{pre}.bn3", F.conv2d(y, t(f"{pre}.conv3.weight")))
            sc = bn(f"{pre}.downsample.1", F.conv2d(h, t(f"{pre}.downsample.0.weight"), stride=stride)) if has_ds else h
            h = F.relu(y + sc)
            maps[pre.split(".")[0]] = h
    return [maps[f"layer{i}"].numpy() for i in (1, 2, 3, 4)]


def test_symbols_are_declared_exported_and_typed():
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rn_hip.h")).read()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None and name in L.SIGNATURES, name
        assert re.search(r"RN_API int " + name + r"\(", header), name
        assert getattr(lib, name).restype is ctypes.c_int and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert re.search(r"typedef struct rn_model_maps \{ float \*layer\[4\]; \} rn_model_maps;", header)
    assert ctypes.sizeof(L.ModelMaps) == 4 * ctypes.sizeof(ctypes.c_void_p)
    # rn_model_outputs keeps its layout
    assert [f[0] for f in L.ModelOutputs._fields_] == ["logits", "features", "probs", "topk_prob", "topk_idx", "k"]
    assert ctypes.sizeof(L.ModelOutputs) == 48


def _model(arch, size=None, flags=None):
    """An unfinalized model whose context is never used (as in test_input_size_host.py): creation, the geometry
    and rn_model_stage_shape are pure host code.  Returns (handle, the buffer standing in for the context)."""
    lib = L.lib()
    ctx = ctypes.create_string_buffer(1 << 16)
    h = ctypes.c_void_p()
    if arch in W.FAMILY:
        assert lib.rn_model_create_ex(ctypes.addressof(ctx), ctypes.byref(h), *W.FAMILY[arch]) == L.RN_OK
    else:
        assert lib.rn_model_create(ctypes.addressof(ctx), ctypes.byref(h), R.model.ARCH_ID[arch]) == L.RN_OK
    if size:
        assert lib.rn_model_set_input_size(h, *size) == L.RN_OK
    if flags:
        assert lib.rn_model_set_dilation(h, *flags) == L.RN_OK
    return h, ctx


def _shapes(h):
    out = []
    for stage in (1, 2, 3, 4):
        c, hh, w = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        assert L.lib().rn_model_stage_shape(h, stage, ctypes.byref(c), ctypes.byref(hh), ctypes.byref(w)) == L.RN_OK
        out.append((c.value, hh.value, w.value))
    return out


SHAPE_CASES = [
    ("resnet50", None, None, [(256, 56, 56), (512, 28, 28), (1024, 14, 14), (2048, 7, 7)]),
    ("resnet50", (33, 47), None, [(256, 9, 12), (512, 5, 6), (1024, 3, 3), (2048, 2, 2)]),
    ("resnet50", (64, 96), (0, 1, 1), [(256, 16, 24), (512, 8, 12), (1024, 8, 12), (2048, 8, 12)]),
    ("resnet50", None, (0, 1, 1), [(256, 56, 56), (512, 28, 28), (1024, 28, 28), (2048, 28, 28)]),
    ("resnet18", None, None, [(64, 56, 56), (128, 28, 28), (256, 14, 14), (512, 7, 7)]),
    ("wide_resnet50_2", None, None, [(256, 56, 56), (512, 28, 28), (1024, 14, 14), (2048, 7, 7)]),
]
IDS = ["resnet50-224", "resnet50-33x47", "resnet50-64x96-011", "resnet50-224-011", "resnet18", "wide_resnet50_2"]


@pytest.mark.parametrize("arch,size,flags,want", SHAPE_CASES, ids=IDS)
def test_stage_shape(arch, size, flags, want):
    h, _ctx = _model(arch, size, flags)
    try:
        assert _shapes(h) == want
        for stage in (0, 5, -1):
            assert L.lib().rn_model_stage_shape(h, stage, None, None, None) == L.RN_ERR_INVALID
        assert L.lib().rn_model_stage_shape(h, 2, None, None, None) == L.RN_OK      # any pointer may be NULL
        assert L.lib().rn_model_stage_shape(None, 1, None, None, None) == L.RN_ERR_INVALID
    finally:
        L.lib().rn_model_destroy(h)


REF_CASES = [("resnet50", (64, 64), (0, 0, 0)), ("resnet50", (33, 47), (0, 0, 0)), ("resnet50", (64, 96), (0, 1, 1)),
             ("resnet18", (64, 64), (0, 0, 0))]


@pytest.mark.parametrize("arch,size,flags", REF_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_reference_maps_agree_with_the_feature_references_and_the_shapes(arch, size, flags):
    """the float64 maps: layer4's mean over H, W is the project's float64 features (1e-12 relative), and their shapes
    are rn_model_stage_shape's"""
    state = W.generate_state(arch, seed=0)
    x = W.generate_input(2, seed=300 + size[0] + size[1], hw=size)
    maps = stage_maps_f64(arch, state, x, flags)
    feats = maps[3].mean(axis=(2, 3))
    want = dilated_features_f64(arch, state, x, flags) if W.block_kind(arch) != "basic" else N.features_f64(arch, state, x)
    assert np.abs(feats - want).max() <= 1e-12 * np.abs(want).max()
    if not any(flags):
        other = N.features_f64(arch, state, x)
        assert np.abs(feats - other).max() <= 1e-12 * np.abs(other).max()
    h, _ctx = _model(arch, size, flags if any(flags) else None)
    try:
        assert [m.shape for m in maps] == [(2,) + s for s in _shapes(h)]
    finally:
        L.lib().rn_model_destroy(h)


def test_python_surface():
    assert isinstance(R.NativeModel.stage_shapes, property)
    for f in ("forward_maps", "forward_maps_u8"):
        assert callable(getattr(R.NativeModel, f))
    assert callable(R.ops.nhwc_to_nchw_dt)
    assert R.NativeModel.STAGES == ("layer1", "layer2", "layer3", "layer4")
