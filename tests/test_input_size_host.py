"""The model's input size on the host: the exported surface, the size rules of rn_model_set_input_size (pure host
code on a model whose context is never used), the sub-batch rule, and weights.forward_flops on rectangles."""
import ctypes
import os
import re
import subprocess

import pytest

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import ops, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rn_global_avgpool_nhwc_forward_dt", "rn_model_set_input_size", "rn_model_input_size", "rn_model_max_sub_batch"]
SIZES = [(32, 32), (64, 96), (44, 64), (104, 72), (40, 272), (224, 224), (1024, 1024)]


def test_new_symbols_are_declared_exported_and_typed():
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rn_[a-z0-9_]+)", out))
    for n in NEW:
        assert re.search(r"RN_API[^;(]*?\b%s\s*\(" % n, header), n
        assert n in exported and hasattr(lib, n) and n in L.SIGNATURES, n
    for n in ("rn_stem_pool_applies", "rn_model_pipeline_attach", "rn_model_pipeline_detach", "rn_ctx_set_error"):
        assert n not in exported, n  # library-internal
    assert callable(ops.global_avgpool)
    assert "input_size" in R.NativeModel.__init__.__code__.co_varnames
    assert isinstance(R.NativeModel.input_size, property)
    for f in ("set_input_size", "max_sub_batch"):
        assert callable(getattr(R.NativeModel, f))


class _HostModel:
    """A model whose context is never used (as in test_head_host.py): creation, the size and the sub-batch rule
    are pure host code as long as no forward has run."""

    def __init__(self, arch):
        self.ctx = ctypes.create_string_buffer(1 << 16)
        self.h = ctypes.c_void_p()
        assert L.lib().rn_model_create(ctypes.addressof(self.ctx), ctypes.byref(self.h), arch) == L.RN_OK

    def size(self):
        h, w = ctypes.c_uint64(), ctypes.c_uint64()
        assert L.lib().rn_model_input_size(self.h, ctypes.byref(h), ctypes.byref(w)) == L.RN_OK
        return h.value, w.value

    def close(self):
        L.lib().rn_model_destroy(self.h)


def out_size(n, k, s, p):
    """the output-size rule restated (ops.cuh: integer division)"""
    return (n + 2 * p - k) // s + 1


def chain(n):
    """stem 7/2/3, max-pool 3/2/1, stage 1 keeps, stages 2-4 3/2/1: the sides a ResNet sees"""
    stem = out_size(n, 7, 2, 3)
    pool = out_size(stem, 3, 2, 1)
    s2 = out_size(pool, 3, 2, 1)
    s3 = out_size(s2, 3, 2, 1)
    return [stem, pool, pool, s2, s3, out_size(s3, 3, 2, 1)]


def expected_cap(arch, H, W):
    """§ 'sub-batch cap': the largest power of two <= 512 with (largest per-image arena tensor) * cap < 2^29"""
    basic = arch in (18, 34)
    sh, ph = chain(H)[:2]
    sw, pw = chain(W)[:2]
    x4 = (H + 6) * (W + 6) * 4
    stem = sh * sw * 64
    s1 = ph * pw * (64 if basic else 256)
    t1 = ph * pw * (64 if basic else 128)
    largest = max(x4, stem, s1, t1)
    cap = 512
    while cap and largest * cap >= 1 << 29:
        cap //= 2
    return cap


@pytest.mark.parametrize("arch", [18, 50])
def test_size_rules_and_sub_batch_cap(arch):
    lib, m = L.lib(), _HostModel(arch)
    try:
        assert m.size() == (224, 224) and lib.rn_model_max_sub_batch(m.h) == 512
        for H, W in [(31, 224), (224, 31), (2049, 224), (224, 2049), (0, 0)]:
            assert lib.rn_model_set_input_size(m.h, H, W) == L.RN_ERR_INVALID
            assert m.size() == (224, 224) and lib.rn_model_max_sub_batch(m.h) == 512
        for H, W in SIZES + [(2048, 2048), (32, 2048), (256, 256)]:
            assert lib.rn_model_set_input_size(m.h, H, W) == L.RN_OK
            assert m.size() == (H, W)
            cap = lib.rn_model_max_sub_batch(m.h)
            assert cap == expected_cap(arch, H, W) and cap >= 1, (H, W, cap)
        assert lib.rn_model_set_input_size(m.h, 1024, 1024) == L.RN_OK
        # the stem tensor is 512 * 512 * 64 = 2^24 elements: 32 of them are 2^29, which is not below 2^29
        assert lib.rn_model_max_sub_batch(m.h) == 16
        assert lib.rn_model_set_input_size(None, 64, 64) == L.RN_ERR_INVALID
        assert lib.rn_model_max_sub_batch(None) == 0
    finally:
        m.close()


@pytest.mark.parametrize("n", sorted({s for hw in SIZES for s in hw}))
def test_output_size_chain_matches_the_library(n):
    lib = L.lib()
    stem = lib.rn_conv_output_size(n, 7, 2, 3)
    pool = lib.rn_conv_output_size(stem, 3, 2, 1)
    got, side = [stem, pool, pool], pool
    for _ in range(3):
        side3, side1 = lib.rn_conv_output_size(side, 3, 2, 1), lib.rn_conv_output_size(side, 1, 2, 0)
        assert side3 == side1  # conv2 / conv1 of a stage's first block and its 1x1 downsample agree
        got.append(side3)
        side = side3
    assert got == chain(n)
    assert got[-1] == -(-n // 32)  # the final map: ceil(n / 32)


def independent_flops(arch, H, W):
    """2 x MACs of every convolution and of fc, from conv_specs and the block structure alone"""
    specs = {name: (cin, cout, k, s, p) for name, cin, cout, k, s, p in weights.conv_specs(arch)}
    h, w = chain(H)[1], chain(W)[1]  # after the max-pool
    cin, cout, k, s, p = specs["conv1"]
    total = 2 * chain(H)[0] * chain(W)[0] * cout * cin * k * k
    blocks = []
    for name in specs:
        pre = name.rsplit(".", 2)[0] if name.endswith("downsample.0") else name.rsplit(".", 1)[0]
        if name != "conv1" and pre not in blocks:
            blocks.append(pre)
    for pre in blocks:
        bh, bw = h, w  # the block's input
        for conv in ("conv1", "conv2", "conv3"):
            if f"{pre}.{conv}" not in specs:
                continue
            cin, cout, k, s, p = specs[f"{pre}.{conv}"]
            h, w = out_size(h, k, s, p), out_size(w, k, s, p)
            total += 2 * h * w * cout * (cin // weights.conv_groups(arch, f"{pre}.{conv}")) * k * k
        if f"{pre}.downsample.0" in specs:
            cin, cout, k, s, p = specs[f"{pre}.downsample.0"]
            assert (out_size(bh, k, s, p), out_size(bw, k, s, p)) == (h, w)
            total += 2 * h * w * cout * cin * k * k
    return total + 2 * weights.feature_width(arch) * weights.NUM_CLASSES


@pytest.mark.parametrize("arch", ["resnet18", "resnet50", "resnext50_32x4d"])
def test_forward_flops_rectangular(arch):
    old = {"resnet50": 8178368512, "resnet18": 3628146688}
    assert weights.forward_flops(arch) == weights.forward_flops(arch, hw=224) == weights.forward_flops(arch, (224, 224))
    if arch in old:
        assert weights.forward_flops(arch, hw=224) == old[arch]
    assert weights.forward_flops(arch, hw=160) == weights.forward_flops(arch, hw=(160, 160))
    for H, W in SIZES[:6]:
        assert weights.forward_flops(arch, hw=(H, W)) == independent_flops(arch, H, W), (H, W)
    assert weights.forward_flops(arch, (64, 96)) == weights.forward_flops(arch, (96, 64))
    assert weights.forward_flops(arch, (64, 96)) != weights.forward_flops(arch, (64, 64))


def test_generate_input_rectangular():
    x = weights.generate_input(2, seed=5, hw=(40, 56))
    assert x.shape == (2, 3, 40, 56) and x.dtype.name == "float32"
    assert (weights.generate_input(1, seed=5, hw=64) == weights.generate_input(1, seed=5, hw=(64, 64))).all()
