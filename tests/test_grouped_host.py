"""Grouped convolution and the ResNeXt / Wide ResNet layer tables, host side (no GPU).

The per-group oracle -- oracle.conv2d (the CPU restatement of the reference's loop) applied to each
group's channel slices and concatenated -- is the definition of a grouped convolution in the
reference's summation order; tests/test_grouped_gpu.py holds the kernels to it.  Here it is held to
torch.nn.functional.conv2d(groups=) in float64.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_c_amd as R
from oracle import netref as N
from oracle import oracle as O
from resnet_c_amd import _lib as L
from resnet_c_amd import weights as W

NEW = {  # name -> (depth name, groups, width_per_group, torchvision's published parameter count)
    "resnext50_32x4d": ("resnet50", 32, 4, 25_028_904),
    "resnext101_32x8d": ("resnet101", 32, 8, 88_791_336),
    "resnext101_64x4d": ("resnet101", 64, 4, 83_455_272),
    "wide_resnet50_2": ("resnet50", 1, 128, 68_883_240),
    "wide_resnet101_2": ("resnet101", 1, 128, 126_886_696),
}


def grouped_oracle(x, w, stride, pad, groups):
    """oracle.conv2d per group on channel slices, concatenated"""
    cg, og = x.shape[1] // groups, w.shape[0] // groups
    return np.concatenate([O.conv2d(np.ascontiguousarray(x[:, g * cg:(g + 1) * cg]),
                                    np.ascontiguousarray(w[g * og:(g + 1) * og]), stride, pad)
                           for g in range(groups)], axis=1)


@pytest.mark.parametrize("case", [(2, 32, 32, 8, 7, 9, 3, 1, 1), (1, 64, 64, 2, 6, 5, 3, 2, 1), (2, 12, 8, 4, 5, 5, 1, 1, 0)])
def test_per_group_oracle_is_torch_grouped_convolution(case):
    B, Cin, Cout, G, H, Wd, k, s, p = case
    g = np.random.default_rng(sum(case))
    x = g.standard_normal((B, Cin, H, Wd), dtype=np.float32)
    w = g.standard_normal((Cout, Cin // G, k, k), dtype=np.float32)
    got = grouped_oracle(x, w, s, p, G)
    ref = F.conv2d(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w.astype(np.float64)), stride=s,
                   padding=p, groups=G).numpy()
    K = k * k * Cin // G
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 2e-6 * np.sqrt(K) * np.abs(ref).max() + 1e-6


@pytest.mark.parametrize("arch", sorted(NEW))
def test_layer_table(arch):
    base, groups, wpg, _ = NEW[arch]
    assert W.family_of(arch) == (int(base[6:]), groups, wpg)
    assert W.family_of(base) == (int(base[6:]), 1, 64)
    widths = W.stage_widths(arch)
    assert [m for _, m, _ in widths] == [planes * wpg // 64 * groups for planes in (64, 128, 256, 512)]
    assert [(i, o) for i, _, o in widths] == [(i, o) for i, _, o in W.STAGE_WIDTHS]
    specs, ref = dict(W.tensor_specs(arch)), dict(W.tensor_specs(base))
    assert list(k for k, _ in W.tensor_specs(arch)) == list(k for k, _ in W.tensor_specs(base))   # the key names
    for (pre, cin, mid, cout, stride, has_ds) in W.iter_blocks(arch):
        assert specs[f"{pre}.conv1.weight"] == (mid, cin, 1, 1)
        assert specs[f"{pre}.conv2.weight"] == (mid, mid // groups, 3, 3)
        assert specs[f"{pre}.conv3.weight"] == (cout, mid, 1, 1)
        assert specs[f"{pre}.bn2.weight"] == (mid,)
        assert W.conv_groups(arch, f"{pre}.conv2") == groups and W.conv_groups(arch, f"{pre}.conv1") == 1
        assert (f"{pre}.downsample.0.weight" in specs) == has_ds
    assert specs["fc.weight"] == ref["fc.weight"] == (1000, 2048)
    for name, cin, cout, k, s, p in W.conv_specs(arch):
        assert k == 3 or W.conv_groups(arch, name) == 1


def closed_form_params(depths, groups, wpg):
    """conv + learnable batch-norm + fc terms of torchvision's bottleneck ResNet"""
    n = 64 * 3 * 49 + 2 * 64
    cin = 64
    for planes, blocks, stride in zip((64, 128, 256, 512), depths, (1, 2, 2, 2)):
        width, cout = planes * wpg // 64 * groups, 4 * planes
        for b in range(blocks):
            n += cin * width + 2 * width + width * (width // groups) * 9 + 2 * width + width * cout + 2 * cout
            if b == 0:
                n += cin * cout + 2 * cout
            cin = cout
    return n + 2048 * 1000 + 1000


@pytest.mark.parametrize("arch", sorted(NEW) + ["resnet50"])
def test_param_count_is_torchvisions(arch):
    base, groups, wpg, published = NEW.get(arch, ("resnet50", 1, 64, 25_557_032))
    assert W.param_count(arch) == closed_form_params(W.DEPTHS[base], groups, wpg) == published


@pytest.mark.parametrize("arch", sorted(NEW) + ["resnet50"])
def test_forward_flops_hand_formula(arch):
    base, groups, wpg, _ = NEW.get(arch, ("resnet50", 1, 64, 0))
    total = 2 * 112 * 112 * 64 * 147
    cin, hw = 64, 56
    for planes, blocks, stride in zip((64, 128, 256, 512), W.DEPTHS[base], (1, 2, 2, 2)):
        width, cout = planes * wpg // 64 * groups, 4 * planes
        for b in range(blocks):
            s = stride if b == 0 else 1
            ho = hw // s
            total += 2 * hw * hw * width * cin                       # conv1 at the input resolution
            total += 2 * ho * ho * width * (width // groups) * 9     # conv2 carries the stride
            total += 2 * ho * ho * cout * width
            if b == 0:
                total += 2 * ho * ho * cout * cin
            cin, hw = cout, ho
    assert W.forward_flops(arch) == total + 2 * 2048 * 1000
    if arch == "resnet50":
        assert total + 2 * 2048 * 1000 == 8_178_368_512


def test_generated_grouped_weight_uses_the_groups_fan_in():
    w = W.generate_tensor("layer1.0.conv2.weight", (128, 4, 3, 3), seed=0)
    bound = np.sqrt(6.0 / 36.0)
    assert np.abs(w).max() <= bound and np.abs(w).max() > 0.95 * bound


def test_packed_weight_numel():
    lib = L.lib()
    f = lib.rn_conv2d_grouped_packed_weight_numel_dt
    for C, G in ((128, 32), (256, 32), (256, 64), (512, 32), (1024, 32)):     # Cg <= 32: one 32-channel K slice
        assert f(L.RN_DTYPE_F32, C, C, 3, G) == C * 9 * 32
    assert f(L.RN_DTYPE_F32, 2048, 2048, 3, 32) == 2048 * 9 * 64             # Cg = 64: no zeros
    assert f(L.RN_DTYPE_F32, 24, 36, 3, 12) == 36 * 2 * 9                    # direct kernel: the OIHW weight
    assert f(L.RN_DTYPE_F32, 128, 128, 5, 32) == 128 * 4 * 25
    assert f(L.RN_DTYPE_BF16, 128, 128, 3, 32) == lib.rn_conv2d_packed_weight_numel_dt(L.RN_DTYPE_BF16, 128, 128, 3)
    assert f(L.RN_DTYPE_F32, 100, 128, 3, 32) == 0                           # groups does not divide


def test_new_symbols_are_exported():
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("rn_conv2d_grouped_forward", "rn_conv2d_grouped_packed_weight_numel_dt",
                 "rn_conv2d_grouped_pack_weight_dt", "rn_conv2d_grouped_nhwc_forward_dt", "rn_model_create_ex",
                 "rn_shard_create_ex"):
        assert getattr(lib, name) is not None
        assert name in L.SIGNATURES


def bottleneck_features_f64(arch, state, x):
    """float64 pooled features of any network of the bottleneck family: torch's grouped convolution for conv2"""
    t = lambda k: torch.from_numpy(np.asarray(state[k], dtype=np.float64))
    bn = lambda name, y: F.batch_norm(y, t(f"{name}.running_mean"), t(f"{name}.running_var"), t(f"{name}.weight"),
                                      t(f"{name}.bias"), False, 0.0, 1e-5)
    groups = W.family_of(arch)[1]
    with torch.no_grad():
        h = torch.from_numpy(np.asarray(x, dtype=np.float64))
        h = F.max_pool2d(F.relu(bn("bn1", F.conv2d(h, t("conv1.weight"), stride=2, padding=3))), 3, 2, 1)
        for pre, _cin, _mid, _cout, stride, has_ds in W.iter_blocks(arch):
            y = F.relu(bn(f"{pre}.bn1", F.conv2d(h, t(f"{pre}.conv1.weight"))))
            y = F.relu(bn(f"{pre}.bn2", F.conv2d(y, t(f"{pre}.conv2.weight"), stride=stride, padding=1, groups=groups)))
            y = bn(f"{pre}.bn3", F.conv2d(y, t(f"{pre}.conv3.weight")))
            sc = bn(f"{pre}.downsample.1", F.conv2d(h, t(f"{pre}.downsample.0.weight"), stride=stride)) if has_ds else h
            h = F.relu(y + sc)
        return h.mean(dim=(2, 3)).numpy()


def test_groups_aware_f64_forward_is_netrefs_on_resnet50(finch, state50):
    x = np.concatenate([finch, R.weights.generate_input(1, seed=3)])
    a, b = bottleneck_features_f64("resnet50", state50, x), N.features_f64("resnet50", state50, x)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
