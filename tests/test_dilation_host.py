"""Dilated convolution, the parts that need no GPU: the exported symbols, the output size, and the two
yardsticks of tests/test_dilation_gpu.py held to each other.

  A  torch on the CPU: F.conv2d(..., dilation=d, groups=g) in float64 (`conv64`);
  B  the committed oracle with a zero-stuffed kernel (`stuffed_oracle`): the weight spread to (k - 1) * d + 1
     taps per side with zeros between, through oracle.conv2d (per group: grouped_oracle).  It has the reference's
     summation order, because the zero products add exact zeros.
"""
import re
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from resnet_c_amd import _lib as L
from test_grouped_host import grouped_oracle


def conv64(x, w, stride, pad, dilation, groups=1):
    """yardstick A"""
    y = F.conv2d(torch.from_numpy(np.asarray(x, dtype=np.float64)), torch.from_numpy(np.asarray(w, dtype=np.float64)),
                 None, stride, pad, dilation, groups)
    return y.numpy()


def stuff(w, d):
    """[Cout][Cg][k][k] -> [Cout][Cg][(k-1)d+1][(k-1)d+1], the taps d apart, zeros between"""
    Cout, Cg, k, _ = w.shape
    span = (k - 1) * d + 1
    out = np.zeros((Cout, Cg, span, span), dtype=np.float32)
    out[:, :, ::d, ::d] = w
    return out


def stuffed_oracle(x, w, stride, pad, dilation, groups=1):
    """yardstick B"""
    return grouped_oracle(np.asarray(x, dtype=np.float32), stuff(np.asarray(w, dtype=np.float32), dilation), stride, pad,
                          groups)


def test_new_symbols_are_exported():
    lib = L.lib()
    for name in ("rn_conv_output_size_dilated", "rn_conv2d_dilated_forward", "rn_conv2d_dilated_nhwc_forward_dt"):
        assert getattr(lib, name) is not None, name
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rn_hip.h")).read()
    bound = int(re.search(r"#define RN_CONV_MAX_DILATION (\d+)", header).group(1))
    assert bound == L.RN_CONV_MAX_DILATION and bound >= 64


def test_output_size_is_torchs():
    """over a grid of (x, k, s, p, d): torch's output shape, and 0 where the dilated kernel does not fit"""
    lib = L.lib()
    for x in (1, 2, 3, 5, 7, 9, 14, 28):
        for k in (1, 2, 3, 5, 7):
            for s in (1, 2, 3):
                for p in (0, 1, 2, 4, 6):
                    for d in (1, 2, 3, 4, 8, 64):
                        got = int(lib.rn_conv_output_size_dilated(x, k, s, p, d))
                        if x + 2 * p < d * (k - 1) + 1:
                            assert got == 0, (x, k, s, p, d, got)
                            with pytest.raises(RuntimeError):
                                F.conv2d(torch.zeros(1, 1, x, x), torch.zeros(1, 1, k, k), None, s, p, d)
                            continue
                        want = F.conv2d(torch.zeros(1, 1, x, 64 * 8), torch.zeros(1, 1, k, 1), None, s, (p, 0), (d, 1)).shape[2]
                        assert got == want, (x, k, s, p, d, got, want)
                        if d == 1:
                            assert got == int(lib.rn_conv_output_size(x, k, s, p))
    assert lib.rn_conv_output_size_dilated(8, 3, 1, 1, 0) == 0
    assert lib.rn_conv_output_size_dilated(8, 3, 0, 1, 1) == 0
    assert lib.rn_conv_output_size_dilated(8, 0, 1, 1, 1) == 0


# (B, Cin, Cout, G, H, W, k, s, p, d): d * (k - 1) >= H, pad != d, stride 2, no padding, k = 5, groups
YARDSTICK_CASES = [(2, 8, 6, 1, 7, 5, 3, 1, 2, 2), (1, 4, 4, 1, 3, 9, 3, 1, 4, 4), (2, 6, 4, 1, 9, 8, 3, 2, 2, 2),
                   (1, 5, 3, 1, 11, 10, 3, 1, 0, 2), (2, 4, 4, 1, 6, 7, 3, 1, 3, 5), (1, 3, 2, 1, 13, 13, 5, 1, 4, 2),
                   (2, 12, 8, 4, 6, 7, 3, 2, 2, 2)]


@pytest.mark.parametrize("case", YARDSTICK_CASES)
def test_stuffed_oracle_is_torchs_dilated_convolution(case):
    B, Cin, Cout, G, H, W, k, s, p, d = case
    g = np.random.default_rng(sum(case))
    x = g.standard_normal((B, Cin, H, W), dtype=np.float32)
    w = g.standard_normal((Cout, Cin // G, k, k), dtype=np.float32)
    a, b = conv64(x, w, s, p, d, G), stuffed_oracle(x, w, s, p, d, G)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= 1e-5 * max(1.0, float(np.abs(a).max()))


def test_stuffing_with_dilation_one_is_the_oracle():
    g = np.random.default_rng(3)
    x, w = g.standard_normal((1, 4, 5, 6), dtype=np.float32), g.standard_normal((3, 4, 3, 3), dtype=np.float32)
    assert np.array_equal(stuff(w, 1), w)
    assert np.array_equal(stuffed_oracle(x, w, 1, 1, 1), grouped_oracle(x, w, 1, 1, 1))


# ---- replace_stride_with_dilation: the block table, the FLOPs, the float64 forward -----------------------------
from oracle import netref as N                      # noqa: E402
from resnet_c_amd import weights as W               # noqa: E402

FLAGS = [(0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)]


def test_model_symbols_are_exported():
    lib = L.lib()
    for name in ("rn_model_set_dilation", "rn_model_dilation", "rn_model_output_stride"):
        assert getattr(lib, name) is not None and name in L.SIGNATURES, name


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("arch", ["resnet50", "resnext50_32x4d"])
def test_block_table_is_torchvisions_make_layer(arch, flags):
    """the rule of the issue, restated by hand: stride, dilation, padding and the presence of a downsample"""
    widths, depths = W.stage_widths(arch), W.depths_of(arch)
    want, dilation = [], 1
    for li in range(4):
        stride = 1 if li == 0 else 2
        previous = dilation
        if li > 0 and flags[li - 1]:
            dilation *= 2
            stride = 1
        cin, mid, cout = widths[li]
        for bi in range(depths[li]):
            want.append((f"layer{li + 1}.{bi}", cin if bi == 0 else cout, mid, cout, stride if bi == 0 else 1, bi == 0,
                         previous if bi == 0 else dilation))
    got = list(W.iter_blocks_dilated(arch, flags))
    assert got == want
    assert list(W.iter_blocks(arch, flags)) == [b[:6] for b in want]
    if not any(flags):
        assert list(W.iter_blocks(arch)) == [b[:6] for b in want] and all(b[6] == 1 for b in got)
        assert W.conv_specs(arch, flags) == W.conv_specs(arch)
    specs = {name: (cin, cout, k, s, p) for name, cin, cout, k, s, p in W.conv_specs(arch, flags)}
    for pre, cin, mid, cout, stride, has_ds, d in want:
        assert specs[f"{pre}.conv2"] == (mid, mid, 3, stride, d)        # padding == dilation
        assert specs[f"{pre}.conv1"] == (cin, mid, 1, 1, 0) and specs[f"{pre}.conv3"] == (mid, cout, 1, 1, 0)
        assert (f"{pre}.downsample.0" in specs) == has_ds
        if has_ds:
            assert specs[f"{pre}.downsample.0"] == (cin, cout, 1, stride, 0)
    assert max(b[6] for b in got) == 2 ** sum(flags)
    if arch == "resnet50" and flags == (0, 1, 1):
        d = {b[0]: b[6] for b in got}
        assert d["layer3.0"] == 1 and all(d[f"layer3.{i}"] == 2 for i in range(1, 6))
        assert d["layer4.0"] == 2 and d["layer4.1"] == d["layer4.2"] == 4


def test_basic_block_networks_refuse_the_flags():
    with pytest.raises(NotImplementedError):
        list(W.iter_blocks_dilated("resnet18", (0, 0, 1)))
    with pytest.raises(NotImplementedError):
        W.forward_flops("resnet34", 224, (1, 0, 0))
    assert W.forward_flops("resnet18", 224, (0, 0, 0)) == W.forward_flops("resnet18")


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("arch", ["resnet50", "resnext50_32x4d"])
def test_forward_flops_hand_formula(arch, flags):
    _, groups, wpg = W.family_of(arch)
    for H, Wd in ((224, 224), (96, 64)):
        sh, sw = (H + 6 - 7) // 2 + 1, (Wd + 6 - 7) // 2 + 1
        total = 2 * sh * sw * 64 * 147
        h, w = (sh + 2 - 3) // 2 + 1, (sw + 2 - 3) // 2 + 1
        cin = 64
        for li, (planes, blocks) in enumerate(zip((64, 128, 256, 512), W.depths_of(arch))):
            stride = 1 if li == 0 or flags[li - 1] else 2
            width, cout = planes * wpg // 64 * groups, 4 * planes
            for b in range(blocks):
                s = stride if b == 0 else 1
                ho, wo = (h - 1) // s + 1, (w - 1) // s + 1             # padding == dilation keeps (n - 1) / s + 1
                total += 2 * h * w * width * cin
                total += 2 * ho * wo * width * (width // groups) * 9
                total += 2 * ho * wo * cout * width
                if b == 0:
                    total += 2 * ho * wo * cout * cin
                cin, h, w = cout, ho, wo
        assert W.forward_flops(arch, (H, Wd), replace_stride_with_dilation=flags) == total + 2 * 2048 * 1000
    if not any(flags):
        assert W.forward_flops(arch, 224, flags) == W.forward_flops(arch)


def dilated_features_f64(arch, state, x, flags=(0, 0, 0)):
    """float64 pooled features of a bottleneck network under replace_stride_with_dilation, on the pattern of
    bottleneck_features_f64 (tests/test_grouped_host.py): torch's convolution with dilation and groups"""
    t = lambda k: torch.from_numpy(np.asarray(state[k], dtype=np.float64))
    bn = lambda name, y: F.batch_norm(y, t(f"{name}.running_mean"), t(f"{name}.running_var"), t(f"{name}.weight"),
                                      t(f"{name}.bias"), False, 0.0, 1e-5)
    groups = W.family_of(arch)[1]
    with torch.no_grad():
        h = torch.from_numpy(np.asarray(x, dtype=np.float64))
        h = F.max_pool2d(F.relu(bn("bn1", F.conv2d(h, t("conv1.weight"), stride=2, padding=3))), 3, 2, 1)
        for pre, _cin, _mid, _cout, stride, has_ds, d in W.iter_blocks_dilated(arch, flags):
            y = F.relu(bn(f"{pre}.bn1", F.conv2d(h, t(f"{pre}.conv1.weight"))))
            y = F.relu(bn(f"{pre}.bn2", F.conv2d(y, t(f"{pre}.conv2.weight"), stride=stride, padding=d, dilation=d,
                                                 groups=groups)))
            y = bn(f"{pre}.bn3", F.conv2d(y, t(f"{pre}.conv3.weight")))
            sc = bn(f"{pre}.downsample.1", F.conv2d(h, t(f"{pre}.downsample.0.weight"), stride=stride)) if has_ds else h
            h = F.relu(y + sc)
        return h.mean(dim=(2, 3)).numpy()


def test_dilated_f64_forward_is_netrefs_undilated(finch, state50):
    x = np.concatenate([finch, W.generate_input(1, seed=3)])
    a, b = dilated_features_f64("resnet50", state50, x), N.features_f64("resnet50", state50, x)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    # and the flags do change the function: the final map is 28 x 28 instead of 7 x 7
    c = dilated_features_f64("resnet50", state50, x[:1, :, :64, :64], (0, 1, 1))
    assert c.shape == (1, 2048) and np.isfinite(c).all()
