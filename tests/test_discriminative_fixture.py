"""The fixture that the bottleneck networks' top-1 tests stand on (oracle/netref.py), proven on the host in
float64: with the fc re-centred on 16 structured images the top-1 follows the image, the top-2 gaps leave
room for the fp32 tolerance, and a convolution bug in the middle of the network moves the logits by more
than that tolerance.  The generated state alone gives every one of these inputs class 112."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_c_amd as R
from oracle import netref as N
from oracle import torch_port as TP

TOL = 1e-4           # the fp32 whole-network tolerance of the GPU tests
ARCHS = ["resnet50", "resnet101", "resnet152"]


@pytest.fixture(scope="module")
def x16(finch):
    return N.structured_inputs(finch)


@pytest.fixture(scope="module")
def rn50(x16):
    """ResNet-50: the generated state, its fp64 features of the 16 images, the re-centred state and logits"""
    state = R.weights.generate_state("resnet50", seed=0)
    feats = N.features_f64("resnet50", state, x16)
    st, logits = N.recentre_fc(state, feats)
    return state, feats, st, logits


def test_structured_inputs_are_the_fixed_set_and_extend_it(finch, x16):
    """n = 16 is the fixed set (8 finch variants, 8 fields of seeds 500-507); a larger n keeps its finch
    variants and fields as prefixes; the images are not duplicates of each other"""
    assert x16.shape == (16, 3, 224, 224) and x16.dtype == np.float32
    assert np.array_equal(x16[0], finch[0]) and np.array_equal(x16[1], finch[0][:, :, ::-1])
    assert np.array_equal(x16[8:], N.low_freq_fields(8, 500))
    x64 = N.structured_inputs(finch, 64)
    assert np.array_equal(x64[:8], x16[:8]) and np.array_equal(x64[32:40], x16[8:])
    flat = x64.reshape(64, -1)
    assert len({r.tobytes() for r in flat}) == 64
    assert not np.array_equal(N.low_freq_fields(4, 10_000), N.low_freq_fields(4, 500))


@pytest.mark.parametrize("arch", ARCHS)
def test_generated_fc_gives_one_class_recentred_fc_follows_the_image(arch, x16):
    """The generated state puts the 16 images in (almost) one class; re-centred (W unscaled) they spread
    over at least 8 classes, at least 12 have a top-2 gap above 10 TOL, and the input-dependent logit spread
    is unchanged by the re-centring (it only moves the bias)."""
    state = R.weights.generate_state(arch, seed=0)
    feats = N.features_f64(arch, state, x16)
    plain = N.ref_logits(state, feats)
    assert len(set(plain.argmax(1).tolist())) <= 2
    st, logits = N.recentre_fc(state, feats)
    assert np.array_equal(st["fc.weight"], state["fc.weight"])
    assert abs(N.logit_spread(logits) - N.logit_spread(plain)) <= 1e-9
    top = logits.argmax(1)
    assert len(set(top.tolist())) >= 8, top
    assert (N.top2_gap(logits) > 10 * TOL).sum() >= 12


def test_held_out_fields_spread_over_many_classes(rn50):
    """96 fields not in the 16-image set, through ResNet-50 with the fc re-centred on the 16: the top-1
    follows these images too (at least 32 distinct classes)"""
    state, _, st, _ = rn50
    x = N.low_freq_fields(96, seed=10_000)
    logits = N.ref_logits(st, N.features_f64("resnet50", state, x))
    assert len(set(logits.argmax(1).tolist())) >= 32


def test_recentre_fc_spread():
    """spread = s: the input-dependent logits have std s; the argmax and the gap ratios do not change"""
    g = np.random.default_rng(3)
    feats = g.standard_normal((12, 64)) + 5.0
    state = {"fc.weight": g.standard_normal((20, 64)).astype(np.float32), "fc.bias": np.zeros(20, np.float32)}
    _, a = N.recentre_fc(state, feats)
    _, b = N.recentre_fc(state, feats, spread=1.0)
    assert abs(N.logit_spread(b) - 1.0) < 1e-6 and abs(a.mean(0)).max() < 1e-4
    assert np.array_equal(a.argmax(1), b.argmax(1))
    gap = N.top2_gap(a) / N.top2_gap(b)
    assert np.allclose(gap, gap[0], rtol=1e-5)


# ---------------------------------------------------------------------------
# sensitivity: what the GPU tests' 1e-4 bound catches
# ---------------------------------------------------------------------------
KEY = "layer3.1.conv2.weight"   # a 3x3, 256 -> 256 convolution at 14 x 14, in the middle of ResNet-50


def _perturb(w, kind):
    w = w.copy()
    if kind == "zero_k_slice":       # one 32-channel K block of the contraction lost
        w[:, 32:64] = 0
    elif kind == "swap_corner_taps":  # taps (0,0) and (2,2) of every 3x3 kernel exchanged: a wrong tap offset
        w[:, :, 0, 0], w[:, :, 2, 2] = w[:, :, 2, 2].copy(), w[:, :, 0, 0].copy()
    elif kind == "zero_centre_tap":   # one tap of every kernel lost
        w[:, :, 1, 1] = 0
    elif kind == "duplicated_row":    # output channel 5 computed with channel 6's weights: a row-index slip
        w[5] = w[6]
    elif kind == "zero_out_channel":  # one output channel's sum lost (only the bias remains)
        w[0] = 0
    elif kind == "bf16_panel":        # this one layer's fp32 panel rounded to bf16
        w = torch.from_numpy(w).to(torch.bfloat16).to(torch.float32).numpy()
    elif kind == "swap_taps_one_kernel":  # corner taps exchanged in a single 3x3 kernel
        w[7, 9, 0, 0], w[7, 9, 2, 2] = w[7, 9, 2, 2], w[7, 9, 0, 0]
    elif kind == "one_weight_ulp":        # one weight off by 2^-9 of itself (a bf16 rounding step)
        w[7, 9, 1, 1] *= 1 + 2.0 ** -9
    elif kind == "dead_input_channel":    # every tap of input channel 0, which the ReLU before keeps at 0
        w[:, 0] = 1.0
    return w


def _blocks():
    """(name, stride, has downsample) of ResNet-50's blocks in order"""
    return [(f"layer{li}.{bi}", stride if bi == 0 else 1, bi == 0)
            for li, (n, stride) in enumerate(zip(TP._DEPTHS["resnet50"], (1, 2, 2, 2)), start=1) for bi in range(n)]


SPLIT = [b[0] for b in _blocks()].index("layer3.1")


@torch.no_grad()
def _tail_logits(st, h, w_key):
    """layer3.1 (with conv2's weight replaced) to the logits, in float64, from layer3.1's input h"""
    t = TP.to_torch(st, torch.float64)
    t[KEY] = torch.from_numpy(np.asarray(w_key, np.float64))
    for pre, stride, ds in _blocks()[SPLIT:]:
        h = TP._block(t, pre, h, stride, ds)
    return N.ref_logits(st, h.mean(dim=(2, 3)).numpy())


@torch.no_grad()
def test_a_mid_network_convolution_bug_moves_the_logits_past_the_bound(rn50, x16):
    """ResNet-50, fc re-centred (W unscaled), float64: one layer (layer3.1.conv2) or its input corrupted in
    eleven ways.  Measured on the host, max |dlogit| over the 16 images:

      caught with 10x room (>= 10 TOL):  a zeroed 32-channel K slice (8e-2), the corner taps of every kernel
        exchanged (3e-2), every centre tap lost (7e-2), one output channel computed with its neighbour's
        weights (9e-3);
      caught by the 1e-4 bound, without that room:  one output channel's sum lost (5e-4), the layer's panel
        rounded to bf16 (3e-4), the corner taps of one single 3x3 kernel exchanged (3e-4);
      NOT caught (< TOL):  one element of the layer's input off by 1.0 (9e-5) or by 0.1 (9e-6), one weight off
        by 2^-9 of itself (4e-6), and any corruption confined to an input channel that the ReLU in front of the
        layer keeps at zero on these images (exactly 0).

    The asserts hold each perturbation to its class, so the list above stays true."""
    state, _, st, want = rn50
    t = TP.to_torch(state, torch.float64)
    h = torch.from_numpy(x16.astype(np.float64))
    h = F.relu(TP._bn(t, "bn1", F.conv2d(h, t["conv1.weight"], stride=2, padding=3)))
    h = F.max_pool2d(h, 3, 2, 1)
    for pre, stride, ds in _blocks()[:SPLIT]:
        h = TP._block(t, pre, h, stride, ds)
    w = st[KEY]
    assert np.abs(_tail_logits(st, h, w) - want).max() <= 1e-10     # the split forward is the whole one
    move = {}
    for kind in ("zero_k_slice", "swap_corner_taps", "zero_centre_tap", "duplicated_row", "zero_out_channel",
                 "bf16_panel", "swap_taps_one_kernel", "one_weight_ulp", "dead_input_channel"):
        move[kind] = float(np.abs(_tail_logits(st, h, _perturb(w, kind)) - want).max())
    for v in (1.0, 0.1):   # one element of the layer's input (image 3, channel 9, pixel (13, 13)) off by v
        hp = h.clone()
        hp[3, 9, 13, 13] += v
        move[f"input_element_{v}"] = float(np.abs(_tail_logits(st, hp, w) - want).max())
    print("\nmax |dlogit| per perturbation of " + KEY + ": " + ", ".join(f"{k} {v:.2e}" for k, v in move.items()))
    for kind in ("zero_k_slice", "swap_corner_taps", "zero_centre_tap", "duplicated_row"):
        assert move[kind] >= 10 * TOL, (kind, move[kind])
    for kind in ("zero_out_channel", "bf16_panel", "swap_taps_one_kernel"):
        assert TOL < move[kind] < 10 * TOL, (kind, move[kind])
    for kind in ("input_element_1.0", "input_element_0.1", "one_weight_ulp"):
        assert 0.0 < move[kind] < TOL, (kind, move[kind])
    assert move["dead_input_channel"] == 0.0
