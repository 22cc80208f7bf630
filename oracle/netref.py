"""Whole-network fp64 references and a discriminative test fixture (CPU).

TEST INFRASTRUCTURE ONLY -- imported by tests, never by the product package.

The generated weights (resnet_c_amd.weights.generate_state) give almost every input the same
class: the fc bias and the input-independent part of the pooled features outweigh the part that
depends on the image.  A top-1 check on them cannot fail on a convolution bug.  This module
builds the fixture that can:

* ``structured_inputs``: images with content (the finch, its flips and reflect-padded crops,
  seeded low-frequency colour fields);
* ``features_f64``: the pooled features [B, C] of any of the five networks in float64
  (bottleneck blocks through ``torch_port``'s ``_bn`` / ``_block``, which are pinned to the
  reference module's goldens; basic blocks with torchvision's BasicBlock semantics);
* ``recentre_fc``: the fc bias replaced by ``-W . mean(f)``, so that the logits are the
  input-dependent part alone and the top-1 follows the image;
* ``features_bf16_emulated``: the same forward with the roundings of the model driver's bf16
  storage (rn_model.c) applied where the driver applies them.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_port as TP

_DEPTHS = TP._DEPTHS
FIELD_SEED = 500   # seed of the first low-frequency field of the 16-image set


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def low_freq_fields(n: int, seed: int = FIELD_SEED) -> np.ndarray:
    """n seeded low-frequency colour fields [n,3,224,224] fp32: field s is the sum of six products of
    cosines of frequencies 0-3 (half periods per image side) with random phases and a random colour,
    drawn from default_rng(seed + s)."""
    yy, xx = np.meshgrid(np.linspace(0, 1, 224), np.linspace(0, 1, 224), indexing="ij")
    out = np.empty((n, 3, 224, 224), np.float32)
    for s in range(n):
        g = np.random.default_rng(seed + s)
        img = np.zeros((3, 224, 224))
        for _ in range(6):
            fy, fx = g.integers(0, 4, 2)
            ph = g.random(2) * 2 * np.pi
            img += g.standard_normal((3, 1, 1)) * np.cos(np.pi * fy * yy + ph[0]) * np.cos(np.pi * fx * xx + ph[1])
        out[s] = img
    return out


def finch_variants(finch: np.ndarray, n: int, seed: int = FIELD_SEED) -> np.ndarray:
    """n images from the finch [1,3,224,224]: the finch, its mirror and six fixed crops of the 24-pixel
    reflect-padded image first; beyond eight, a random horizontal / vertical flip of a crop at a random
    offset, drawn from default_rng(seed)."""
    f = finch[0]
    pad = np.pad(f, ((0, 0), (24, 24), (24, 24)), mode="reflect")
    imgs = [f, f[:, :, ::-1]]
    for dy, dx in ((24, 0), (48, 48), (0, 48), (48, 0), (12, 36), (40, 8)):
        imgs.append(pad[:, dy:dy + 224, dx:dx + 224])
    imgs = imgs[:n]
    g = np.random.default_rng(seed)
    while len(imgs) < n:
        dy, dx = g.integers(0, 49, 2)
        c = pad[:, dy:dy + 224, dx:dx + 224]
        flip = g.integers(0, 4)
        if flip & 1:
            c = c[:, :, ::-1]
        if flip & 2:
            c = c[:, ::-1, :]
        imgs.append(c)
    return np.ascontiguousarray(np.stack(imgs), dtype=np.float32)


def structured_inputs(finch: np.ndarray, n: int = 16, seed: int = FIELD_SEED) -> np.ndarray:
    """n images with content [n,3,224,224] fp32: n // 2 finch variants then n - n // 2 low-frequency
    fields.  n = 16 at the default seed: the finch, its mirror, six shifted crops, eight fields -- the
    fixed set the fc is re-centred on."""
    k = n // 2
    return np.ascontiguousarray(np.concatenate([finch_variants(finch, k, seed), low_freq_fields(n - k, seed)]))


# ---------------------------------------------------------------------------
# fp64 networks
# ---------------------------------------------------------------------------
def _t(state, key):
    return torch.from_numpy(np.asarray(state[key], dtype=np.float64))


def _bn64(state, name, x):
    return F.batch_norm(x, _t(state, f"{name}.running_mean"), _t(state, f"{name}.running_var"),
                        _t(state, f"{name}.weight"), _t(state, f"{name}.bias"), False, 0.0, 1e-5)


def _basic_features(arch, state, x):
    from resnet_c_amd import weights as W

    h = torch.from_numpy(np.asarray(x, dtype=np.float64))
    h = F.relu(_bn64(state, "bn1", F.conv2d(h, _t(state, "conv1.weight"), stride=2, padding=3)))
    h = F.max_pool2d(h, 3, 2, 1)
    for pre, _cin, _cout, stride, has_ds in W.iter_basic_blocks(arch):
        t = F.relu(_bn64(state, f"{pre}.bn1", F.conv2d(h, _t(state, f"{pre}.conv1.weight"), stride=stride, padding=1)))
        t = _bn64(state, f"{pre}.bn2", F.conv2d(t, _t(state, f"{pre}.conv2.weight"), stride=1, padding=1))
        sc = h
        if has_ds:
            sc = _bn64(state, f"{pre}.downsample.1", F.conv2d(h, _t(state, f"{pre}.downsample.0.weight"), stride=stride))
        h = F.relu(t + sc)
    return h.mean(dim=(2, 3)).numpy()


def _bottleneck_features(arch, state, x):
    t = TP.to_torch({k: v for k, v in state.items() if not k.startswith("fc.")}, torch.float64)
    y = torch.from_numpy(np.asarray(x, dtype=np.float64))
    y = F.relu(TP._bn(t, "bn1", F.conv2d(y, t["conv1.weight"], stride=2, padding=3)))
    y = F.max_pool2d(y, kernel_size=3, stride=2, padding=1)
    for li, (n, stride) in enumerate(zip(_DEPTHS[arch], (1, 2, 2, 2)), start=1):
        for bi in range(n):
            y = TP._block(t, f"layer{li}.{bi}", y, stride if bi == 0 else 1, bi == 0)
    return y.mean(dim=(2, 3)).numpy()


@torch.no_grad()
def features_f64(arch: str, state: Dict[str, np.ndarray], x: np.ndarray) -> np.ndarray:
    """float64 pooled features [B, 2048] (bottleneck) or [B, 512] (basic block) of NCHW images x."""
    if arch in _DEPTHS:
        return _bottleneck_features(arch, state, x)
    return _basic_features(arch, state, x)


def ref_logits(state: Dict[str, np.ndarray], feats: np.ndarray) -> np.ndarray:
    """float64 fc of float64 features, with the state's (fp32) fc weight and bias."""
    return feats @ np.asarray(state["fc.weight"], np.float64).T + np.asarray(state["fc.bias"], np.float64)


def recentre_fc(state: Dict[str, np.ndarray], feats: np.ndarray, spread: Optional[float] = None):
    """The state with its fc re-centred on the features feats [N, C] (bias = -W . mean(feats), in float64
    from the fp32-rounded W), and the float64 logits of feats under it.  spread: W is first divided by the
    std of the input-dependent logits (feats - mean) W^T and multiplied by spread; None keeps W as it is
    (argmax and gap ratios do not depend on that scale, absolute tolerances keep their meaning)."""
    w = np.asarray(state["fc.weight"], np.float64)
    if spread is not None:
        d = (feats - feats.mean(0)) @ w.T
        w = w / (d.std() / spread)
    st = dict(state)
    st["fc.weight"] = w.astype(np.float32)
    st["fc.bias"] = (-(w.astype(np.float32).astype(np.float64) @ feats.mean(0))).astype(np.float32)
    return st, ref_logits(st, feats)


def top2_gap(logits: np.ndarray) -> np.ndarray:
    """per row: largest minus second largest logit"""
    s = np.sort(logits, axis=1)
    return s[:, -1] - s[:, -2]


def logit_spread(logits: np.ndarray) -> float:
    """std of the input-dependent part of the logits (each class's mean over the images removed)"""
    return float((logits - logits.mean(0)).std())


# ---------------------------------------------------------------------------
# bf16 storage of the model driver, emulated (bottleneck networks, fused mode)
# ---------------------------------------------------------------------------
def _rb(a):
    """round to fp32, then to the nearest bf16 (round to nearest even), back to float64"""
    return a.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _fold(state, bn):
    """eval-mode batch-norm as scale and shift, the way the driver folds it"""
    sc = _t(state, f"{bn}.weight") / torch.sqrt(_t(state, f"{bn}.running_var") + 1e-5)
    return sc, _t(state, f"{bn}.bias") - _t(state, f"{bn}.running_mean") * sc


def _affine(y, sc, sh):
    return y * sc[None, :, None, None] + sh[None, :, None, None]


@torch.no_grad()
def features_bf16_emulated(arch: str, state: Dict[str, np.ndarray], x: np.ndarray) -> np.ndarray:
    """float64 pooled features [B, 2048] with the roundings of the model driver's bf16 storage (rn_model.c,
    fused mode, pair fusion and chains on): the image is stored as bf16; every weight panel is bf16 (RNE);
    the batch-norm scale and shift are fp32 epilogue constants, except in the pair panel of a stage's first
    block (conv3 + downsample as one contraction), where both scales are multiplied into the weights before
    rounding and the two shifts are added; every stored activation is bf16 (after the epilogue: stem +
    ReLU + max-pool, each convolution, the average pool).  A chain launch rounds its intermediate tensor
    like the two launches it replaces, so it needs no case of its own.  Sums are float64 here (fp32 on the
    GPU)."""
    q = lambda k: _rb(_t(state, k))
    h = _rb(torch.from_numpy(np.asarray(x, dtype=np.float64)))
    sc, sh = _fold(state, "bn1")
    h = F.relu(_affine(F.conv2d(h, q("conv1.weight"), stride=2, padding=3), sc, sh))
    h = _rb(F.max_pool2d(h, 3, 2, 1))
    for li, (n, stride) in enumerate(zip(_DEPTHS[arch], (1, 2, 2, 2)), start=1):
        for bi in range(n):
            pre, s = f"layer{li}.{bi}", stride if bi == 0 else 1
            sc1, sh1 = _fold(state, f"{pre}.bn1")
            sc2, sh2 = _fold(state, f"{pre}.bn2")
            sc3, sh3 = _fold(state, f"{pre}.bn3")
            t = _rb(F.relu(_affine(F.conv2d(h, q(f"{pre}.conv1.weight")), sc1, sh1)))
            t = _rb(F.relu(_affine(F.conv2d(t, q(f"{pre}.conv2.weight"), stride=s, padding=1), sc2, sh2)))
            if bi == 0:
                scd, shd = _fold(state, f"{pre}.downsample.1")
                w3 = _rb(_t(state, f"{pre}.conv3.weight") * sc3[:, None, None, None])
                wd = _rb(_t(state, f"{pre}.downsample.0.weight") * scd[:, None, None, None])
                y = F.conv2d(t, w3) + F.conv2d(h, wd, stride=s) + (sh3 + shd)[None, :, None, None]
            else:
                y = _affine(F.conv2d(t, q(f"{pre}.conv3.weight")), sc3, sh3) + h
            h = _rb(F.relu(y))
    return _rb(h.mean(dim=(2, 3))).numpy()


def logits_bf16_emulated(state: Dict[str, np.ndarray], feats_bf16: np.ndarray) -> np.ndarray:
    """the bf16 model's fc: bf16 weights times the bf16 pooled features, fp32 bias, float64 here"""
    w = _rb(_t(state, "fc.weight")).numpy()
    return feats_bf16 @ w.T + np.asarray(state["fc.bias"], np.float64)
