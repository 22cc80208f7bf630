"""Feature pyramid neck on the host: the index contract, torchvision's keys and arithmetic, and the references the GPU
tests hold the device to.

torchvision is not installed where the suite runs, so its FeaturePyramidNetwork.forward is restated here from
torch.nn.functional exactly as its source runs it (lateral 1x1, F.interpolate(mode="nearest", size=...) added top-down,
3x3 with padding 1, LastLevelMaxPool = max_pool2d(kernel 1, stride 2)).  The necks, map sizes and seeds are the ones
tests/test_fpn_gpu.py runs; it imports them.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from resnet_c_amd import _lib as L
from resnet_c_amd import fpn as P
from resnet_c_amd import ops
from resnet_c_amd import weights as W
from test_dilation_gpu import tol_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (in_channels_list, out_channels, extra): the two necks of the neck-alone GPU tests
NECKS = {"four": ((64, 128, 256, 512), 64, "pool"), "two": ((256, 512), 128, None)}
SIZES = ((18, 10), (9, 5), (5, 3), (3, 2))   # the stage maps of a 72 x 40 image: every ratio but one is odd
NECK_SEED, NECK_B = 0, 2

# (h, w) -> (H, W) of the kernel tests: one pixel, one pixel enlarged, exact 2x, odd ratios both ways, equal, shrinking
GEOMETRIES = (((1, 1), (1, 1)), ((1, 1), (5, 3)), ((2, 3), (4, 6)), ((3, 2), (5, 3)), ((7, 5), (13, 9)), ((4, 4), (4, 4)),
              ((5, 5), (2, 3)))


@functools.lru_cache(maxsize=None)
def neck_state(name):
    cin, a, _ = NECKS[name]
    return P.generate_fpn_state(cin, a, seed=NECK_SEED)


@functools.lru_cache(maxsize=None)
def neck_maps(name, B=NECK_B):
    """Seeded NCHW fp32 maps of the neck's levels, O(1) values like a stage's output, the finest first."""
    cin, _, _ = NECKS[name]
    sizes = SIZES[len(SIZES) - len(cin):]
    out = []
    for i, (c, (h, w)) in enumerate(zip(cin, sizes)):
        m = W._uniform(f"fpn_map.{name}.{i}", (B, c, h, w), -1.0, 1.0, NECK_SEED)
        m.setflags(write=False)
        out.append(m)
    return tuple(out)


def products(cin, a, level):
    """K of tol_f32 for an output of `level`: the 3x3's 9 * a products and, through the top-down sums, the lateral
    products of this level and of every coarser one."""
    return 9 * a + sum(cin[level:])


def torch_neck(maps, state, extra, dtype):
    """torchvision's FeaturePyramidNetwork.forward (norm_layer=None) in `dtype`."""
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)  # noqa: E731  (a copy: the fixtures are read-only)
    n = len(maps)
    conv = lambda x, kind, i, **kw: F.conv2d(x, t(state[f"{kind}.{i}.0.weight"]), t(state[f"{kind}.{i}.0.bias"]), **kw)  # noqa: E731
    with torch.no_grad():
        last = conv(t(maps[n - 1]), "inner_blocks", n - 1)
        results = [conv(last, "layer_blocks", n - 1, padding=1)]
        for i in range(n - 2, -1, -1):
            lateral = conv(t(maps[i]), "inner_blocks", i)
            last = lateral + F.interpolate(last, size=lateral.shape[-2:], mode="nearest")
            results.insert(0, conv(last, "layer_blocks", i, padding=1))
        out = {str(i): r.numpy() for i, r in enumerate(results)}
        if extra == "pool":
            out["pool"] = F.max_pool2d(results[-1], kernel_size=1, stride=2, padding=0).numpy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
def test_nearest_index_is_torchs():
    """ops.nearest_index (the contract of rn_upsample_nearest_add_forward_dt) against F.interpolate(mode="nearest") on a
    grid of size pairs: a ramp upsampled along one axis reads back the source index."""
    bad = 0
    for n_in in list(range(1, 24)) + [31, 32, 33, 50, 64, 69]:
        src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in, 1)
        for n_out in list(range(1, 48)) + [63, 64, 65, 100, 127, 128, 139]:
            got = ops.nearest_index(n_in, n_out)
            want = F.interpolate(src, size=(n_out, 1), mode="nearest").reshape(-1).numpy().astype(np.int64)
            bad += int((got != want).sum())
    assert bad == 0


@pytest.mark.parametrize("geom", GEOMETRIES + (((7, 5), (25, 50)), ((13, 25), (25, 50))))
def test_upsample_nearest_add_ref_is_torchs(geom):
    (h, w), (H, Wd) = geom
    rng = np.random.default_rng(h * 1000 + w * 100 + H * 10 + Wd)
    top = rng.standard_normal((2, h, w, 8)).astype(np.float32)
    lat = rng.standard_normal((2, H, Wd, 8)).astype(np.float32)
    up = F.interpolate(torch.from_numpy(top).permute(0, 3, 1, 2), size=(H, Wd), mode="nearest")
    # channels_last input takes torch's other kernel: the same indices
    up_cl = F.interpolate(torch.from_numpy(top).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last),
                          size=(H, Wd), mode="nearest")
    assert torch.equal(up, up_cl)
    want_up = up.permute(0, 2, 3, 1).numpy()
    assert np.array_equal(ops.upsample_nearest_add_ref(top, size=(H, Wd)).view(np.uint32), want_up.view(np.uint32))
    want = (torch.from_numpy(lat) + up.permute(0, 2, 3, 1)).numpy()
    assert np.array_equal(ops.upsample_nearest_add_ref(top, lat).view(np.uint32), want.view(np.uint32))


def test_upsample_nearest_add_ref_bf16_rounds_once():
    """widen, fp32 add, one rounding to the nearest even: 1 + 2^-8 is a tie between 1 and 1 + 2^-7 and goes to the even
    1; 1 + 2^-7 + 2^-8 is a tie that goes up to the even 1 + 2^-6."""
    one, ulp, half = np.float32(1.0), np.float32(2.0 ** -7), np.float32(2.0 ** -8)
    lat = ops.to_bf16_bits(np.array([one, one + ulp, one, -one], dtype=np.float32)).reshape(1, 1, 1, 4)
    top = ops.to_bf16_bits(np.array([half, half, ulp, -half], dtype=np.float32)).reshape(1, 1, 1, 4)
    got = ops.from_bf16_bits(ops.upsample_nearest_add_ref(top, lat)).reshape(-1)
    assert got.tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0]


def test_fpn_shapes():
    s = P.fpn_shapes((64, 128, 256, 512), 64)
    assert list(s)[:2] == ["inner_blocks.0.0.weight", "inner_blocks.0.0.bias"]
    assert list(s)[8:10] == ["layer_blocks.0.0.weight", "layer_blocks.0.0.bias"] and len(s) == 16
    assert s["inner_blocks.3.0.weight"] == (64, 512, 1, 1) and s["inner_blocks.3.0.bias"] == (64,)
    assert s["layer_blocks.2.0.weight"] == (64, 64, 3, 3) and s["layer_blocks.2.0.bias"] == (64,)
    state = P.generate_fpn_state((256, 512), 128, seed=3)
    assert {k: v.shape for k, v in state.items()} == P.fpn_shapes((256, 512), 128)
    assert all(v.dtype == np.float32 for v in state.values())
    again = P.generate_fpn_state((256, 512), 128, seed=3)
    assert all(np.array_equal(state[k], again[k]) for k in state)
    assert not np.array_equal(state["inner_blocks.0.0.weight"], P.generate_fpn_state((256, 512), 128, seed=4)["inner_blocks.0.0.weight"])


def test_split_state_takes_both_spellings():
    state = neck_state("two")
    new = {"backbone.fpn." + k: torch.from_numpy(v) for k, v in state.items()}
    old = {"fpn." + k.replace(".0.weight", ".weight").replace(".0.bias", ".bias"): v for k, v in state.items()}
    assert "fpn.inner_blocks.1.weight" in old and "fpn.layer_blocks.0.bias" in old
    new["backbone.body.conv1.weight"] = torch.zeros(64, 3, 7, 7)
    new["backbone.body.bn1.num_batches_tracked"] = torch.zeros(())
    new["rpn.head.conv.0.0.weight"] = torch.zeros(4)
    for given in (new, old, state):
        body, neck = P.split_state(given)
        assert list(neck) != [] and set(neck) == set(state)
        assert all(np.array_equal(neck[k], state[k]) for k in state)
    body, _ = P.split_state(new)
    assert list(body) == ["conv1.weight"]
    with pytest.raises(ValueError):
        P.split_state({"fpn.inner_blocks.0.0.gamma": np.zeros(4, dtype=np.float32)})


@pytest.mark.parametrize("name", sorted(NECKS))
def test_fpn_ref_is_torchvisions_arithmetic(name):
    cin, a, extra = NECKS[name]
    maps = [m.astype(np.float64) for m in neck_maps(name)]
    got = P.fpn_ref(maps, neck_state(name), extra)
    want = torch_neck(maps, neck_state(name), extra, torch.float64)
    assert list(got) == list(want) == [str(i) for i in range(len(cin))] + (["pool"] if extra else [])
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float64
        assert float(np.abs(got[k] - want[k]).max()) <= 1e-12 * float(np.abs(want[k]).max()), k
    if extra:
        last = str(len(cin) - 1)
        assert np.array_equal(got["pool"], got[last][:, :, ::2, ::2])


@pytest.mark.parametrize("name", sorted(NECKS))
def test_fp32_bound_is_reachable(name):
    """The GPU tests hold an fp32 neck to tol_f32(ref, K) with K = products(...): torch's own fp32 execution of the
    same neck stays inside that bound, so it asks nothing an fp32 implementation cannot give."""
    cin, a, extra = NECKS[name]
    ref = P.fpn_ref([m.astype(np.float64) for m in neck_maps(name)], neck_state(name), extra)
    got = torch_neck(neck_maps(name), neck_state(name), extra, torch.float32)
    for i in range(len(cin)):
        err, tol = float(np.abs(got[str(i)] - ref[str(i)]).max()), tol_f32(ref[str(i)], products(cin, a, i))
        print(f"\n  fpn {name}: torch fp32, level {i}: max error {err:.3e}, bound {tol:.3e}")
        assert err <= tol


def test_fpn_ref_round_fn_rounds_what_is_stored():
    cin, a, extra = NECKS["two"]
    maps = [m.astype(np.float64) for m in neck_maps("two")]
    plain = P.fpn_ref(maps, neck_state("two"), extra)
    rounded = P.fpn_ref(maps, neck_state("two"), extra, round_fn=ops.bf16_round)
    for k in plain:
        d = float(np.abs(plain[k] - rounded[k]).max())
        assert 0.0 < d <= 2.0 ** -5 * float(np.abs(plain[k]).max()), (k, d)


def test_surface():
    text = open(os.path.join(ROOT, "include", "rn_hip.h")).read()
    declared = set(re.findall(r"RN_API[^;(]*?\b(rn_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rn_[a-z0-9_]+)", out))
    lib = L.lib()
    for name in ("rn_upsample_nearest_add_forward_dt", "rn_fpn_create", "rn_fpn_set_dtype", "rn_fpn_set_tensor",
                 "rn_fpn_finalize", "rn_fpn_destroy", "rn_fpn_level_shape", "rn_fpn_forward", "rn_model_forward_fpn",
                 "rn_model_forward_fpn_u8"):
        assert name in declared and name in exported and name in L.SIGNATURES and hasattr(lib, name), name
    assert ctypes.sizeof(L.FpnOutputs) == 5 * 8
