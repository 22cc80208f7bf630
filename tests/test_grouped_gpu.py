"""Grouped convolution (rn_conv_group.hip) and the ResNeXt / Wide ResNet models on the GPU.

Yardsticks from outside the code under test: the per-group oracle (oracle.conv2d on each group's channel
slices, concatenated: the reference's summation order) for the op, a float64 forward with torch's grouped
convolution for the networks (tests/test_grouped_host.py holds both to torch / oracle.netref on the CPU).
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_c_amd as R
import views as V
from oracle import netref as N
from resnet_c_amd import _lib as L
from resnet_c_amd import ops
from resnet_c_amd import weights as W
from test_grouped_host import bottleneck_features_f64, grouped_oracle

pytestmark = pytest.mark.gpu

TOL = 1e-4  # fp32 whole-network bound, as test_model_gpu.py / test_top1_gpu.py


def rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def tol_of(ref, cg):
    return 2e-6 * np.sqrt(9 * cg) * float(np.abs(ref).max()) + 1e-6


# (C, G): every Cg the networks use -- 4, 8, 4, 16, 32, 64
SHAPES = [(128, 32), (256, 32), (256, 64), (512, 32), (1024, 32), (2048, 32)]
# B, H, W: odd planes, B = 1, and a ragged last M tile (256 output pixels per tile)
PLANES = [(1, 7, 61), (3, 1, 9), (2, 13, 11)]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cg", SHAPES)
def test_grouped_conv_matches_per_group_oracle(cg, stride, layout):
    C, G = cg
    for B, H, Wd in PLANES if C <= 512 else PLANES[:2]:
        x, w = rnd((B, C, H, Wd), C + G + H), rnd((C, C // G, 3, 3), C + G + H + 1)
        want = grouped_oracle(x, w, stride, 1, G)
        got = ops.conv2d_grouped(x, w, stride, 1, G, layout)
        assert got.shape == want.shape
        err = float(np.abs(got - want).max())
        assert err <= tol_of(want, C // G), (cg, stride, layout, (B, H, Wd), err, tol_of(want, C // G))


def test_grouped_conv_many_tiles():
    """more M tiles than one, several super-groups, B that leaves a ragged last tile: 3 * 20 * 20 = 1200 pixels"""
    x, w = rnd((3, 128, 20, 20), 5), rnd((128, 4, 3, 3), 6)
    want = grouped_oracle(x, w, 1, 1, 32)
    for layout in ("nchw", "nhwc"):
        assert np.abs(ops.conv2d_grouped(x, w, 1, 1, 32, layout) - want).max() <= tol_of(want, 4)


@pytest.mark.parametrize("cg", [(128, 32), (1024, 32), (2048, 32)])
def test_grouped_epilogue(cg):
    C, G = cg
    B, H, Wd = 2, 6, 7
    x, w = rnd((B, C, H, Wd), 31 + C), rnd((C, C // G, 3, 3), 32 + C) / np.float32(np.sqrt(9 * C // G))
    g = np.random.default_rng(33 + C)
    sc, sh = g.random(C, dtype=np.float32) + 0.5, g.standard_normal(C, dtype=np.float32)
    res = rnd((B, C, H, Wd), 34 + C)
    conv = grouped_oracle(x, w, 1, 1, G)
    bc = lambda v: v[None, :, None, None]
    for scale, shift, residual, relu in ((sc, sh, res, True), (sc, sh, None, True), (None, sh, None, False),
                                         (sc, None, res, False), (None, None, None, True)):
        ref = conv * (bc(scale) if scale is not None else 1) + (bc(shift) if shift is not None else 0)
        if residual is not None:
            ref = ref + residual
        if relu:
            ref = np.maximum(ref, 0)
        got = ops.conv2d_grouped_nhwc(x, w, 1, 1, G, scale, shift, residual, relu)
        assert np.abs(got - ref).max() <= 2e-5 * float(np.abs(ref).max()) + 1e-6
    # the residual counts
    a = ops.conv2d_grouped_nhwc(x, w, 1, 1, G, sc, sh, res, False)
    b = ops.conv2d_grouped_nhwc(x, w, 1, 1, G, sc, sh, None, False)
    assert np.abs((a - b) - res).max() <= 1e-5 * float(np.abs(a).max()) + 1e-6 and np.abs(a - b).max() > 1.0


# B, Cin, Cout, G, H, W, k, stride, pad: shapes the super-group kernel does not take
DIRECT = [(2, 12, 8, 4, 5, 5, 1, 1, 0), (1, 24, 36, 12, 7, 6, 3, 2, 1), (2, 96, 96, 2, 5, 4, 3, 1, 1),
          (1, 64, 64, 16, 6, 6, 5, 1, 2), (1, 64, 128, 32, 5, 5, 3, 1, 1)]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("case", DIRECT)
def test_grouped_direct_is_bit_exact_with_reference_order(case, layout):
    B, Cin, Cout, G, H, Wd, k, s, p = case
    x, w = rnd((B, Cin, H, Wd), sum(case)), rnd((Cout, Cin // G, k, k), sum(case) + 1)
    assert np.array_equal(ops.conv2d_grouped(x, w, s, p, G, layout), grouped_oracle(x, w, s, p, G))
    assert np.array_equal(ops.conv2d_grouped_nhwc(x, w, s, p, G), grouped_oracle(x, w, s, p, G))


def run_grouped_nhwc(x, w, s, p, G, scale, shift, residual, relu, offs):
    """rn_conv2d_grouped_pack_weight_dt + rn_conv2d_grouped_nhwc_forward_dt on views between guard bands"""
    B, Cin, H, Wd = x.shape
    Cout, _, k, _ = w.shape
    what = f"rn_conv2d_grouped_nhwc_forward_dt {x.shape} w={w.shape} G={G} s={s} offs={offs}"
    ho, wo = V.out_size(H, k, s, p), V.out_size(Wd, k, s, p)
    pn = int(L.lib().rn_conv2d_grouped_packed_weight_numel_dt(L.RN_DTYPE_F32, Cin, Cout, k, G))
    vw0, vp = V.place(w), V.place_out(pn * 4, offs.get("weight", 0))
    V.must("rn_conv2d_grouped_pack_weight_dt", L.RN_DTYPE_F32, vw0.ptr, vp.ptr, Cin, Cout, k, G)
    packed = V.fetch(vp, np.float32, what + " pack")
    vi, vw = V.place(V._dev(x, "nhwc"), offs.get("inp", 0)), V.place(packed, offs.get("weight", 0))
    vsc = V.place(scale, offs.get("scale", 0)) if scale is not None else None
    vsh = V.place(shift, offs.get("shift", 0)) if shift is not None else None
    vr = V.place(V._dev(residual, "nhwc"), offs.get("residual", 0)) if residual is not None else None
    vo = V.place_out(B * Cout * ho * wo * 4, offs.get("out", 0))
    ep = L.Epilogue(vsc.ptr if vsc else None, vsh.ptr if vsh else None, vr.ptr if vr else None, int(relu))
    V.must("rn_conv2d_grouped_nhwc_forward_dt", L.RN_DTYPE_F32, L.RN_DTYPE_F32, vi.ptr, vo.ptr, vw.ptr, k, s, p, ho, wo,
           B, Cin, Cout, H, Wd, G, ctypes.byref(ep))
    V.check_guards(what, vi, vw, vsc, vsh, vr)
    return V._host(V.fetch(vo, np.float32, what), (B, Cout, ho, wo), "nhwc")


def run_grouped(x, w, s, p, G, layout, offs):
    B, Cin, H, Wd = x.shape
    Cout, _, k, _ = w.shape
    what = f"rn_conv2d_grouped_forward {layout} {x.shape} w={w.shape} G={G} s={s} offs={offs}"
    ho, wo = V.out_size(H, k, s, p), V.out_size(Wd, k, s, p)
    vi, vw = V.place(V._dev(x, layout), offs.get("inp", 0)), V.place(w, offs.get("weight", 0))
    vo = V.place_out(B * Cout * ho * wo * 4, offs.get("out", 0))
    V.must("rn_conv2d_grouped_forward", vi.ptr, vo.ptr, vw.ptr, k, s, p, ho, wo, B, Cin, Cout, H, Wd, G, layout=layout)
    V.check_guards(what, vi, vw)
    return V._host(V.fetch(vo, np.float32, what), (B, Cout, ho, wo), layout)


@pytest.mark.parametrize("cg", [(128, 32), (256, 32), (2048, 32)])
def test_views_16_byte_fast_4_byte_direct_bands_intact(cg):
    """every operand on a 16-byte boundary: the matrix-core kernel (within tolerance of the oracle); one of them
    4 bytes off: the direct kernel, bit for bit the oracle; the guard bands around every tensor stay as uploaded"""
    C, G = cg
    x, w = rnd((2, C, 5, 9), 70 + C), rnd((C, C // G, 3, 3), 71 + C)
    want = grouped_oracle(x, w, 1, 1, G)
    for layout in ("nchw", "nhwc"):
        for offs in V.offset_configs(("inp", "weight", "out"), offsets=(4, 16)):
            got = run_grouped(x, w, 1, 1, G, layout, offs)
            if any(v % 16 for v in offs.values()):
                assert np.array_equal(got, want), (layout, offs)
            else:
                assert np.abs(got - want).max() <= tol_of(want, C // G), (layout, offs)
    g = np.random.default_rng(72)
    sc, sh, res = g.random(C, dtype=np.float32) + 0.5, g.standard_normal(C, dtype=np.float32), rnd(want.shape, 73)
    ref = np.maximum(want * sc[None, :, None, None] + sh[None, :, None, None] + res, 0)
    for offs in V.offset_configs(("inp", "weight", "out", "scale", "shift", "residual"), offsets=(4,)):
        got = run_grouped_nhwc(x, w, 1, 1, G, sc, sh, res, True, offs)
        assert np.abs(got - ref).max() <= 2e-5 * float(np.abs(ref).max()) + 1e-6, offs


@pytest.mark.parametrize("cg", [(128, 32), (512, 32), (2048, 32)])
def test_fast_path_against_direct_path(cg):
    C, G = cg
    x, w = rnd((2, C, 9, 8), 90 + C), rnd((C, C // G, 3, 3), 91 + C)
    fast = run_grouped_nhwc(x, w, 2, 1, G, None, None, None, False, {})
    direct = run_grouped_nhwc(x, w, 2, 1, G, None, None, None, False, {"inp": 4})
    want = grouped_oracle(x, w, 2, 1, G)
    assert np.array_equal(direct, want)
    assert np.abs(fast - direct).max() <= tol_of(want, C // G)


@pytest.mark.parametrize("cg", SHAPES)
def test_no_leakage_between_groups(cg):
    C, G = cg
    cgs = C // G
    x, w = rnd((1, C, 6, 7), 50 + C), rnd((C, cgs, 3, 3), 51 + C)
    for ch in (0, cgs + 1, C - 1):
        x2 = x.copy()
        x2[:, ch] += 3.0
        grp = ch // cgs
        for layout in ("nchw", "nhwc"):
            a, b = ops.conv2d_grouped(x, w, 1, 1, G, layout), ops.conv2d_grouped(x2, w, 1, 1, G, layout)
            other = np.ones(C, bool)
            other[grp * cgs:(grp + 1) * cgs] = False
            assert np.array_equal(a[:, other], b[:, other]), (cg, ch, layout)
            assert not np.array_equal(a[:, ~other], b[:, ~other])


@pytest.mark.parametrize("cg", [(128, 32), (512, 32), (2048, 32)])
def test_nan_in_one_group_stays_inside_its_super_group(cg):
    """rn_hip.h: on the fast path a non-finite input may surface in the other groups of its 32-channel super-group,
    never outside it; the direct kernel keeps it inside its group."""
    C, G = cg
    cgs = C // G
    x, w = rnd((1, C, 5, 5), 60 + C), rnd((C, cgs, 3, 3), 61 + C)
    ch = 37
    x[0, ch, 2, 2] = np.nan
    fast = ops.conv2d_grouped(x, w, 1, 1, G, "nhwc")
    bad = np.isnan(fast).any(axis=(0, 2, 3))
    sg = ch // 32
    grp = np.zeros(C, bool)
    grp[ch // cgs * cgs:(ch // cgs + 1) * cgs] = True
    assert bad[grp].all()                                        # it does surface in its own group
    if cgs >= 32:
        assert not bad[~grp].any()                               # no structural zeros: confined to the group
    else:
        assert not bad[:sg * 32].any() and not bad[(sg + 1) * 32:].any()
    assert np.isfinite(fast[0, :, 0, 0]).all()                   # and only in the pixels that read it
    direct = run_grouped_nhwc(x, w, 1, 1, G, None, None, None, False, {"out": 4})
    assert np.array_equal(np.isnan(direct).any(axis=(0, 2, 3)), grp)


def test_bf16_route_is_the_dense_panel():
    """bf16: the dense contraction on the zero-filled dense weight -- the same bits as building that weight by hand"""
    C, G = 128, 32
    x, w = rnd((2, C, 6, 5), 80), rnd((C, C // G, 3, 3), 81) / 6
    dense = np.zeros((C, C, 3, 3), np.float32)
    for o in range(C):
        g = o // (C // G)
        dense[o, g * 4:(g + 1) * 4] = w[o]
    got = ops.conv2d_grouped_nhwc_bf16(x, w, 1, 1, G)
    assert np.array_equal(got, ops.conv2d_nhwc_bf16(x, dense, 1, 1))
    want = grouped_oracle(ops.bf16_round(x), ops.bf16_round(w), 1, 1, G)
    assert np.abs(got - want).max() <= 2.0 ** -8 * float(np.abs(want).max()) + 1e-6


def test_groups_one_and_bad_groups_are_refused():
    ctx, lib = R.get_ctx(), L.lib()
    x = R.FloatTensor.from_numpy(rnd((1, 32, 4, 4), 1), R.Device.GPU)
    w = R.FloatTensor.from_numpy(rnd((32, 32, 3, 3), 2), R.Device.GPU)
    out = R.FloatTensor((1, 32, 4, 4), R.Device.GPU)
    for g in (1, 3, 0):
        assert lib.rn_conv2d_grouped_forward(ctx.handle, x.data(), out.data(), w.data(), 3, 1, 1, 4, 4, 1, 32, 32, 4, 4,
                                             g) == L.RN_ERR_INVALID


# ---------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def state_of(arch):
    return W.generate_state(arch, seed=0)


def ref_logits(arch, state, x):
    return N.ref_logits(state, bottleneck_features_f64(arch, state, x))


@pytest.mark.parametrize("arch", ["resnext50_32x4d", "wide_resnet50_2"])
def test_model_matches_f64_forward(arch, finch):
    """op by op, fused, fused without pair fusion: logits within TOL of the float64 forward, B = 2"""
    state = state_of(arch)
    x = np.concatenate([finch, W.generate_input(1, seed=5)])
    want = ref_logits(arch, state, x)
    m = R.NativeModel(arch, state=state)
    try:
        ops_ = m.forward(x, fused=False)
        fused = m.forward(x, fused=True)
        m.set_pair_fusion(False)
        nopair = m.forward(x, fused=True)
    finally:
        m.close()
    for label, got in (("ops", ops_), ("fused", fused), ("fused, no pair", nopair)):
        err = float(np.abs(got - want).max())
        print(f"\n{arch} {label}: max |fp32 - fp64| = {err:.3e}")
        assert err <= TOL, (arch, label, err)
        assert np.array_equal(got.argmax(1), want.argmax(1))


@pytest.mark.parametrize("arch", ["resnext101_32x8d", "resnext101_64x4d", "wide_resnet101_2"])
def test_deep_models_match_f64_forward(arch, finch):
    state = W.generate_state(arch, seed=0)
    want = ref_logits(arch, state, finch)
    m = R.NativeModel(arch, state=state)
    try:
        got = m.forward(finch, fused=True)
    finally:
        m.close()
    err = float(np.abs(got - want).max())
    print(f"\n{arch} fused: max |fp32 - fp64| = {err:.3e}")
    assert err <= TOL, (arch, err)


@functools.lru_cache(maxsize=None)
def recentred(arch):
    finch = np.fromfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finch_224.bin"),
                        np.float32).reshape(1, 3, 224, 224)
    x16 = N.structured_inputs(finch)
    state = state_of(arch)
    st, want = N.recentre_fc(state, bottleneck_features_f64(arch, state, x16), spread=1.0)
    return x16, st, want


@pytest.mark.parametrize("arch", ["resnext50_32x4d", "wide_resnet50_2"])
def test_top1_follows_the_image(arch):
    x16, st, want = recentred(arch)
    top = want.argmax(1)
    assert len(set(top.tolist())) >= 8, top
    sep = N.top2_gap(want) > 10 * TOL
    assert sep.sum() >= 12
    m = R.NativeModel(arch, state=st)
    try:
        for fused in (True, False):
            got = m.forward(x16, fused=fused)
            err = float(np.abs(got - want).max())
            print(f"\n{arch} fused={fused}: {len(set(top.tolist()))} classes, max |fp32 - fp64| = {err:.3e}")
            assert err <= TOL, (arch, fused, err)
            assert np.array_equal(got.argmax(1)[sep], top[sep])
    finally:
        m.close()


def _rb(a):
    return a.to(torch.float32).to(torch.bfloat16).to(torch.float64)


@torch.no_grad()
def features_bf16_emulated(arch, state, x):
    """oracle.netref.features_bf16_emulated with torch's grouped convolution for conv2: the roundings of the
    driver's bf16 storage (image, weight panels, every stored activation; the pair panel of a stage's first block
    carries both batch-norm scales), float64 sums"""
    t = lambda k: torch.from_numpy(np.asarray(state[k], dtype=np.float64))
    q = lambda k: _rb(t(k))
    groups = W.family_of(arch)[1]
    h = _rb(torch.from_numpy(np.asarray(x, dtype=np.float64)))
    sc, sh = N._fold(state, "bn1")
    h = F.relu(N._affine(F.conv2d(h, q("conv1.weight"), stride=2, padding=3), sc, sh))
    h = _rb(F.max_pool2d(h, 3, 2, 1))
    for pre, _cin, _mid, _cout, s, has_ds in W.iter_blocks(arch):
        sc1, sh1 = N._fold(state, f"{pre}.bn1")
        sc2, sh2 = N._fold(state, f"{pre}.bn2")
        sc3, sh3 = N._fold(state, f"{pre}.bn3")
        y = _rb(F.relu(N._affine(F.conv2d(h, q(f"{pre}.conv1.weight")), sc1, sh1)))
        y = _rb(F.relu(N._affine(F.conv2d(y, q(f"{pre}.conv2.weight"), stride=s, padding=1, groups=groups), sc2, sh2)))
        if has_ds:
            scd, shd = N._fold(state, f"{pre}.downsample.1")
            w3 = _rb(t(f"{pre}.conv3.weight") * sc3[:, None, None, None])
            wd = _rb(t(f"{pre}.downsample.0.weight") * scd[:, None, None, None])
            z = F.conv2d(y, w3) + F.conv2d(h, wd, stride=s) + (sh3 + shd)[None, :, None, None]
        else:
            z = N._affine(F.conv2d(y, q(f"{pre}.conv3.weight")), sc3, sh3) + h
        h = _rb(F.relu(z))
    return _rb(h.mean(dim=(2, 3))).numpy()


@pytest.mark.parametrize("arch", ["resnext50_32x4d", "wide_resnet50_2"])
def test_bf16_within_the_emulated_rounding_error(arch):
    """bf16 storage: logits within 2.5x the error of the CPU emulation of the bf16 roundings (both against
    float64), and the inputs' spread is more than 5x that bound"""
    x16, st, want = recentred(arch)
    emul = N.logits_bf16_emulated(st, features_bf16_emulated(arch, st, x16))
    bound = 2.5 * float(np.abs(emul - want).max())
    spread = N.logit_spread(want)
    m = R.NativeModel(arch, state=st, dtype="bf16")
    try:
        got = m.forward(x16, fused=True)
    finally:
        m.close()
    err = float(np.abs(got - want).max())
    print(f"\n{arch} bf16: max |bf16 - fp64| = {err:.3e}, emulation {bound / 2.5:.3e}, spread {spread:.3e}")
    assert spread > 5 * bound, (spread, bound)
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rescheduling_changes_no_bit(finch, dtype):
    """resnext50_32x4d: batch position, streams, depth-first front, tuning, graph capture, the host pipeline, a shard
    group (device 0 twice) and the byte route only reschedule the same arithmetic."""
    arch = "resnext50_32x4d"
    state = state_of(arch)
    m = R.NativeModel(arch, state=state, dtype=dtype)
    try:
        x5 = W.generate_input(5, seed=41)
        x5[2] = finch[0]
        base5 = m.forward(x5, fused=True)
        for i in (0, 2, 4):
            assert np.array_equal(m.forward(x5[i:i + 1], fused=True), base5[i:i + 1])
        B = 128
        x = W.generate_input(B, seed=42)
        x[7] = finch[0]
        m.set_streams(1)
        want = m.forward(x, fused=True)
        assert np.array_equal(want[7:8], base5[2:3])
        m.set_streams(2)
        assert m.parts(B) == 2
        assert np.array_equal(m.forward(x, fused=True), want)
        m.set_front_parts(4)
        assert np.array_equal(m.forward(x, fused=True), want)
        m.set_front_parts(1)
        xin = R.FloatTensor.from_numpy(x5, R.Device.GPU)
        out = R.FloatTensor((5, 1000), R.Device.GPU)
        m.tune(xin.data(), 5, out.data(), True)
        m.ctx.sync()
        assert np.array_equal(out.numpy(), base5)
        assert np.array_equal(m.forward(x5, fused=True), base5)
        xd = R.FloatTensor.from_numpy(x[:8], R.Device.GPU)
        o8 = R.FloatTensor((8, 1000), R.Device.GPU)
        g = R.Graph(m, xd.data(), 8, o8.data(), fused=True)
        L.check(L.lib().rn_memset(m.ctx.handle, o8.data(), 0, 8 * 4000), "memset", m.ctx.handle)
        g.launch(); g.launch(); m.ctx.sync()
        assert np.array_equal(o8.numpy(), want[:8])
        g.close()
        pipe = R.Pipeline(m, 16, fused=True)
        got = list(pipe.run([x[:16], x[16:32]]))
        pipe.close()
        assert np.array_equal(got[0], want[:16]) and np.array_equal(got[1], want[16:32])
        # 8-bit RGB input: the same logits as the host-normalised image
        px = np.random.default_rng(9).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
        mean, std = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
        xn = ((px.astype(np.float32) / np.float32(255.0) - mean) / std).transpose(0, 3, 1, 2)
        assert np.array_equal(m.forward_u8(px, fused=True), m.forward(np.ascontiguousarray(xn), fused=True))
    finally:
        m.close()
    sh = R.ShardedModel([0, 0], arch, state=state, dtype=dtype)
    try:
        logits, top1 = sh.forward(x[:10], fused=True)
        assert np.array_equal(logits, want[:10])
        assert np.array_equal(top1, want[:10].argmax(1).astype(np.uint64))
    finally:
        sh.close()


def test_create_ex_refuses_what_it_does_not_build():
    ctx, lib = R.get_ctx(), L.lib()
    h = ctypes.c_void_p()
    for depth, g, wpg in ((50, 2, 64), (50, 32, 3), (18, 32, 4), (34, 1, 128), (50, 64, 8), (49, 32, 4), (50, 0, 64)):
        assert lib.rn_model_create_ex(ctx.handle, ctypes.byref(h), depth, g, wpg) == L.RN_ERR_UNSUPPORTED
        assert not h.value
    for depth, g, wpg in ((50, 1, 64), (101, 32, 8), (101, 64, 4), (152, 1, 128)):
        assert lib.rn_model_create_ex(ctx.handle, ctypes.byref(h), depth, g, wpg) == L.RN_OK
        assert lib.rn_model_destroy(h) == L.RN_OK


def test_create_ex_1_64_is_rn_model_create(finch, state50):
    ctx, lib = R.get_ctx(), L.lib()
    a = R.NativeModel("resnet50", state=state50)
    try:
        want = a.forward(finch)
        per_img = a.activation_bytes()
    finally:
        a.close()
    b = R.NativeModel.__new__(R.NativeModel)
    h = ctypes.c_void_p()
    L.check(lib.rn_model_create_ex(ctx.handle, ctypes.byref(h), 50, 1, 64), "create_ex", ctx.handle)
    b.ctx, b.arch, b.handle, b.dtype = ctx, "resnet50", h, "f32"
    try:
        for key, numel in b.tensor_keys():
            arr = np.ascontiguousarray(state50[key], dtype=np.float32)
            L.check(lib.rn_model_set_tensor(h, key.encode(), arr.ctypes.data, numel), key, ctx.handle)
        L.check(lib.rn_model_finalize(h), "finalize", ctx.handle)
        assert np.array_equal(b.forward(finch), want)
        assert b.activation_bytes() == per_img == 4 * (230 * 230 * 4 + 3 * 112 * 112 * 64 + 2 * 56 * 56 * 128 + 2048)
    finally:
        b.close()


def test_tuning_table_tells_the_families_apart(state50):
    x = W.generate_input(2, seed=1)
    a = R.NativeModel("resnet50", state=state50)
    b = R.NativeModel("resnext50_32x4d", state=state_of("resnext50_32x4d"))
    try:
        xin = R.FloatTensor.from_numpy(x, R.Device.GPU)
        out = R.FloatTensor((2, 1000), R.Device.GPU)
        a.tune(xin.data(), 2, out.data(), True)
        b.tune(xin.data(), 2, out.data(), True)
        wa, wb = a.export_tuning(), b.export_tuning()
        assert wa[9] == 0 and wb[9] == (32 << 32 | 4) and len(wa) == len(wb)
        with pytest.raises(L.RnError):
            b.import_tuning(wa)
        with pytest.raises(L.RnError):
            a.import_tuning(wb)
        a.import_tuning(wa)
        b.import_tuning(wb)
    finally:
        a.close()
        b.close()


def test_profile_accounts_for_every_reference_op(finch):
    arch = "resnext50_32x4d"
    m = R.NativeModel(arch, state=state_of(arch))
    try:
        m.set_profiling(True)
        m.forward(finch, fused=False)
        recs = m.profile()
    finally:
        m.close()
    count = lambda op: sum(r["op"] == op for r in recs)
    assert (count("conv2d"), count("batchnorm2d"), count("relu"), count("add")) == (53, 53, 49, 16)
    flops = sum(r["flops"] for r in recs)
    assert abs(flops - W.forward_flops(arch)) < 1.0


def test_weights_dir_and_arena_sizes(finch, tmp_path):
    arch = "wide_resnet50_2"
    state = state_of(arch)
    W.save_weights_bin(state, str(tmp_path))
    a = R.NativeModel(arch, weights_dir=str(tmp_path))
    b = R.NativeModel(arch, state=state)
    try:
        assert np.array_equal(a.forward(finch), b.forward(finch))
        assert a.activation_bytes() == 4 * (230 * 230 * 4 + 3 * 112 * 112 * 64 + 2 * 56 * 56 * 256 + 2048)
    finally:
        a.close()
        b.close()
