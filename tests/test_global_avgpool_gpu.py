"""rn_global_avgpool_nhwc_forward_dt: the mean over any H x W map, fp32 and bf16 storage, against float64; the
7 x 7 bits of rn_avgpool2d_nhwc_forward_dt; a summation order that depends on (H, W) alone; the refusals."""
import numpy as np
import pytest

import resnet_c_amd as R
from bf16_ref import half_step
from resnet_c_amd import _lib as L
from resnet_c_amd import ops
from resnet_c_amd.tensor import _DeviceBuffer

pytestmark = pytest.mark.gpu

SHAPES = [(3, 64, 1, 1), (2, 2048, 7, 7), (2, 64, 2, 3), (5, 8, 5, 9), (1, 512, 16, 16), (3, 72, 33, 17), (257, 8, 4, 3)]
U = 2.0 ** -24  # unit roundoff of fp32


def make_input(shape, seed):
    """mixed signs, values over several binades and a few large ones: a wrong order or a dropped tap shows"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) * np.exp2(rng.integers(-6, 3, shape))
    big = rng.random(shape) < 0.01
    x[big] *= 300.0
    return x.astype(np.float32)


_CASES = {}


def case(shape, bf16):
    """input as the kernel sees it (NCHW fp32 values, bf16-rounded for bf16 storage), its float64 mean and
    mean|x| per output, and the kernel's result: computed once per (shape, dtype), shared, never changed"""
    key = (shape, bf16)
    if key not in _CASES:
        x = make_input(shape, seed=sum(shape))
        if bf16:
            x = ops.bf16_round(x)
        x64 = x.astype(np.float64)
        got = ops.global_avgpool(x, bf16=bf16)
        for a in (x, got):
            a.setflags(write=False)
        _CASES[key] = (x, x64.mean(axis=(2, 3)), np.abs(x64).mean(axis=(2, 3)), got)
    return _CASES[key]


def fp32_bound(shape, mean_abs):
    """first-order bound of ANY fp32 summation order of T terms plus the division: T * 2^-24 * mean|x|"""
    return shape[2] * shape[3] * U * mean_abs


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_within_the_summation_bound(shape):
    x, ref, mean_abs, got = case(shape, False)
    assert got.shape == shape[:2] and got.dtype == np.float32
    err, bound = np.abs(got.astype(np.float64) - ref), fp32_bound(shape, mean_abs)
    print(f"fp32 {shape}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bf16_within_half_an_ulp_of_the_fp32_value(shape):
    """the fp32 value lies within fp32_bound of the float64 mean; the stored bf16 is that value rounded once"""
    x, ref, mean_abs, got = case(shape, True)
    bound = fp32_bound(shape, mean_abs)
    hs = np.maximum(np.maximum(half_step(ref - bound), half_step(ref + bound)), half_step(ref))
    err = np.abs(got.astype(np.float64) - ref)
    assert np.array_equal(ops.bf16_round(got), got)  # bf16 values
    print(f"bf16 {shape}: max err / (bound + half ulp) = {float((err / (bound + hs + 1e-300)).max()):.3f}")
    assert (err <= bound + hs).all()


def _avgpool2d_dt(x, bf16):
    """rn_avgpool2d_nhwc_forward_dt with the kernel the size of the (square) map"""
    ctx = R.get_ctx()
    B, C, H, W = x.shape
    nhwc = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    dx = ops._up_raw(ops.to_bf16_bits(nhwc) if bf16 else nhwc)
    out = _DeviceBuffer(ctx, B * C * 4)
    L.check(L.lib().rn_avgpool2d_nhwc_forward_dt(ctx.handle, L.RN_DTYPE_BF16 if bf16 else L.RN_DTYPE_F32, dx.ptr, out.ptr,
                                                 H, 1, 0, 1, 1, B, C, H, W), "rn_avgpool2d_nhwc_forward_dt", ctx.handle)
    ctx.sync()
    if bf16:
        return ops.from_bf16_bits(ops._down_raw(out, np.uint16, B * C)).reshape(B, C)
    return ops._down_raw(out, np.float32, B * C).reshape(B, C)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_7x7_is_the_existing_kernel_bit_for_bit(bf16):
    x, _, _, got = case((2, 2048, 7, 7), bf16)
    want = _avgpool2d_dt(x, bf16)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(257, 8, 4, 3), (3, 72, 33, 17)], ids=["B257", "33x17"])
def test_order_does_not_depend_on_the_batch(shape, bf16):
    """row i of a B-image launch == the same image run alone (another grid, another place in it)"""
    x, _, _, got = case(shape, bf16)
    rows = [0, shape[0] // 2, shape[0] - 1]
    for i in rows:
        alone = ops.global_avgpool(x[i:i + 1], bf16=bf16)
        assert np.array_equal(alone.view(np.uint32), got[i:i + 1].view(np.uint32)), i
    # and inside a batch of another size, at another position
    pair = ops.global_avgpool(x[[rows[2], rows[1]]], bf16=bf16)
    assert np.array_equal(pair.view(np.uint32), got[[rows[2], rows[1]]].view(np.uint32))


def test_order_is_the_documented_one():
    """the comment above global_avgpool_kernel restated: slices of L = ceil(T / S) taps added in ascending order
    in fp32, the slice sums added in ascending order, one division by T"""
    shape = (3, 72, 33, 17)
    x, _, _, got = case(shape, False)
    T = shape[2] * shape[3]
    S = 1
    while S < 16 and S * 16 < T:
        S *= 2
    Lc = -(-T // S)
    taps = x.reshape(shape[0], shape[1], T)
    total = None
    for s in range(-(-T // Lc)):
        p = np.zeros(shape[:2], dtype=np.float32)
        for t in range(s * Lc, min(T, (s + 1) * Lc)):
            p = p + taps[:, :, t]
        total = p if total is None else total + p
    want = total / np.float32(T)
    assert want.dtype == np.float32 and np.array_equal(want.view(np.uint32), got.view(np.uint32))


def test_refusals_launch_nothing():
    ctx, lib = R.get_ctx(), L.lib()
    B, C, H, W = 2, 16, 3, 5
    a = _DeviceBuffer(ctx, B * C * H * W * 4 + 64)
    b = _DeviceBuffer(ctx, B * C * 4 + 64)
    before = lib.rn_ctx_launch_count(ctx.handle)
    f32, bf = L.RN_DTYPE_F32, L.RN_DTYPE_BF16
    bad = [
        (f32, None, b.ptr, B, C, H, W), (f32, a.ptr, None, B, C, H, W),          # null
        (bf, None, b.ptr, B, C, H, W), (bf, a.ptr, None, B, C, H, W),
        (f32, a.ptr, a.ptr, B, C, H, W), (bf, a.ptr, a.ptr, B, C, H, W),         # aliased
        (f32, a.ptr + 4, b.ptr, B, C, H, W), (f32, a.ptr, b.ptr + 8, B, C, H, W),  # off a 16-byte boundary
        (bf, a.ptr + 2, b.ptr, B, C, H, W), (bf, a.ptr, b.ptr + 4, B, C, H, W),
        (f32, a.ptr, b.ptr, B, 6, H, W), (f32, a.ptr, b.ptr, B, 3, H, W),        # C % 4
        (bf, a.ptr, b.ptr, B, 12, H, W), (bf, a.ptr, b.ptr, B, 4, H, W),         # C % 8
        (7, a.ptr, b.ptr, B, C, H, W),                                           # unknown dtype
    ]
    for dt, i, o, *dims in bad:
        st = lib.rn_global_avgpool_nhwc_forward_dt(ctx.handle, dt, i, o, *dims)
        assert st == L.RN_ERR_INVALID, (dt, dims)
        assert b"rn_global_avgpool_nhwc_forward_dt" in lib.rn_last_error(ctx.handle)
    assert lib.rn_global_avgpool_nhwc_forward_dt(None, f32, a.ptr, b.ptr, B, C, H, W) == L.RN_ERR_INVALID
    assert lib.rn_global_avgpool_nhwc_forward_dt(ctx.handle, f32, a.ptr, b.ptr, 0, C, H, W) == L.RN_OK  # nothing to do
    assert lib.rn_ctx_launch_count(ctx.handle) == before
    assert lib.rn_global_avgpool_nhwc_forward_dt(ctx.handle, f32, a.ptr, b.ptr, B, C, H, W) == L.RN_OK
    ctx.sync()
    assert lib.rn_ctx_launch_count(ctx.handle) == before + 1
