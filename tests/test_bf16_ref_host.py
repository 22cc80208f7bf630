"""tests/bf16_ref.py discriminates: numpy emulations of one small fused bf16 layer (64 -> 64 channels, 3x3,
residual + ReLU, K = 576) -- a right kernel with another summation order passes assert_bf16_rounded, four
subtly wrong ones do not.  This is the evidence that test_bf16_rounding_gpu.py would notice such a kernel;
the tensor-maximum bound (2**-8 * max|want| + 1e-5) accepts the last two of them outright and the first two at
all but the few elements of the largest binade."""
import numpy as np
import pytest

import bf16_ref as BR
from oracle import oracle as O
from resnet_c_amd import ops

B, C, H, W, K = 2, 64, 9, 9, 576


def truncate_bf16(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32).reshape(np.shape(a))


class Layer:
    """The operands as the kernel sees them, the float64 reference, and the fp32 products per output element."""

    def __init__(self):
        g = np.random.default_rng(20)
        self.x = ops.bf16_round(g.standard_normal((B, C, H, W), dtype=np.float32))
        self.w = ops.bf16_round(g.standard_normal((C, C, 3, 3), dtype=np.float32) / np.float32(np.sqrt(K)))
        self.scale = g.random(C, dtype=np.float32) + np.float32(0.5)
        self.shift = g.standard_normal(C, dtype=np.float32)
        self.res32 = g.standard_normal((B, C, H, W), dtype=np.float32)
        self.res = ops.bf16_round(self.res32)
        self.ref = BR.epilogue64(BR.conv64(self.x, self.w, 1, 1), self.scale, self.shift, self.res, True)
        xp = np.zeros((B, C, H + 2, W + 2), dtype=np.float32)
        xp[:, :, 1:-1, 1:-1] = self.x
        cols = np.stack([xp[:, :, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)], axis=2)  # B,C,9,H,W
        self.cols = np.ascontiguousarray(cols.transpose(0, 3, 4, 1, 2).reshape(B * H * W, K))      # k = c * 9 + tap
        self.wk = self.w.reshape(C, K)

    def acc32(self, order, drop=None):
        """fp32 accumulation of the (exact) fp32 products, one k at a time in `order`; drop = (row, cout, k)"""
        acc = np.zeros((B * H * W, C), dtype=np.float32)
        for k in order:
            prod = self.cols[:, k, None] * self.wk[None, :, k]      # bf16 x bf16: exact in fp32
            if drop is not None and drop[2] == k:
                prod[drop[0], drop[1]] = 0.0
            acc += prod
        return acc.reshape(B, H, W, C).transpose(0, 3, 1, 2)

    def epilogue32(self, acc, res):
        bc = lambda v: v[None, :, None, None]
        return np.maximum(acc * bc(self.scale) + bc(self.shift) + res, np.float32(0))


@pytest.fixture(scope="module")
def layer():
    return Layer()


@pytest.fixture(scope="module")
def acc(layer):
    return layer.acc32(range(K))


def old_bound_accepts(got, ref):
    return np.abs(got - ref).max() <= 2 ** -8 * np.abs(ref).max() + 1e-5


def old_bound_misses(got, ref):
    """the share of the elements outside the per-element bound that the tensor-maximum bound lets through"""
    err = np.abs(got - ref)
    wrong = err > BR.half_step(ref) + BR.eps_sum(ref, K)
    return float((err[wrong] <= 2 ** -8 * np.abs(ref).max() + 1e-5).mean())


def test_conv64_is_the_oracle_convolution(layer):
    for (s, p, shape) in ((1, 1, (C, C, 3, 3)), (2, 0, (72, C, 1, 1)), (2, 3, (8, C, 7, 7))):
        w = np.random.default_rng(sum(shape)).standard_normal(shape, dtype=np.float32) / np.float32(np.sqrt(np.prod(shape[1:])))
        want = O.conv2d(layer.x, w, s, p)
        got = BR.conv64(layer.x, w, s, p)
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.abs(got - want).max() <= 3e-7 * np.sqrt(np.prod(shape[1:])) * np.abs(want).max() + 1e-6
    # groups: each group's slice on its own
    w = np.random.default_rng(5).standard_normal((C, 4, 3, 3), dtype=np.float32)
    got = BR.conv64(layer.x, w, 1, 1, groups=16)
    for g in (0, 7, 15):
        assert np.array_equal(got[:, 4 * g:4 * g + 4], BR.conv64(layer.x[:, 4 * g:4 * g + 4], w[4 * g:4 * g + 4], 1, 1))


def test_half_step_is_half_the_bf16_spacing():
    v = np.array([1.0, 1.99, 2.0, -3.5, 0.0, 2.0 ** -20, 0.75])
    assert np.array_equal(BR.half_step(v), [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 0.0, 2.0 ** -28, 2.0 ** -9])
    # the neighbours of a bf16 value are two half steps away
    one = np.float32(1.0)
    up = ops.from_bf16_bits(ops.to_bf16_bits(one) + np.uint16(1))
    assert float(up[0] - one) == 2 * BR.half_step(1.0)


def test_right_kernel_in_another_summation_order_passes(layer, acc):
    for order in (range(K - 1, -1, -1), [k for c in range(K // 32 - 1, -1, -1) for k in range(32 * c, 32 * c + 32)]):
        got = ops.bf16_round(layer.epilogue32(layer.acc32(order), layer.res))
        m = BR.assert_bf16_rounded(got, layer.ref, K, "reordered fp32 sum")
        assert 0.25 < m["max_err_steps"] <= 0.5 + 1e-2
    # chunks of 32 added as partial sums, ((c0 + c1) + c2) + ...
    parts = [layer.acc32(range(32 * c, 32 * c + 32)) for c in range(K // 32)]
    total = parts[0]
    for part in parts[1:]:
        total = total + part
    BR.assert_bf16_rounded(ops.bf16_round(layer.epilogue32(total, layer.res)), layer.ref, K, "chunked fp32 sum")
    BR.assert_bf16_rounded(ops.bf16_round(layer.epilogue32(acc, layer.res)), layer.ref, K, "plain fp32 sum")


def test_truncation_fails(layer, acc):
    got = truncate_bf16(layer.epilogue32(acc, layer.res))
    assert old_bound_misses(got, layer.ref) > 0.99
    with pytest.raises(AssertionError, match="outside half a bf16 step"):
        BR.assert_bf16_rounded(got, layer.ref, K, "truncated")


def test_rounding_before_the_residual_add_fails(layer, acc):
    bc = lambda v: v[None, :, None, None]
    early = ops.bf16_round(acc * bc(layer.scale) + bc(layer.shift))
    got = ops.bf16_round(np.maximum(early + layer.res, np.float32(0)))
    assert old_bound_misses(got, layer.ref) > 0.99
    with pytest.raises(AssertionError, match="outside half a bf16 step"):
        BR.assert_bf16_rounded(got, layer.ref, K, "rounded twice")


def test_unrounded_residual_fails(layer, acc):
    got = ops.bf16_round(layer.epilogue32(acc, layer.res32))
    assert old_bound_accepts(got, layer.ref)
    with pytest.raises(AssertionError, match="outside half a bf16 step"):
        BR.assert_bf16_rounded(got, layer.ref, K, "fp32 residual")


def test_one_dropped_product_fails(layer, acc):
    # an element well above the ReLU, and the median product of its 576 by magnitude: not a hand-picked large one
    flat = layer.ref.transpose(0, 2, 3, 1).reshape(B * H * W, C)
    row, co = np.unravel_index(int(np.argmin(np.abs(flat - 1.0))), flat.shape)
    prods = np.abs(layer.cols[row].astype(np.float64) * layer.wk[co])
    k = int(np.argsort(prods)[K // 2])
    got = ops.bf16_round(layer.epilogue32(layer.acc32(range(K), drop=(row, co, k)), layer.res))
    good = ops.bf16_round(layer.epilogue32(acc, layer.res))
    assert (got != good).sum() == 1 and old_bound_accepts(got, layer.ref)
    with pytest.raises(AssertionError) as e:
        BR.assert_bf16_rounded(got, layer.ref, K, "dropped product")
    b, hw = divmod(int(row), H * W)
    assert f"worst at ({b}, {int(co)}, {hw // W}, {hw % W})" in str(e.value) and "1 of" in str(e.value)


def test_failure_report_names_the_worst_element():
    ref = np.array([[1.0, 3.0], [0.0, -0.3]])
    got = ops.bf16_round(ref.astype(np.float32))
    BR.assert_bf16_rounded(got, ref, 1)
    got[1, 1] = np.float32(-0.3046875)       # two steps (of 2**-9) off
    with pytest.raises(AssertionError) as e:
        BR.assert_bf16_rounded(got, ref, 1, "unit")
    msg = str(e.value)
    assert "unit: 1 of 4" in msg and "worst at (1, 1)" in msg and "got -0.3046875" in msg and "ref -0.3" in msg
    assert "steps of 1.953e-03" in msg
    nan = got.copy()
    nan[0, 0] = np.nan
    with pytest.raises(AssertionError, match=r"worst at \(0, 0\)"):
        BR.assert_bf16_rounded(nan, ref, 1)
