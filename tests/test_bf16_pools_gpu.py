"""Every target of pool_bf16_dispatch (rn_pool.hip) behind rn_maxpool2d_nhwc_forward_dt /
rn_avgpool2d_nhwc_forward_dt(RN_DTYPE_BF16), bit for bit, and the RN_DTYPE_F32 form of the same entry points.

The expected value is always bf16_round(O.maxpool2d / O.avgpool2d(bf16_round(x), k, s, p)): the maximum takes no
rounding, the average is the fp32 kh-major sum of the in-bounds taps divided by k twice, then one round to
nearest even -- the loop the fp32 NHWC kernels already reproduce bit for bit.  `target_of` restates the
dispatcher's predicates, and every case list asserts the target it is meant for:

    walk      maxpool3s2_walk_kernel<bf16,8>     max, 3/2/1, h_out >= 8
    maxpool3  maxpool3_nhwc_kernel<bf16,8>       max, k = 3, every window holds a real pixel, not the walk
    global    avgpool_global_kernel<bf16,8,49>   average, k = 7 on 7x7, padding 0
    generic   pool_nhwc_bf16_kernel<kMax>        everything else, both forms

Every call runs on views between guard bands (tests/views.py): the output buffer starts as 0xA5 bytes, the
input of an average lies between NaNs and the input of a maximum between +inf (which fmaxf cannot swallow), so
an element never written or a read outside the tensor shows in the result."""
import numpy as np
import pytest

import resnet_c_amd as R
import views as V
from oracle import oracle as O
from resnet_c_amd import _lib as L
from resnet_c_amd import ops

pytestmark = pytest.mark.gpu

BF16, F32 = L.RN_DTYPE_BF16, L.RN_DTYPE_F32
MARGIN = 128  # bf16 +inf elements on each side of a max-pool input (256 bytes, the width of views.GUARD)


def rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def target_of(is_max, k, s, p, H, W):
    ho, wo = V.out_size(H, k, s, p), V.out_size(W, k, s, p)
    if is_max and (k, s, p) == (3, 2, 1) and ho >= 8:
        return "walk"
    if is_max and k == 3 and p < k and (ho - 1) * s < H + p and (wo - 1) * s < W + p:   # windows_never_empty
        return "maxpool3"
    if not is_max and k == 7 and H == 7 and W == 7 and p == 0:
        return "global"
    return "generic"


def entry(is_max):
    return "rn_maxpool2d_nhwc_forward_dt" if is_max else "rn_avgpool2d_nhwc_forward_dt"


def place_input(bits_nhwc, offset, is_max):
    """The bf16 tensor on a view; returns (view, pointer to the first element)."""
    flat = np.ascontiguousarray(bits_nhwc).reshape(-1)
    if not is_max:
        v = V.place(flat, offset)                       # NaN bytes around it
        return v, v.ptr
    inf = np.full(MARGIN, 0x7F80, dtype=np.uint16)
    v = V.place(np.concatenate([inf, flat, inf]), offset)
    return v, v.ptr + 2 * MARGIN


def run_pool(x, k, s, p, is_max, offs=None):
    """One call of the bf16 entry point on NCHW host floats; the output's bf16 bits as [B,C,ho,wo]."""
    offs = offs or {}
    B, C, H, W = x.shape
    ho, wo = V.out_size(H, k, s, p), V.out_size(W, k, s, p)
    what = f"{entry(is_max)} bf16 {x.shape} k={k} s={s} p={p} offs={offs}"
    vi, ptr = place_input(ops.to_bf16_bits(x.transpose(0, 2, 3, 1)).reshape(B, H, W, C), offs.get("inp", 0), is_max)
    vo = V.place_out(B * ho * wo * C * 2, offs.get("out", 0))
    V.must(entry(is_max), BF16, ptr, vo.ptr, k, s, p, ho, wo, B, C, H, W)
    V.check_guards(what, vi)
    return V.fetch(vo, np.uint16, what).reshape(B, ho, wo, C).transpose(0, 3, 1, 2).copy()


def expected(x, k, s, p, is_max):
    with np.errstate(all="ignore"):
        xb = ops.bf16_round(x)
        return ops.bf16_round(O.maxpool2d(xb, k, s, p) if is_max else O.avgpool2d(xb, k, s, p))


def check(bits, want, is_max, what):
    got = ops.from_bf16_bits(bits)
    assert got.shape == want.shape, what
    if is_max:
        assert not np.isnan(got).any(), what
        assert np.array_equal(bits, ops.to_bf16_bits(want).reshape(want.shape)), what
        assert np.array_equal(np.signbit(got), np.signbit(want)), what
    else:
        assert np.array_equal(got, want, equal_nan=True), what
        keep = ~np.isnan(want)
        assert np.array_equal(bits[keep], ops.to_bf16_bits(want).reshape(want.shape)[keep]), what


def run_and_check(case, is_max, target, special=False, offs=None):
    B, H, W, k, s, p = case
    assert target_of(is_max, k, s, p, H, W) == target, (case, target_of(is_max, k, s, p, H, W))
    for C in (8, 24):
        x = rnd((B, C, H, W), 6000 + sum(case) + C)
        if special:
            x = poison(x, is_max)
        what = f"{target} {'max' if is_max else 'avg'} B={B} C={C} {H}x{W} k={k} s={s} p={p} special={special} offs={offs}"
        check(run_pool(x, k, s, p, is_max, offs), expected(x, k, s, p, is_max), is_max, what)


def poison(x, is_max):
    """NaN row and column, rows of NaN that cover whole windows, a -inf block, +inf, bands of 0.0 and -0.0 on a
    negative background (a band of one sign per channel: where both zeros meet in a window the CPU oracle's fmaxf
    returns whichever came last, the device's v_max_f32 +0.0), and for the average two neighbours of 3e38 whose fp32
    sum is inf.  Channels 0..7 of the first / last image, so C = 8 holds them all."""
    x = x.copy()
    B, C, H, W = x.shape
    x[0, 0, H // 2, :] = np.nan
    x[-1, 1, :, W // 2] = np.nan
    x[0, 2, :min(H, 7), :] = np.nan
    x[0, 3, :min(H, 4), :min(W, 4)] = -np.inf
    x[-1, 4, H - 1, W - 1] = np.inf
    x[:, 5:7] = -np.abs(x[:, 5:7]) - 0.5
    x[:, 5, H // 3:H // 3 + 4, :] = -0.0
    x[:, 6, H // 3:H // 3 + 4, :] = 0.0
    if not is_max:
        x[0, 7, 0, :2] = 3e38
    else:
        x[0, 7] = -np.inf       # a whole plane of -inf
    return x


WALK = [(1, 15, 5, 3, 2, 1),    # odd H, h_out = 8 exactly
        (2, 16, 3, 3, 2, 1),
        (3, 17, 1, 3, 2, 1),    # one pixel wide: all three columns clamp to column 0
        (2, 33, 4, 3, 2, 1),    # h_out = 17: two segments, 9 and 8 rows
        (1, 62, 6, 3, 2, 1)]    # h_out = 31: 16 and 15 rows
MAXPOOL3 = [(2, 6, 5, 3, 1, 1), (1, 6, 5, 3, 1, 0), (3, 6, 5, 3, 3, 0), (2, 6, 5, 3, 1, 2), (1, 6, 5, 3, 2, 2),
            (2, 7, 7, 3, 2, 1),     # the network's geometry with h_out = 4 < 8: not the walk
            (3, 5, 13, 3, 2, 1)]
GLOBAL = [(3, 7, 7, 7, 1, 0)]
GENERIC_MAX = [(2, 8, 6, 2, 2, 0), (1, 9, 9, 5, 2, 2),
               (3, 4, 4, 3, 1, 3),  # pad >= k: whole windows in the padding, -inf
               (2, 5, 7, 1, 2, 0)]
GENERIC_AVG = [(2, 8, 6, 2, 2, 0),
               (1, 9, 8, 3, 2, 1),  # the divisor counts padded taps (k * k always)
               (3, 8, 8, 7, 1, 0), (2, 7, 7, 7, 1, 1),   # 7x7 averages that are not the global form
               (3, 1, 1, 3, 1, 1)]


@pytest.mark.parametrize("case", WALK)
def test_walk(case):
    run_and_check(case, True, "walk")


@pytest.mark.parametrize("case", MAXPOOL3)
def test_maxpool3(case):
    run_and_check(case, True, "maxpool3")


@pytest.mark.parametrize("case", GLOBAL)
def test_global_average(case):
    run_and_check(case, False, "global")


@pytest.mark.parametrize("case", GENERIC_MAX)
def test_generic_max(case):
    run_and_check(case, True, "generic")


@pytest.mark.parametrize("case", GENERIC_AVG)
def test_generic_average(case):
    run_and_check(case, False, "generic")


def test_generic_max_windows_in_the_padding_are_minus_inf():
    x = rnd((1, 8, 4, 4), 61)
    bits = run_pool(x, 3, 1, 3, True)
    got = ops.from_bf16_bits(bits)
    assert got.shape == (1, 8, 8, 8)
    assert np.isneginf(got[:, :, 0, :]).all() and np.isneginf(got[:, :, :, -1]).all() and np.isfinite(got[:, :, 1:-1, 1:-1]).all()


# one case per target (and per form of the generic kernel): special values, then offset views
ONE_PER_TARGET = [((2, 33, 4, 3, 2, 1), True, "walk"), ((2, 7, 7, 3, 2, 1), True, "maxpool3"),
                  ((3, 7, 7, 7, 1, 0), False, "global"), ((2, 9, 9, 5, 2, 2), True, "generic"),
                  ((2, 9, 8, 3, 2, 1), False, "generic")]


@pytest.mark.parametrize("case,is_max,target", ONE_PER_TARGET + [((2, 6, 5, 3, 1, 2), True, "maxpool3"),
                                                                 ((2, 8, 8, 7, 1, 0), False, "generic")])
def test_special_values(case, is_max, target):
    run_and_check(case, is_max, target, special=True)


@pytest.mark.parametrize("case,target", [(c, t) for c, m, t in ONE_PER_TARGET if m])
def test_max_of_mixed_zeros_is_plus_zero(case, target):
    """Where +0.0 and -0.0 meet in one window the CPU oracle's fmaxf returns whichever came last, so this pins the
    device's result without it: on a negative background the maximum is a zero wherever the window holds one, and
    +0.0 wherever it holds a +0.0 (v_max_f32 orders -0 < +0 whatever the operand order)."""
    B, H, W, k, s, p = case
    assert target_of(True, k, s, p, H, W) == target
    g = np.random.default_rng(6200 + sum(case))
    x = -np.abs(g.standard_normal((B, 8, H, W), dtype=np.float32)) - np.float32(0.5)
    z = g.random(x.shape)
    x[z < 0.06] = 0.0
    x[(z >= 0.06) & (z < 0.12)] = -0.0
    got = ops.from_bf16_bits(run_pool(x, k, s, p, True))
    any_zero = O.maxpool2d((x == 0).astype(np.float32), k, s, p) == 1
    any_plus = O.maxpool2d(((x == 0) & ~np.signbit(x)).astype(np.float32), k, s, p) == 1
    assert any_plus.any() and (any_zero & ~any_plus).any() and (~any_zero).any()
    assert np.array_equal(got == 0, any_zero)
    assert np.array_equal(got[~any_zero], expected(x, k, s, p, True)[~any_zero])
    assert np.array_equal(np.signbit(got[any_zero]), ~any_plus[any_zero])


@pytest.mark.parametrize("offs", [{"inp": 16, "out": 48}, {"inp": 48, "out": 16}])
@pytest.mark.parametrize("case,is_max,target", ONE_PER_TARGET)
def test_offset_views(case, is_max, target, offs):
    """16 and 48 bytes off the allocation (still on 16-byte boundaries): the same bits, guard bands intact
    (run_pool checks the input's bands, fetch the output's)."""
    run_and_check(case, is_max, target, special=True, offs=offs)


@pytest.mark.parametrize("is_max", [True, False])
def test_refusals_launch_nothing(is_max):
    """Every pointer is a valid allocation of the right size; the library has to refuse before any launch: the
    output, prefilled with NaN bytes, and its guard bands are as uploaded."""
    ctx, lib = R.get_ctx(), L.lib()
    fn = getattr(lib, entry(is_max))
    B, H, W, k, s, p = 2, 9, 9, 3, 2, 1
    ho = wo = V.out_size(H, k, s, p)

    def bufs(C, off_in=0, off_out=0):
        x = ops.to_bf16_bits(rnd((B, H, W, C), 62 + C)).reshape(B, H, W, C)
        vi, ptr = place_input(x, off_in, is_max)
        return vi, ptr, V.place(None, off_out, V.GUARD, "nan", B * ho * wo * C * 2)

    def refused(args, vo, what):
        launches = lib.rn_ctx_launch_count(ctx.handle)
        st = fn(ctx.handle, *args)
        assert st == L.RN_ERR_INVALID, (what, st)
        assert lib.rn_ctx_launch_count(ctx.handle) == launches, what
        assert lib.rn_last_error(ctx.handle), what
        ctx.sync()
        V.assert_untouched(vo, what)

    vi, ptr, vo = bufs(12)
    refused((BF16, ptr, vo.ptr, k, s, p, ho, wo, B, 12, H, W), vo, "C = 12")
    vi, ptr, vo = bufs(8, off_in=8)
    refused((BF16, ptr, vo.ptr, k, s, p, ho, wo, B, 8, H, W), vo, "input 8 bytes off")
    vi, ptr, vo = bufs(8, off_out=8)
    refused((BF16, ptr, vo.ptr, k, s, p, ho, wo, B, 8, H, W), vo, "output 8 bytes off")
    vi, ptr, vo = bufs(8)
    refused((BF16, ptr, ptr, k, s, p, ho, wo, B, 8, H, W), vo, "inp == out")
    refused((7, ptr, vo.ptr, k, s, p, ho, wo, B, 8, H, W), vo, "unknown dtype")
    assert fn(ctx.handle, BF16, None, None, k, s, p, ho, wo, 0, 8, H, W) == L.RN_OK
    # and the same buffers are accepted once the call is right
    assert fn(ctx.handle, BF16, ptr, vo.ptr, k, s, p, ho, wo, B, 8, H, W) == L.RN_OK
    ctx.sync()
    assert not np.isnan(ops.from_bf16_bits(V.fetch(vo, np.uint16, "accepted"))).any()


F32_CASES = [(2, 8, 33, 4, 3, 2, 1),    # NHWC walk
             (1, 8, 6, 5, 3, 1, 1),     # maxpool3 / vector average
             (2, 6, 8, 6, 2, 2, 0),     # C % 4 != 0: the scalar kernel
             (3, 12, 7, 7, 7, 1, 0),    # global average
             (1, 4, 9, 8, 3, 2, 1)]


@pytest.mark.parametrize("is_max", [True, False])
@pytest.mark.parametrize("case", F32_CASES)
def test_f32_through_the_dt_entry_points(case, is_max):
    """RN_DTYPE_F32: the context's layout is saved, the call runs as rn_maxpool2d_forward / rn_avgpool2d_forward
    under NHWC (the same bits), and the layout is NCHW again afterwards -- after a refused call too."""
    B, C, H, W, k, s, p = case
    ctx, lib = R.get_ctx(), L.lib()
    x = rnd((B, C, H, W), 6300 + sum(case))
    ho, wo = V.out_size(H, k, s, p), V.out_size(W, k, s, p)
    want = (ops.maxpool2d if is_max else ops.avgpool2d)(x, k, s, p, "nhwc")
    assert np.array_equal(want, (O.maxpool2d if is_max else O.avgpool2d)(x, k, s, p))
    what = f"{entry(is_max)} f32 {case}"
    try:
        ctx.set_layout(L.RN_LAYOUT_NCHW)
        vi = V.place(np.ascontiguousarray(x.transpose(0, 2, 3, 1)), 0, fill="inf" if is_max else "nan")
        vo = V.place_out(B * ho * wo * C * 4)
        V.must(entry(is_max), F32, vi.ptr, vo.ptr, k, s, p, ho, wo, B, C, H, W)
        assert lib.rn_ctx_get_layout(ctx.handle) == L.RN_LAYOUT_NCHW
        V.check_guards(what, vi)
        got = V.fetch(vo, np.float32, what).reshape(B, ho, wo, C).transpose(0, 3, 1, 2)
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
        st, msg = V.call(entry(is_max), F32, vi.ptr, vi.ptr, k, s, p, ho, wo, B, C, H, W)
        assert st == L.RN_ERR_INVALID and msg
        assert lib.rn_ctx_get_layout(ctx.handle) == L.RN_LAYOUT_NCHW
        V.check_guards(what + " after the refusal", vi)
        assert np.array_equal(V.fetch(vo, np.float32, what + " after the refusal").reshape(B, ho, wo, C).transpose(0, 3, 1, 2), want)
    finally:
        ctx.set_layout(L.RN_LAYOUT_NCHW)
