"""Every bf16 epilogue against a float64 reference, element by element (tests/bf16_ref.py).

The bit-for-bit comparisons of test_bf16_gpu.py show that tile candidates, chains and strips agree with each
other; these show that the common answer is the correctly rounded one.  The reference is the float64 value of
the kernel's expression on the operands as the kernel sees them (bf16-rounded activations, weights and
residual, fp32 scale and shift); every element has to lie within half of ITS OWN bf16 step of it, plus the
fp32 accumulation bound of test_ops_gpu.py::assert_close (bf16_ref.assert_bf16_rounded).  Shapes are the
smallest the dispatch predicates accept; each says which predicate it satisfies.  Every comparison prints its
figures (largest error in steps of the element, eps_sum's share of the bound) for the record."""
import numpy as np
import pytest

import bf16_ref as BR
import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import ops

pytestmark = pytest.mark.gpu

rb = ops.bf16_round


def rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def record(part, what, m):
    print(f"\nbf16-rounding {part}: {what}: max error {m['max_err_steps']:.4f} steps, bound used {m['max_bound_used']:.3f}, "
          f"eps_sum {m['eps_sum']:.2e} = {100 * m['eps_share_median']:.2f} % of the median non-zero element's bound "
          f"({m['elements']} elements)")


class forced_tile:
    """rn_ctx_set_conv_tile(cand) for the block, 0 (the dispatcher's own choice) afterwards"""

    def __init__(self, cand):
        self.cand = cand

    def __enter__(self):
        L.check(L.lib().rn_ctx_set_conv_tile(R.get_ctx().handle, self.cand), "rn_ctx_set_conv_tile")

    def __exit__(self, *exc):
        L.lib().rn_ctx_set_conv_tile(R.get_ctx().handle, 0)


def bn_consts(C, seed):
    g = np.random.default_rng(seed)
    return g.random(C, dtype=np.float32) + np.float32(0.5), g.standard_normal(C, dtype=np.float32)


# ---- 1. rn_conv2d_nhwc_forward_dt, bf16 -> bf16 ---------------------------------------------------------------
# in_channels % 64 == 0 (rn_conv2d_nhwc_forward_dt); candidate 4 = the 4-wave kernel's 64x64 tile, one block per
# tile (launch_gemm: conv_tile 1..8); candidate 9 = the first 256-wide tile (rn_conv_wide_eligible: whole 128-byte
# channel segments, Cout % 8 == 0); the last candidate = the strip kernel (rn_conv_strip_eligible: 3x3 / stride 1 /
# pad 1, 64 -> 64 or 128 -> 128 channels, W + 3 within the ring margin).  A forced candidate whose predicate fails
# would fall through to the dispatcher's own choice, so "strip" is listed only where the predicate holds.
CONV_CASES = [
    ((2, 64, 64, 9, 9, 3, 1, 1), ("tile", "wide", "strip")),     # strip: 64 -> 64, K = 576; 162 rows: ragged M tiles
    ((1, 128, 128, 7, 6, 3, 1, 1), ("tile", "wide", "strip")),   # strip: 128 -> 128, K = 1152; 42 rows: one ragged tile
    ((2, 64, 72, 9, 7, 1, 2, 0), ("tile", "wide")),              # 1x1 stride 2, Cout = 72: ragged N tile, % 8 == 0
    ((1, 128, 64, 5, 5, 3, 1, 1), ("tile", "wide")),             # K = 1152 >= 1152, 25 rows: ragged M
]
FORMS = [("scale+shift+residual+relu", True, True, True, True), ("shift only", False, True, False, False),
         ("residual, no relu", False, False, True, False)]


def conv_operands(case):
    B, Cin, Cout, H, W, k, s, p = case
    seed = 3000 + sum(case)
    x, w = rnd((B, Cin, H, W), seed), rnd((Cout, Cin, k, k), seed + 1) / np.float32(np.sqrt(Cin * k * k))
    sc, sh = bn_consts(Cout, seed + 2)
    y64 = BR.conv64(rb(x), rb(w), s, p)
    res = rnd(y64.shape, seed + 3)
    return x, w, sc, sh, res, y64


def family_takes(fam, case):
    """The predicates of launch_gemm, rn_conv_wide_eligible and rn_conv_strip_eligible (kStripMargin = 64,
    kMargin2 = 32), restated: a forced candidate whose predicate fails is not an error, it runs candidate 0."""
    B, Cin, Cout, H, W, k, s, p = case
    if fam == "tile":
        return Cin % 64 == 0
    if fam == "wide":
        return Cin % 64 == 0 and Cout % 8 == 0
    return (k, s, p) == (3, 1, 1) and (((Cin, Cout) == (64, 64) and W + 3 <= 64) or ((Cin, Cout) == (128, 128) and W + 3 <= 32))


@pytest.mark.parametrize("case,families", CONV_CASES)
def test_conv_epilogue_is_correctly_rounded(case, families):
    B, Cin, Cout, H, W, k, s, p = case
    assert all(family_takes(fam, case) for fam in families) and ("strip" in families) == family_takes("strip", case)
    x, w, sc, sh, res, y64 = conv_operands(case)
    lib = L.lib()
    cands = {"tile": 4, "wide": 9, "strip": lib.rn_conv_tile_candidates()}
    assert cands["strip"] > 9
    for name, use_sc, use_sh, use_res, relu in FORMS:
        a_sc, a_sh, a_res = (sc if use_sc else None), (sh if use_sh else None), (res if use_res else None)
        ref = BR.epilogue64(y64, a_sc, a_sh, rb(res) if use_res else None, relu)
        own = ops.conv2d_nhwc_bf16(x, w, s, p, a_sc, a_sh, a_res, relu)     # candidate 0: the dispatcher's choice
        for fam in families:
            with forced_tile(cands[fam]):
                got = ops.conv2d_nhwc_bf16(x, w, s, p, a_sc, a_sh, a_res, relu)
            what = f"{case} candidate {cands[fam]} ({fam}) {name}"
            assert np.array_equal(got, own), what      # the k order per element does not depend on the candidate
            record("1 conv", what, BR.assert_bf16_rounded(got, ref, Cin * k * k, what))
    assert lib.rn_ctx_set_conv_tile(R.get_ctx().handle, 0) == L.RN_OK


# ---- 2. rn_conv2d_nhwc_pair_forward_dt ------------------------------------------------------------------------
# both channel counts % 64 == 0, one output size for both sources; 50 rows x 128 channels.  The scales are folded
# into the packed panel: the kernel multiplies bf16(fl32(w * scale)).
@pytest.mark.parametrize("stride2", [1, 2])
@pytest.mark.parametrize("with_res", [False, True])
def test_conv_pair_is_correctly_rounded(stride2, with_res):
    B, Cin, Cout, H, W, Cin2 = 2, 64, 128, 5, 5, 128
    H2 = H if stride2 == 1 else 2 * H - 1
    seed = 3300 + stride2
    K = Cin + Cin2
    t, x2 = rnd((B, Cin, H, W), seed), rnd((B, Cin2, H2, H2), seed + 1)
    w, w2 = rnd((Cout, Cin, 1, 1), seed + 2) / np.float32(np.sqrt(K)), rnd((Cout, Cin2, 1, 1), seed + 3) / np.float32(np.sqrt(K))
    sc1, shift = bn_consts(Cout, seed + 4)
    sc2, _ = bn_consts(Cout, seed + 5)
    res = rnd((B, Cout, H, W), seed + 6) if with_res else None
    w1b, w2b = rb(w * sc1[:, None, None, None]), rb(w2 * sc2[:, None, None, None])
    y64 = BR.conv64(rb(t), w1b, 1, 0) + BR.conv64(rb(x2), w2b, stride2, 0)
    ref = BR.epilogue64(y64, None, shift, rb(res) if with_res else None, True)
    for cand in (0, 4, 9):      # the dispatcher's choice, a 4-wave tile, the wide kernel's two-source form
        with forced_tile(cand):
            got = ops.conv2d_nhwc_pair(t, w, x2, w2, 1, 0, stride2, sc1, sc2, shift, res, True, bf16=True)
        what = f"pair stride2={stride2} residual={with_res} candidate {cand}"
        record("2 pair", what, BR.assert_bf16_rounded(got, ref, K, what))


# ---- 3. rn_conv_chain_forward_dt / rn_conv_chain_pair_forward_dt ----------------------------------------------
# chain_launch: 64 -> 256 -> 64 | 128 channels, or (bf16, one source) 128 -> 512 -> 128.  64 and 189 rows: one
# step, and a ragged last step of the 64- and 32-row walks, for every instantiation (one per next_mid).
@pytest.mark.parametrize("case", [(1, 8, 8, 64, 64), (3, 9, 7, 64, 64), (1, 8, 8, 64, 128), (3, 9, 7, 64, 128),
                                  (1, 8, 8, 128, 128), (3, 9, 7, 128, 128)])
def test_conv_chain_is_correctly_rounded(case):
    B, H, W, MID, N1 = case
    C = 4 * MID
    seed = 3500 + sum(case)
    t2, x = rnd((B, MID, H, W), seed), rnd((B, C, H, W), seed + 1)
    w3, w1 = rnd((C, MID, 1, 1), seed + 2) / np.float32(np.sqrt(MID)), rnd((N1, C, 1, 1), seed + 3) / np.float32(np.sqrt(C))
    sc3, sh3 = bn_consts(C, seed + 4)
    sc1, sh1 = bn_consts(N1, seed + 5)
    got_y, got_t1 = ops.conv_chain_bf16(t2, x, w3, sc3, sh3, w1, sc1, sh1)
    ref_y = BR.epilogue64(BR.conv64(rb(t2), rb(w3)), sc3, sh3, rb(x), True)
    record("3 chain", f"{case} y", BR.assert_bf16_rounded(got_y, ref_y, MID, f"chain {case} y"))
    # t1's operand is the y the kernel wrote (already bf16): not the code under test as its own reference for y
    assert np.array_equal(got_y, rb(got_y))
    ref_t1 = BR.epilogue64(BR.conv64(got_y, rb(w1)), sc1, sh1, None, True)
    record("3 chain", f"{case} t1", BR.assert_bf16_rounded(got_t1, ref_t1, C, f"chain {case} t1"))


@pytest.mark.parametrize("case", [(1, 8, 8, 64), (3, 9, 7, 128), (3, 9, 7, 64), (1, 8, 8, 128)])
def test_conv_chain_pair_is_correctly_rounded(case):
    B, H, W, N1 = case
    seed = 3700 + sum(case)
    t2, x2 = rnd((B, 64, H, W), seed), rnd((B, 64, H, W), seed + 1)
    w3, wd = rnd((256, 64, 1, 1), seed + 2) / np.float32(np.sqrt(128)), rnd((256, 64, 1, 1), seed + 3) / np.float32(np.sqrt(128))
    w1 = rnd((N1, 256, 1, 1), seed + 4) / np.float32(16)
    sc3, shift = bn_consts(256, seed + 5)
    scd, _ = bn_consts(256, seed + 6)
    sc1, sh1 = bn_consts(N1, seed + 7)
    got_y, got_t1 = ops.conv_chain_pair_bf16(t2, x2, w3, sc3, wd, scd, shift, w1, sc1, sh1)
    w3b, wdb = rb(w3 * sc3[:, None, None, None]), rb(wd * scd[:, None, None, None])
    ref_y = BR.epilogue64(BR.conv64(rb(t2), w3b) + BR.conv64(rb(x2), wdb), None, shift, None, True)
    record("3 chain pair", f"{case} y", BR.assert_bf16_rounded(got_y, ref_y, 128, f"chain pair {case} y"))
    assert np.array_equal(got_y, rb(got_y))
    ref_t1 = BR.epilogue64(BR.conv64(got_y, rb(w1)), sc1, sh1, None, True)
    record("3 chain pair", f"{case} t1", BR.assert_bf16_rounded(got_t1, ref_t1, 256, f"chain pair {case} t1"))


# ---- 4. rn_stem_pool_forward_dt / rn_stem_pool_nchw_forward_dt ------------------------------------------------
# stem_pool_launch: 1..3 input channels, conv output width % 8 == 0 (16 and 24), the NCHW form an image width
# % 4 == 0, the padded form an even padded width; the second shape has an odd height and two channels.  Rounding
# is monotone, so the pooled maximum of the rounded stem values is the rounded pooled maximum.
@pytest.mark.parametrize("from_nchw", [False, True])
@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (1, 2, 23, 48)])
def test_stem_pool_is_correctly_rounded(shape, from_nchw):
    B, Cin, H, W = shape
    seed = 3900 + sum(shape)
    x, w = rb(rnd(shape, seed)), rb(rnd((64, Cin, 7, 7), seed + 1) / np.float32(np.sqrt(Cin * 49)))
    sc, sh = bn_consts(64, seed + 2)
    sh = sh * np.float32(0.3)
    ref = BR.maxpool64(BR.epilogue64(BR.conv64(x, w, 2, 3), sc, sh, None, True), 3, 2, 1)
    got = ops.stem_pool(x, w, sc, sh, True, bf16=True, from_nchw=from_nchw)
    what = f"stem + pool {shape} from_nchw={from_nchw}"
    record("4 stem", what, BR.assert_bf16_rounded(got, ref, Cin * 49, what))


# ---- 5. rn_conv2d_grouped_nhwc_forward_dt, bf16 ---------------------------------------------------------------
# 128 channels in 32 groups (4 per group, the networks' smallest super-group shape), the planes of
# test_grouped_gpu.py; the bf16 route is the dense contraction on a panel that is zero outside the groups, so a
# wrong zero fill shows as foreign products in the sum.
@pytest.mark.parametrize("plane", [(2, 6, 7), (3, 1, 9)])
@pytest.mark.parametrize("stride", [1, 2])
def test_grouped_conv_epilogue_is_correctly_rounded(plane, stride):
    C, G = 128, 32
    B, H, W = plane
    seed = 4100 + sum(plane) + stride
    x, w = rnd((B, C, H, W), seed), rnd((C, C // G, 3, 3), seed + 1) / np.float32(np.sqrt(9 * C // G))
    sc, sh = bn_consts(C, seed + 2)
    y64 = BR.conv64(rb(x), rb(w), stride, 1, groups=G)
    res = rnd(y64.shape, seed + 3)
    for name, a_sc, a_sh, a_res, relu in (("scale+shift+residual+relu", sc, sh, res, True), ("shift only", None, sh, None, False),
                                          ("residual, no relu", None, None, res, False)):
        ref = BR.epilogue64(y64, a_sc, a_sh, rb(res) if a_res is not None else None, relu)
        got = ops.conv2d_grouped_nhwc_bf16(x, w, stride, 1, G, a_sc, a_sh, a_res, relu)
        what = f"grouped {plane} stride {stride} {name}"
        record("5 grouped", what, BR.assert_bf16_rounded(got, ref, 9 * C // G, what))


# ---- 6. bf16 -> fp32 with bias (the fc of a bf16 model) -------------------------------------------------------
def test_fc_form_with_bias_against_float64():
    """No rounding of the result: the fp32 accumulation bound of test_ops_gpu.py::assert_close, against conv64
    instead of the fp32 oracle.  K = 2048 = 32 K tiles: the chunked sum (launch_gemm: bf16 in, fp32 out, nk >= 32)."""
    B, K, N = 3, 2048, 40
    x, w = rnd((B, K, 1, 1), 4300), rnd((N, K, 1, 1), 4301) / np.float32(np.sqrt(K))
    bias = rnd((N,), 4302)
    ref = BR.epilogue64(BR.conv64(rb(x), rb(w)), None, bias, None, False)
    got = ops.conv2d_nhwc_bf16(x, w, 1, 0, None, bias, None, False, out_f32=True)
    tol = BR.eps_sum(ref, K)
    err = float(np.abs(got - ref).max())
    print(f"\nbf16-rounding 6 fc: max error {err:.3e}, bound {tol:.3e}")
    assert got.shape == ref.shape and err <= tol
