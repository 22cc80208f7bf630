"""RoIAlign over the pyramid on the GPU: the launch on views between guard bands against the fp32 statement of its
contract (ops.roi_align_ref) bit for bit, and the pooler behind the neck and the model against the same launch on
the levels the same call returns, and against the float64 reference on the neck's float64 reference.

Bit equality is what is asked wherever the device and the host state the same fp32 operations; the float64
comparisons use the FPN tests' bounds for the levels plus the contract's own bound (test_roi_host.py derives it).
"""
import ctypes

import numpy as np
import pytest

import resnet_c_amd as R
import views as V
from resnet_c_amd import _lib as L
from resnet_c_amd import fpn as P
from resnet_c_amd import ops, preprocess
from resnet_c_amd import roi as RO
from resnet_c_amd import weights as W
from test_dilation_gpu import bits, tol_bf16, tol_f32
from test_fpn_gpu import MB, SIZE, WIDTH, images, launches, model_neck_state, nets  # noqa: F401  (nets: a fixture)
from test_fpn_host import products
from test_roi_host import U, sample_coords

pytestmark = pytest.mark.gpu

DT = {"f32": L.RN_DTYPE_F32, "bf16": L.RN_DTYPE_BF16}
NAME = "rn_roi_align_forward_dt"
FP = ctypes.POINTER(ctypes.c_float)


def typed_map(shape, dtype, seed):
    a = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    return a if dtype == "f32" else ops.to_bf16_bits(a).reshape(shape)


def make_rois(h, w, B, scale=0.25, n=48, seed=3):
    """n random boxes that reach outside the image, the four special boxes of the host test's kind, and boxes whose
    samples land on integers, on -1, on h and on h - 1 (7 bins of one pixel, S = 1: the samples are the integers)"""
    rng = np.random.default_rng(seed + 31 * h + w)
    H, Wd = h / scale, w / scale
    cx, cy = rng.uniform(-8, Wd + 8, n), rng.uniform(-8, H + 8, n)
    bw, bh = rng.uniform(0.5, 1.5 * Wd + 4, n), rng.uniform(0.5, 1.5 * H + 4, n)
    r = np.stack([rng.integers(0, B, n).astype(np.float64), cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], axis=1)
    special = [[0, 20 * Wd, 20 * H, 21 * Wd, 21 * H], [B - 1, 0.3 * Wd, 0.4 * H, 0.3 * Wd, 0.4 * H],
               [0, 0.5 * Wd, 0.5 * H, 0.5 * Wd + 0.3, 0.5 * H + 0.2], [B - 1, -Wd, -H, 2 * Wd, 2 * H]]
    exact = [[0, -6, -6, 22, 22], [B - 1, -10, -10, 18, 18],                                  # samples -1, 0, .. / -2, -1, ..
             [0, 4 * w - 26, 4 * h - 26, 4 * w + 2, 4 * h + 2],                               # .. h - 1, h
             [B - 1, 4 * w - 22, 4 * h - 22, 4 * w + 6, 4 * h + 6], [0, 0, 0, 4 * w, 4 * h], [B - 1, 4, 4, 8, 8]]
    return np.concatenate([r, np.array(special, np.float64), np.array(exact, np.float64)]).astype(np.float32)


def run_roi(maps, rois, scales, thr, P_, S, aligned, dtype, out_off=0, want_levels=True, B=None):
    """one launch on views between guard bands: input guards intact, the output written everywhere"""
    n, C = len(maps), maps[0].shape[3]
    B = maps[0].shape[0] if B is None else B
    K = rois.shape[0]
    vm = [V.place(m) for m in maps]
    vr = V.place(np.ascontiguousarray(rois, dtype=np.float32))
    vo = V.place_out(K * C * P_[0] * P_[1] * 4, out_off)
    vl = V.place_out(K * 4) if want_levels else None
    sc = np.ascontiguousarray(scales, dtype=np.float32)
    th = np.concatenate([np.asarray(thr, np.float32).reshape(-1), np.zeros(1, np.float32)])
    before = launches()
    V.must(NAME, DT[dtype], n, (ctypes.c_void_p * n)(*[v.ptr for v in vm]), (ctypes.c_uint64 * n)(*[m.shape[1] for m in maps]),
           (ctypes.c_uint64 * n)(*[m.shape[2] for m in maps]), sc.ctypes.data_as(FP), th.ctypes.data_as(FP), B, C, vr.ptr, K,
           P_[0], P_[1], S, int(aligned), vo.ptr, vl.ptr if vl else None)
    assert launches() == before + 1
    V.check_guards(f"{NAME} inputs", vr, *vm)
    what = f"{NAME} {dtype} C={C} {P_} S={S} aligned={aligned} +{out_off}"
    out = V.fetch(vo, np.float32, what, written=True).reshape(K, C, P_[0], P_[1])
    return (out, V.fetch(vl, np.int32, what + " levels", written=True)) if want_levels else out


# =====================================================================================================================
# 1. the launch alone
# =====================================================================================================================
@pytest.mark.parametrize("hw", [(13, 17), (2, 3), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_op_is_the_contract_bit_for_bit(dtype, hw):
    h, w = hw
    B = 2
    rois = make_rois(h, w, B)
    for C in ((4, 64) if dtype == "f32" else (8, 64)):
        m = typed_map((B, h, w, C), dtype, seed=C + h)
        for P_ in ((7, 7), (14, 14), (3, 5)):
            for S in (1, 2, 3):
                for aligned in (False, True):
                    want = ops.roi_align_ref([m], rois, [0.25], P_, S, aligned)
                    V.assert_no_poison(want, False, "reference")
                    got, lv = run_roi([m], rois, [0.25], [], P_, S, aligned, dtype)
                    assert np.array_equal(bits(got), bits(want)), (C, P_, S, aligned)
                    assert not lv.any()
    if hw == (13, 17) and dtype == "f32":      # S = 4, the largest grid, and the largest output
        for P_, S in (((7, 7), 4), ((32, 32), 2), ((1, 1), 1), ((32, 1), 1)):
            m = typed_map((B, h, w, 8), dtype, seed=77)
            assert np.array_equal(bits(run_roi([m], rois, [0.25], [], P_, S, True, dtype, want_levels=False)),
                                  bits(ops.roi_align_ref([m], rois, [0.25], P_, S, True))), (P_, S)


def test_op_destination_off_a_16_byte_boundary():
    """out 4, 8 and 12 bytes off: every element written, no guard byte touched, the same bits"""
    B, h, w = 2, 5, 6
    rois = make_rois(h, w, B, n=9)
    for dtype, C in (("f32", 4), ("f32", 72), ("bf16", 8)):
        m = typed_map((B, h, w, C), dtype, seed=C)
        for P_ in ((7, 7), (3, 5), (1, 1)):
            want = ops.roi_align_ref([m], rois, [0.25], P_, 2, False)
            V.assert_no_poison(want, False, "reference")
            for off in (0, 4, 8, 12):
                got = run_roi([m], rois, [0.25], [], P_, 2, False, dtype, out_off=off, want_levels=False)
                assert np.array_equal(bits(got), bits(want)), (dtype, C, P_, off)


def test_op_more_than_one_block_each_way():
    """more RoIs than the grid has rows (the RoIs stride), C = 320 (five slabs of 64 channels) and 72 (a slab and a
    rest of two chunks), K = 0"""
    B, h, w = 2, 4, 5
    few = make_rois(h, w, B, n=20)
    many = np.tile(few, (65535 // len(few) + 2, 1))
    assert len(many) > 65535 + len(few)
    m = typed_map((B, h, w, 4), "f32", seed=1)
    got = run_roi([m], many, [0.25], [], (1, 2), 1, False, "f32", want_levels=False)
    want = np.tile(ops.roi_align_ref([m], few, [0.25], (1, 2), 1, False), (len(many) // len(few), 1, 1, 1))
    assert np.array_equal(bits(got), bits(want))
    for dtype, C in (("f32", 320), ("f32", 72), ("bf16", 320), ("bf16", 72)):
        m = typed_map((B, h, w, C), dtype, seed=C)
        for P_ in ((7, 7), (14, 14)):
            got = run_roi([m], few, [0.25], [], P_, 2, True, dtype, want_levels=False)
            assert np.array_equal(bits(got), bits(ops.roi_align_ref([m], few, [0.25], P_, 2, True))), (dtype, C, P_)
    vm, vo = V.place(typed_map((B, h, w, 4), "f32", 1)), V.place_out(64)
    sc = np.array([0.25], np.float32)
    before = launches()
    for K, Bn in ((0, B), (3, 0)):
        V.must(NAME, L.RN_DTYPE_F32, 1, (ctypes.c_void_p * 1)(vm.ptr), (ctypes.c_uint64 * 1)(h), (ctypes.c_uint64 * 1)(w),
               sc.ctypes.data_as(FP), None, Bn, 4, None, K, 7, 7, 2, 0, vo.ptr, None)
    assert launches() == before
    V.assert_untouched(vo, "K == 0 and B == 0")


PYRAMID = ((16, 20), (8, 10), (4, 5), (2, 3))
SCALES = (1 / 4, 1 / 8, 1 / 16, 1 / 32)


def pyramid_rois(B, thr):
    """boxes of every level, and boxes whose area is each threshold, the fp32 value below it and the one above"""
    rng = np.random.default_rng(8)
    n = 40
    side = 2.0 ** rng.uniform(2, 10, n)
    x1, y1 = rng.uniform(-10, 70, n), rng.uniform(-10, 50, n)
    r = [np.stack([rng.integers(0, B, n).astype(np.float64), x1, y1, x1 + side, y1 + side * rng.uniform(0.5, 2, n)], axis=1)]
    edge = []
    for t in thr:
        for a in (np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(np.inf))):
            edge.append([len(edge) % B, 0.0, 0.0, 1.0, float(a)])                # area = 1 * a, exact in fp32
    return np.concatenate(r + [np.array(edge)]).astype(np.float32)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_four_levels_in_one_launch(dtype):
    B, C = 2, 16
    maps = [typed_map((B, h, w, C), dtype, seed=h) for h, w in PYRAMID]
    thr = ops.roi_level_thresholds(SCALES)
    rois = pyramid_rois(B, thr)
    want_lv = ops.roi_levels_ref(rois, thr)
    assert set(want_lv.tolist()) == {0, 1, 2, 3}
    assert want_lv[-9:].tolist() == [0, 1, 1, 1, 2, 2, 2, 3, 3]               # below, on and above each threshold
    for P_, S, aligned in (((7, 7), 2, False), ((3, 5), 3, True)):
        got, lv = run_roi(maps, rois, SCALES, thr, P_, S, aligned, dtype)
        assert np.array_equal(lv, want_lv)
        assert np.array_equal(bits(got), bits(ops.roi_align_ref(maps, rois, SCALES, P_, S, aligned, thr)))
        for i in range(4):                                                    # every row is the single-level launch's
            alone = run_roi([maps[i]], rois, [SCALES[i]], [], P_, S, aligned, dtype, want_levels=False)
            assert np.array_equal(bits(got[want_lv == i]), bits(alone[want_lv == i])), i
    # fewer levels: two and three, from another stride; another canonical box moves the thresholds
    two = run_roi(maps[1:3], rois, SCALES[1:3], ops.roi_level_thresholds(SCALES[1:3]), (7, 7), 2, False, dtype)[1]
    assert np.array_equal(two, np.clip(want_lv, 1, 2) - 1)
    thr2 = ops.roi_level_thresholds(SCALES[:3], 32.0, 4)
    three, lv3 = run_roi(maps[:3], rois, SCALES[:3], thr2, (7, 7), 2, False, dtype)
    assert np.array_equal(lv3, ops.roi_levels_ref(rois, thr2)) and len(set(lv3.tolist())) == 3
    assert np.array_equal(bits(three), bits(ops.roi_align_ref(maps[:3], rois, SCALES[:3], (7, 7), 2, False, thr2)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_hostile_rois(dtype):
    """NaN, infinite and huge coordinates index nothing outside the maps (the clamps are unconditional: every guard
    stays intact, every value is the contract's); an image index that is no integer in [0, B) gives zeros and -1"""
    B, C = 2, 16
    maps = [typed_map((B, h, w, C), dtype, seed=h + 1) for h, w in PYRAMID]
    thr = ops.roi_level_thresholds(SCALES)
    nan, inf, big = np.nan, np.inf, 1e30
    rois = np.array([[0, nan, 1, 9, 9], [1, 1, nan, 9, 9], [0, 1, 1, nan, 9], [1, nan, nan, nan, nan],
                     [0, -inf, 1, 9, 9], [1, 1, 1, inf, 9], [0, -inf, -inf, inf, inf], [1, inf, inf, inf, inf],
                     [0, -big, -big, big, big], [1, big, big, 2 * big, 2 * big], [0, -big, 3, 9, 20], [1, 3, 4, big, 20],
                     [0, 9, 9, 1, 1], [1, 3e9, 3e9, 3.1e9, 3.1e9], [0, -3e9, -3e9, 5, 5],
                     [-1, 1, 1, 9, 9], [B, 1, 1, 9, 9], [0.5, 1, 1, 9, 9], [nan, 1, 1, 9, 9], [inf, 1, 1, 9, 9],
                     [-0.0, 1, 1, 9, 9], [1e10, 1, 1, 9, 9], [3e38, 1, 1, 9, 9], [1, 1, 1, 9, 9]], dtype=np.float32)
    for P_, S, aligned in (((7, 7), 2, False), ((7, 7), 2, True), ((2, 3), 1, False)):
        want, want_lv = ops.roi_align_ref(maps, rois, SCALES, P_, S, aligned, thr, return_levels=True)
        got, lv = run_roi(maps, rois, SCALES, thr, P_, S, aligned, dtype)
        assert np.array_equal(lv, want_lv) and lv[15:20].tolist() == [-1] * 5 and lv[20] >= 0 and lv[21:23].tolist() == [-1, -1]
        assert np.array_equal(bits(got), bits(want)), (P_, S, aligned)
        assert not got[15:20].any() and not got[21:23].any()          # invalid images: zeros
        assert not got[3].any() and not got[7].any()                  # no coordinate contributes: zeros
        assert got[20].any() and got[23].any()
        assert np.isfinite(got).all()


def test_op_refusals_launch_nothing():
    lib, ctx = L.lib(), R.get_ctx()
    B, h, w, C, K = 2, 4, 5, 8, 3
    vm = [V.place(np.ones((B, h, w, C), np.float32)), V.place(np.ones((B, 2, 3, C), np.float32))]
    vr = V.place(np.array([[0, 1, 1, 9, 9]] * K, np.float32))
    vo, vl = V.place_out(K * C * 49 * 4), V.place_out(K * 4)
    big = V.place(np.ones(B * h * w * C + K * C * 49, np.float32))
    ptrs = lambda *p: (ctypes.c_void_p * len(p))(*p)      # noqa: E731
    u64s = lambda *v: (ctypes.c_uint64 * len(v))(*v)      # noqa: E731
    f32s = lambda *v: np.array(v, np.float32).ctypes.data_as(FP)  # noqa: E731
    keep = [np.array([0.25, 0.125], np.float32), np.array([100.0, 0.0], np.float32)]
    good = dict(dtype=L.RN_DTYPE_F32, n=2, maps=ptrs(vm[0].ptr, vm[1].ptr), h=u64s(h, 2), w=u64s(w, 3),
                scales=keep[0].ctypes.data_as(FP), thr=keep[1].ctypes.data_as(FP), B=B, C=C, rois=vr.ptr, K=K, PH=7, PW=7, S=2,
                aligned=0, out=vo.ptr, levels=vl.ptr)

    def but(**kw):
        return tuple(kw.get(k, v) for k, v in good.items())

    bad_scale = [np.array(v, np.float32) for v in ([0.25, 0.0], [np.nan, 0.125], [np.inf, 0.125], [-0.25, 0.125])]
    cases = [(but(dtype=7), "dtype"), (but(n=0), "n_levels"), (but(n=5), "n_levels"), (but(maps=None), "NULL"), (but(h=None), "NULL"),
             (but(w=None), "NULL"), (but(scales=None), "NULL"), (but(thr=None), "thr"), (but(maps=ptrs(vm[0].ptr, None)), "map is NULL"),
             (but(maps=ptrs(vm[0].ptr + 4, vm[1].ptr)), "16-byte"), (but(rois=None), "rois_dev"), (but(out=None), "out is NULL"),
             (but(rois=vr.ptr + 2), "rois_dev"), (but(out=vo.ptr + 2), "out is off"), (but(levels=vl.ptr + 2), "levels_out"),
             (but(C=6), "C must"), (but(C=0), "C must"), (but(dtype=L.RN_DTYPE_BF16, C=12), "C must"), (but(C=1 << 31), "C must"),
             (but(PH=0), "1..32"), (but(PW=33), "1..32"), (but(S=5), "1..4"), (but(aligned=2), "aligned"),
             (but(h=u64s(0, 2)), ">= 1"), (but(w=u64s(w, 1 << 31)), "2^31"), (but(B=1 << 31), "2^31"), (but(K=1 << 31), "2^31"),
             (but(h=u64s(1 << 16, 2), w=u64s(1 << 16, 3)), "2^31"),
             (but(maps=ptrs(big.ptr, vm[1].ptr), out=big.ptr + 16), "overlaps a level"), (but(out=vr.ptr), "overlaps rois"),
             (but(levels=vr.ptr), "levels_out overlaps"), (but(levels=vo.ptr + 16), "levels_out overlaps"),
             (but(maps=ptrs(vm[0].ptr, vl.ptr)), "levels_out overlaps")]
    cases += [(but(scales=s.ctypes.data_as(FP)), "scale") for s in bad_scale]
    before = launches()
    for args, word in cases:
        st, msg = V.call(NAME, *args)
        assert st == L.RN_ERR_INVALID and word in msg and NAME in msg, (word, st, msg)
    for s in (0, -1):
        st, msg = V.call(NAME, *but(S=s))
        assert st == L.RN_ERR_UNSUPPORTED and "adaptive" in msg, (st, msg)
    assert lib.rn_roi_align_forward_dt(None, *but()) == L.RN_ERR_INVALID
    assert launches() == before
    ctx.sync()
    for v in (vo, vl, big):
        V.assert_untouched(v, "refused calls")
    V.must(NAME, *but())                                  # and the call they all almost were
    assert launches() == before + 1
    V.fetch(vo, np.float32, "the good call", written=True), V.fetch(vl, np.int32, "the good call", written=True)


def test_python_wrappers():
    B = 2
    maps = [typed_map((B, h, w, 8), "f32", seed=h) for h, w in PYRAMID]
    thr = ops.roi_level_thresholds(SCALES)
    rois = pyramid_rois(B, thr)
    got, lv = ops.roi_align(maps, rois, SCALES, 7, return_levels=True)
    want, want_lv = ops.roi_align_ref(maps, rois, SCALES, 7, return_levels=True)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(lv, want_lv)
    mb = [ops.to_bf16_bits(m).reshape(m.shape) for m in maps]
    assert np.array_equal(bits(ops.roi_align_bf16(mb, rois, SCALES, (3, 5), 3, True)),
                          bits(ops.roi_align_ref(mb, rois, SCALES, (3, 5), 3, True)))
    bad = rois.copy()
    bad[3, 0] = B
    with pytest.raises(ValueError):
        ops.roi_align(maps, bad, SCALES, 7)
    pooler = R.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    feats = {str(i): np.ascontiguousarray(m.transpose(0, 3, 1, 2)) for i, m in enumerate(maps)}
    boxes = [rois[rois[:, 0] == b, 1:] for b in range(B)]
    by_image = pooler(feats, boxes, (64, 80))
    order = np.concatenate([np.flatnonzero(rois[:, 0] == b) for b in range(B)])
    assert np.array_equal(bits(by_image), bits(want[order]))


# =====================================================================================================================
# 2. the pooler behind the neck and the model
# =====================================================================================================================
def pooler_for(names=("0", "1", "2", "3"), P_=7, S=2, aligned=False):
    """a canonical box of 16 pixels at level 4 spreads the boxes of a 72 x 40 image over all four levels"""
    return R.MultiScaleRoIAlign(names, P_, S, canonical_scale=16.0, canonical_level=4, aligned=aligned)


def image_rois(B, size, n=40, invalid=False, seed=17):
    """boxes of all images interleaved; invalid: a few rows whose image index names no image"""
    rng = np.random.default_rng(seed + B)
    side = 2.0 ** rng.uniform(1.5, 6, n)
    x1, y1 = rng.uniform(-4, size[1], n), rng.uniform(-4, size[0], n)
    r = np.stack([(np.arange(n) * 7 % B).astype(np.float64), x1, y1, x1 + side, y1 + side * rng.uniform(0.6, 1.6, n)], axis=1)
    r = r.astype(np.float32)
    if invalid:
        r[[2, 11, 29], 0] = [B, -1, 0.5]
    return r


def pooled_like_the_launch(out, names, rois, pooler, size):
    """ops.roi_align on the levels a forward returned (NCHW, transposed here)"""
    maps = [np.ascontiguousarray(out[k].transpose(0, 2, 3, 1)) for k in names]
    scales = RO.infer_scales([m.shape[1:3] for m in maps], size)
    ok = ops.roi_image_valid(rois, maps[0].shape[0])
    want = np.zeros((len(rois), maps[0].shape[3]) + pooler.output_size, np.float32)
    lv = np.full(len(rois), -1, np.int32)
    want[ok], lv[ok] = ops.roi_align(maps, rois[ok], scales, pooler.output_size, pooler.sampling_ratio, pooler.aligned,
                                     pooler.thresholds(scales), return_levels=True)
    return want, lv


def check_pooled_against_f64(pooled, levels, ref, names, rois, pooler, size, cin, a, dtype, what):
    """within the FPN tests' bound for the RoI's level (a bin is an average of level values with weights that sum to at
    most one) plus the contract's own bound (test_roi_host.py)"""
    maps = [ref[k] for k in names]
    scales = RO.infer_scales([m.shape[2:] for m in maps], size)
    want = RO.roi_align_f64(maps, rois, scales, pooler.output_size, pooler.sampling_ratio, pooler.aligned, levels=levels)
    worst = 0.0
    for r in range(len(rois)):
        i = int(levels[r])
        lvl = int(names[i])
        tol = tol_f32(maps[i], products(cin, a, lvl)) if dtype == "f32" else tol_bf16(maps[i])
        A = sample_coords(rois[r].astype(np.float64), scales[i], pooler.output_size, pooler.sampling_ratio, pooler.aligned)[2]
        tol += float(np.abs(maps[i]).max()) * (64 * U * A + 20 * U)
        err = float(np.abs(pooled[r] - want[r]).max())
        worst = max(worst, err / tol)
        assert err <= tol, (what, r, i, err, tol)
    print(f"\n  roi {what} {dtype}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_model_pooled(nets, arch, dtype):
    m, neck = nets(arch, dtype)
    x, rois, pooler = images(), image_rois(MB, SIZE), pooler_for()
    plain = m.forward_fpn(x, neck, logits=True)
    got = m.forward_fpn(x, neck, logits=True, rois=rois, pooler=pooler, roi_levels=True)
    assert list(got) == list(plain) + ["pooled", "roi_levels"]
    assert all(np.array_equal(bits(got[k]), bits(plain[k])) for k in plain)           # the other outputs keep their bits
    want, lv = pooled_like_the_launch(got, pooler.featmap_names, rois, pooler, SIZE)
    assert got["pooled"].shape == (len(rois), WIDTH[arch], 7, 7) and np.array_equal(got["roi_levels"], lv)
    assert set(lv.tolist()) == {0, 1, 2, 3}
    assert np.array_equal(bits(got["pooled"]), bits(want))
    maps = m.forward_maps(x)
    ref = P.fpn_ref([maps[s].astype(np.float64) for s in m.STAGES], model_neck_state(arch), "pool",
                    round_fn=ops.bf16_round if dtype == "bf16" else None)
    check_pooled_against_f64(got["pooled"], lv, ref, pooler.featmap_names, rois, pooler, SIZE, neck.in_channels_list,
                             neck.out_channels, dtype, f"{arch} model")
    # no level exported: the 3x3 of every level the pooler reads still runs; and a pooler of two levels, 14 x 14, aligned
    only = m.forward_fpn(x, neck, levels=(), rois=rois, pooler=pooler)
    assert list(only) == ["pooled"] and np.array_equal(bits(only["pooled"]), bits(want))
    p2 = pooler_for(("1", "2"), 14, 2, True)
    some = m.forward_fpn(x, neck, levels=("0",), rois=rois, pooler=p2, roi_levels=True)
    want2, lv2 = pooled_like_the_launch(plain, p2.featmap_names, rois, p2, SIZE)
    assert list(some) == ["0", "pooled", "roi_levels"] and np.array_equal(some["roi_levels"], lv2)
    assert np.array_equal(bits(some["pooled"]), bits(want2)) and np.array_equal(bits(some["0"]), bits(plain["0"]))
    # the byte route
    px = np.random.default_rng(9).integers(0, 256, (MB,) + SIZE + (3,), dtype=np.uint8)
    a = m.forward_fpn_u8(px, neck, rois=rois, pooler=pooler, roi_levels=True)
    b = m.forward_fpn(preprocess.normalize_u8(px), neck, rois=rois, pooler=pooler, roi_levels=True)
    assert list(a) == list(b) and all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_neck_pooled(dtype):
    from test_fpn_host import NECKS, neck_maps, neck_state
    cin, a, extra = NECKS["four"]
    neck = P.FeaturePyramidNetwork(cin, a, neck_state("four"), extra=extra, dtype=dtype)
    try:
        maps = neck_maps("four")
        B = maps[0].shape[0]
        nhwc = [np.ascontiguousarray(m.transpose(0, 2, 3, 1)) for m in maps]
        rois, pooler = image_rois(B, SIZE, invalid=True), pooler_for(("0", "1", "2", "3"), (3, 5), 3, True)
        with pytest.raises(ValueError):
            neck.forward(nhwc, rois=rois, pooler=pooler, image_size=SIZE)                 # host RoIs are checked
        plain = neck.forward(nhwc)
        got = neck.forward(nhwc, rois=rois, pooler=pooler, image_size=SIZE, roi_levels=True, validate=False)
        assert all(np.array_equal(bits(got[k]), bits(plain[k])) for k in plain)
        want, lv = pooled_like_the_launch(plain, pooler.featmap_names, rois, pooler, SIZE)
        assert np.array_equal(got["roi_levels"], lv) and lv[[2, 11, 29]].tolist() == [-1, -1, -1]
        assert np.array_equal(bits(got["pooled"]), bits(want)) and not got["pooled"][[2, 11, 29]].any()
        ok = lv >= 0
        ref = P.fpn_ref([m.astype(np.float64) for m in maps], neck_state("four"), extra,
                        round_fn=ops.bf16_round if dtype == "bf16" else None)
        check_pooled_against_f64(got["pooled"][ok], lv[ok], ref, pooler.featmap_names, rois[ok], pooler, SIZE, cin, a, dtype,
                                 "neck alone")
        only = neck.forward(nhwc, levels=(), rois=rois[ok], pooler=pooler, image_size=SIZE)
        assert list(only) == ["pooled"] and np.array_equal(bits(only["pooled"]), bits(want[ok]))
        with pytest.raises(ValueError):
            neck.forward(nhwc, rois=rois[ok], pooler=pooler_for(("0", "pool")), image_size=SIZE)
    finally:
        neck.close()


def poisoned_forward_rois(m, neck, x, rois, pooler, size, levels=()):
    """rn_model_forward_rois with `pooled` and `levels_out` as 0xA5-filled views between guard bands (and, for the
    names in `levels`, the exported levels likewise): every guard intact, every element written by the forward"""
    lib = L.lib()
    B, K, a = x.shape[0], len(rois), neck.out_channels
    PH, PW = pooler.output_size
    dx, dr = ops._up_raw(np.ascontiguousarray(x, dtype=np.float32)), ops._up_raw(np.ascontiguousarray(rois, dtype=np.float32))
    vp, vl = V.place_out(K * a * PH * PW * 4), V.place_out(K * 4)
    fo, views, shapes = L.FpnOutputs(), {}, {}
    for i, name in enumerate(neck.names):
        if name in levels:
            _, h, w = m.stage_shapes[m.STAGES[min(i, 3)]]
            shapes[name] = (B,) + neck.level_shape(name, h, w)
            views[name] = V.place_out(int(np.prod(shapes[name])) * 4)
            fo.level[i] = views[name].ptr
    req = pooler.request(neck.names, dr.ptr, K, size, vp.ptr, vl.ptr)
    st = lib.rn_model_forward_rois(m.handle, neck.handle, dx.ptr, B, None, (ctypes.c_int * 4)(1, 2, 3, 4), ctypes.byref(fo),
                                   ctypes.byref(req), L.RN_FWD_FUSED)
    assert st == L.RN_OK, (lib.rn_last_error(m.ctx.handle) or b"").decode()
    m.ctx.sync()
    out = {k: V.fetch(v, np.float32, f"level {k}", written=True).reshape(shapes[k]) for k, v in views.items()}
    out["pooled"] = V.fetch(vp, np.float32, "pooled", written=True).reshape(K, a, PH, PW)
    out["roi_levels"] = V.fetch(vl, np.int32, "roi_levels", written=True)
    return out


def test_model_parts_on_two_streams_and_two_sub_batches(nets):
    """Every row is written by the part that holds its image, the rows of an invalid image index by the first part:
    128 images as two parts on two streams, then one image more than a launch batch holds.  `pooled` and `levels_out`
    are the caller's buffers here, filled with 0xA5 between guard bands before every forward, so a row that no part
    wrote -- or one left over from an earlier forward -- shows; the bits are those of the launch alone on the levels
    of a one-stream forward."""
    m, neck = nets()
    x = W.generate_input(128, seed=300 + SIZE[0] + SIZE[1], hw=SIZE)
    rois, pooler = image_rois(128, SIZE, n=300, invalid=True), pooler_for()
    try:
        m.set_streams(1)
        plain = m.forward_fpn(x, neck)
        one = poisoned_forward_rois(m, neck, x, rois, pooler, SIZE)
        m.set_streams(2)
        assert m.parts(128) == 2
        two = poisoned_forward_rois(m, neck, x, rois, pooler, SIZE, levels=("0", "pool"))
    finally:
        m.set_streams(0)
    want, lv = pooled_like_the_launch(plain, pooler.featmap_names, rois, pooler, SIZE)
    V.assert_no_poison(want, False, "reference")
    assert lv[[2, 11, 29]].tolist() == [-1, -1, -1] and not want[[2, 11, 29]].any()
    assert len(set(rois[lv >= 0, 0].astype(int).tolist()) & set(range(64, 128))) > 20       # the second part has rows to write
    for got in (one, two):
        assert np.array_equal(got["roi_levels"], lv) and np.array_equal(bits(got["pooled"]), bits(want))
    assert all(np.array_equal(bits(two[k]), bits(plain[k])) for k in ("0", "pool"))
    m18, neck18 = nets("resnet18")
    try:
        m18.set_input_size(32, 32)
        cap = m18.max_sub_batch()
        x = W.generate_input(cap + 1, seed=43, hw=(32, 32))
        rois = image_rois(cap + 1, (32, 32), n=2 * cap + 9, invalid=True)
        rois[5, 0], rois[6, 0] = cap, cap - 1                        # the last image, alone in its sub-batch, and the one before
        full = m18.forward_fpn(x, neck18)
        want, lv = pooled_like_the_launch(full, pooler.featmap_names, rois, pooler, (32, 32))
        V.assert_no_poison(want, False, "reference")
        whole = poisoned_forward_rois(m18, neck18, x, rois, pooler, (32, 32), levels=("1", "3"))
        assert np.array_equal(whole["roi_levels"], lv) and np.array_equal(bits(whole["pooled"]), bits(want))
        assert lv[5] >= 0 and lv[6] >= 0 and want[5].any() and lv[[2, 11, 29]].tolist() == [-1, -1, -1]
        assert np.array_equal(bits(whole["1"]), bits(full["1"])) and np.array_equal(bits(whole["3"]), bits(full["3"]))
        m18.set_profiling(True)         # the records are the last sub-batch's: one part of one image, one pooler launch
        m18.forward_fpn(x, neck18, levels=("0",), rois=rois, pooler=pooler, validate=False)
        recs = [r for r in m18.profile() if r["layer"] == "fpn"]
        names = [r["op"] for r in recs]
        assert names.count("roi_align") == 1 and names.count("fpn_layer3") == 1 and names.count("fpn_export0") == 1
        assert "fpn_export1" not in names and names[-1] == "roi_align"
        # a part's record carries its share of the output bytes: its images over the call's
        assert abs(recs[-1]["bytes"] / (4.0 * len(rois) * 64 * 49 / (cap + 1)) - 1) < 1e-12
    finally:
        m18.set_profiling(False)
        m18.set_input_size(*SIZE)


def test_profile_records_one_part(nets):
    m, neck = nets()
    x, rois, pooler = images(), image_rois(MB, SIZE), pooler_for()
    m.set_profiling(True)
    try:
        m.forward_fpn(x, neck)
        plain = m.profile()
        m.forward_fpn(x, neck, rois=rois, pooler=pooler)
        recs = m.profile()
    finally:
        m.set_profiling(False)
    ops_ = [r["op"] for r in recs]
    assert ops_.count("roi_align") == 1                               # one per part, and a profiled forward is one part
    at = ops_.index("roi_align")
    assert ops_[at - 1] == "fpn_export_pool"                          # behind the neck's last launch
    assert [(r["op"], r["layer"]) for r in recs[:at] + recs[at + 1:]] == [(r["op"], r["layer"]) for r in plain]
    mine = recs[at]
    assert mine["layer"] == "fpn" and mine["ms"] > 0 and mine["bytes"] == 4.0 * len(rois) * 256 * 49


def test_model_refusals(nets):
    m, neck = nets()
    mb, neckb = nets("resnet50", "bf16")
    lib = L.lib()
    x = ops._up_raw(images())
    rois = image_rois(MB, SIZE)
    dr = ops._up_raw(rois)
    K = len(rois)
    out = V.place_out(K * 256 * 49 * 4)
    asc = (ctypes.c_int * 4)(1, 2, 3, 4)
    names = neck.names

    def req(pooler=None, rois_ptr=dr.ptr, pooled=out.ptr, **kw):
        r = (pooler or pooler_for()).request(names, rois_ptr, K, SIZE, pooled)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def call(model, nk, r, mode=L.RN_FWD_FUSED):
        st = lib.rn_model_forward_rois(model.handle, nk.handle, x.ptr, MB, None, asc, None, ctypes.byref(r) if r else None, mode)
        return st, (lib.rn_last_error(model.ctx.handle) or b"").decode()

    before, before_b = launches(m.ctx), launches(mb.ctx)
    lv4 = req()
    lv4.level[3] = 4                                                          # the pooled level is none of the pooler's
    desc = req()
    desc.level[1], desc.level[2] = 2, 1
    for r, word in ((None, "rois is NULL"), (req(rois_ptr=None), "rois_dev is NULL"), (req(pooled=None), "pooled is NULL"),
                    (lv4, "the neck's"), (desc, "ascending"), (req(n_levels=5), "n_levels"), (req(n_levels=0), "n_levels"),
                    (req(PH=0), "1..32"), (req(PW=33), "1..32"), (req(sampling_ratio=5), "1..4"), (req(aligned=3), "aligned"),
                    (req(image_h=0), "image_h"), (req(canonical_scale=0.0), "canonical_scale"),
                    (req(pooled=out.ptr + 2), "4-byte"), (req(pooled=dr.ptr), "overlaps")):
        st, msg = call(m, neck, r)
        assert st == L.RN_ERR_INVALID and word in msg, (word, st, msg)
    st, msg = call(m, neck, req(sampling_ratio=0))
    assert st == L.RN_ERR_UNSUPPORTED and "adaptive" in msg, (st, msg)
    alias = L.FpnOutputs()                                                    # pooled inside an exported level of the call
    alias.level[0] = out.ptr + 64
    st = lib.rn_model_forward_rois(m.handle, neck.handle, x.ptr, MB, None, asc, ctypes.byref(alias), ctypes.byref(req()),
                                   L.RN_FWD_FUSED)
    assert st == L.RN_ERR_INVALID and "another output" in (lib.rn_last_error(m.ctx.handle) or b"").decode()
    head = L.ModelOutputs(out.ptr + 128, None, None, None, None, 0)           # and the logits inside pooled
    st = lib.rn_model_forward_rois(m.handle, neck.handle, x.ptr, MB, ctypes.byref(head), asc, None, ctypes.byref(req()),
                                   L.RN_FWD_FUSED)
    assert st == L.RN_ERR_INVALID and "another output" in (lib.rn_last_error(m.ctx.handle) or b"").decode()
    st, msg = call(mb, neckb, req(), L.RN_FWD_REFERENCE_OPS)
    assert st == L.RN_ERR_UNSUPPORTED and "bf16" in msg, (st, msg)
    with pytest.raises(ValueError):
        m.forward_fpn(images(), neck, rois=rois, pooler=pooler_for(("0", "4")))          # names that are not the neck's
    with pytest.raises(ValueError):
        m.forward_fpn(images(), neck, rois=rois)                                          # rois without a pooler
    assert launches(m.ctx) == before and launches(mb.ctx) == before_b
    m.ctx.sync()
    V.assert_untouched(out, "refused pooler calls")
    st, msg = call(m, neck, req())                                            # and the call they all almost were
    assert st == L.RN_OK, msg
    m.ctx.sync()
    want = m.forward_fpn(images(), neck, levels=(), rois=rois, pooler=pooler_for())["pooled"]
    assert np.array_equal(bits(V.fetch(out, np.float32, "pooled", written=True).reshape(want.shape)), bits(want))
    empty = req()
    empty.K, empty.rois_dev, empty.pooled = 0, None, None                     # no RoIs: the forward runs, nothing is pooled
    fo = L.FpnOutputs()
    lvl0 = V.place_out(MB * 256 * 18 * 10 * 4)
    fo.level[0] = lvl0.ptr
    st = lib.rn_model_forward_rois(m.handle, neck.handle, x.ptr, MB, None, asc, ctypes.byref(fo), ctypes.byref(empty), L.RN_FWD_FUSED)
    assert st == L.RN_OK
    m.ctx.sync()
    V.fetch(lvl0, np.float32, "level 0 with K == 0", written=True)
