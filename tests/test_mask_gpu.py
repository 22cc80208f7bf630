"""The mask head on the device (rn_mask.hip, the NHWC pooler form of rn_roi.hip): the four launches alone on views between
guard bands, the object, and the stage behind the neck and inside a forward.  What is bit-defined (the NHWC pooler, the
RoI former, the paste) is held to the numpy contract bit for bit; the predictor to a derived bound of float64; the
routes to the stand-alone run of the same device code, bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import views as V
import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import detection as D
from resnet_c_amd import mask as MK
from resnet_c_amd import ops
from resnet_c_amd import roi as RO
from resnet_c_amd import weights as W
from test_detect_gpu import MC, MD, MREP, model_head, same, same_entry
from test_dilation_gpu import bits, tol_f32
from test_fpn_gpu import SIZE, WIDTH, images, launches, nets  # noqa: F401  (nets: a fixture)
from test_mask_host import paste_boxes, paste_probs, predict_case
from test_roi_gpu import DT, FP, PYRAMID, SCALES, make_rois, pyramid_rois, run_roi, typed_map
from test_rpn_gpu import model_rpn
from test_rpn_host import EXPF_ULP

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24


def record(line):
    """print a measured error beside its bound and, where RN_MASK_ERRORS_FILE names a file, append it there: that is how
    profiles/mask/errors_and_bounds.txt is written"""
    print(line)
    path = os.environ.get("RN_MASK_ERRORS_FILE")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


# =====================================================================================================================
# 1. the pooler with an NHWC output
# =====================================================================================================================
NHWC = "rn_roi_align_nhwc_forward_dt"


def roi_args(vm, maps, scales, thr, B, C, vr, K, P_, S, aligned, dtype, out_ptr, lv_ptr):
    n = len(maps)
    sc = np.ascontiguousarray(scales, dtype=F)
    th = np.concatenate([np.asarray(thr, F).reshape(-1), np.zeros(1, F)])
    return (DT[dtype], n, (ctypes.c_void_p * n)(*[v.ptr for v in vm]), (ctypes.c_uint64 * n)(*[m.shape[1] for m in maps]),
            (ctypes.c_uint64 * n)(*[m.shape[2] for m in maps]), sc.ctypes.data_as(FP), th.ctypes.data_as(FP), B, C, vr.ptr, K,
            P_[0], P_[1], S, int(aligned), out_ptr, lv_ptr), (sc, th)


def run_roi_nhwc(maps, rois, scales, thr, P_, S, aligned, dtype):
    """one launch on views between guard bands: input guards intact, the output written everywhere"""
    C, B, K = maps[0].shape[3], maps[0].shape[0], rois.shape[0]
    vm, vr = [V.place(m) for m in maps], V.place(np.ascontiguousarray(rois, dtype=F))
    vo, vl = V.place_out(K * C * P_[0] * P_[1] * 4), V.place_out(K * 4)
    args, keep = roi_args(vm, maps, scales, thr, B, C, vr, K, P_, S, aligned, dtype, vo.ptr, vl.ptr)
    before = launches()
    V.must(NHWC, *args)
    assert launches() == before + 1
    V.check_guards(f"{NHWC} inputs", vr, *vm)
    what = f"{NHWC} {dtype} C={C} {P_} S={S}"
    return (V.fetch(vo, F, what, written=True).reshape(K, P_[0], P_[1], C), V.fetch(vl, np.int32, what + " levels", written=True))


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("P_", [(1, 1), (3, 2), (14, 14)], ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("dtype,C", [("f32", 4), ("f32", 68), ("f32", 256), ("bf16", 8), ("bf16", 64)])
def test_roi_align_nhwc_is_the_transpose_bit_for_bit(dtype, C, P_, S):
    """one level, K = 37 (more rows than one block's, an odd count), rows of an invalid image index among them: every
    value is rn_roi_align_forward_dt's at the transposed position, the zero rows and level -1 included"""
    B, h, w = 2, 5, 6
    maps = [typed_map((B, h, w, C), dtype, seed=C + h)]
    rois = make_rois(h, w, B, n=27)[:37]
    assert rois.shape[0] == 37
    rois[5, 0], rois[11, 0], rois[36, 0] = -1.0, B, 0.5
    want, wl = run_roi(maps, rois, (0.25,), (), P_, S, False, dtype)
    got, gl = run_roi_nhwc(maps, rois, (0.25,), (), P_, S, False, dtype)
    assert np.array_equal(bits(got), bits(np.ascontiguousarray(want.transpose(0, 2, 3, 1))))
    assert np.array_equal(gl, wl) and (gl[[5, 11, 36]] == -1).all() and not got[[5, 11, 36]].any() and got.any()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_roi_align_nhwc_four_levels_and_one_row(dtype):
    B, C = 2, 16
    maps = [typed_map((B, h, w, C), dtype, seed=h) for h, w in PYRAMID]
    thr = ops.roi_level_thresholds(SCALES)
    rois = pyramid_rois(B, thr)
    for r, P_ in ((rois, (3, 2)), (rois[:1], (14, 14))):    # K = 1: one block row
        want, wl = run_roi(maps, r, SCALES, thr, P_, 2, True, dtype)
        got, gl = run_roi_nhwc(maps, r, SCALES, thr, P_, 2, True, dtype)
        assert np.array_equal(bits(got), bits(np.ascontiguousarray(want.transpose(0, 2, 3, 1)))) and np.array_equal(gl, wl)
    assert len(set(wl.tolist())) >= 1 and set(run_roi(maps, rois, SCALES, thr, (1, 1), 1, False, dtype)[1].tolist()) == {0, 1, 2, 3}
    py = ops.roi_align_nhwc(maps, rois, SCALES, (3, 2), 2, True, thr, bf16=dtype == "bf16")
    assert np.array_equal(bits(py), bits(np.ascontiguousarray(run_roi(maps, rois, SCALES, thr, (3, 2), 2, True, dtype)[0].transpose(0, 2, 3, 1))))


def test_roi_align_nhwc_refusals_launch_nothing():
    B, h, w, C, K = 2, 4, 5, 8, 3
    maps = [np.ones((B, h, w, C), F)]
    vm, vr = [V.place(maps[0])], V.place(make_rois(h, w, B, n=3)[:K])
    vo = V.place_out(K * C * 4 * 4, 0)
    n0 = launches()
    for ptr, text in ((vo.ptr + 4, "out is off a 16-byte boundary"), (vo.ptr + 8, "16-byte"), (vm[0].ptr, "out overlaps"),
                      (vr.ptr - 16, "out overlaps rois_dev")):
        args, keep = roi_args(vm, maps, (0.25,), (), B, C, vr, K, (2, 2), 2, False, "f32", ptr, None)
        st, msg = V.call(NHWC, *args)
        assert st == L.RN_ERR_INVALID and text in msg and NHWC in msg, (st, msg, text)
    assert launches() == n0
    V.assert_untouched(vo, "refused calls")
    args, keep = roi_args(vm, maps, (0.25,), (), B, C, vr, 0, (2, 2), 2, False, "f32", None, None)
    assert V.call(NHWC, *args)[0] == L.RN_OK and launches() == n0       # K == 0


# =====================================================================================================================
# 2. detections -> RoIs
# =====================================================================================================================
@pytest.mark.parametrize("off", [0, 4, 8, 12])
def test_detection_rois_equal_the_contract(off):
    B, Dn = 3, 5
    g = np.random.default_rng(B * Dn)
    boxes = g.uniform(-5, 80, (B, Dn, 4)).astype(F)
    labels = g.integers(1, 9, (B, Dn)).astype(np.int32)
    labels[0, 3:], labels[1, :], labels[2, 4] = -1, -1, 0      # padding rows, an image without a detection, a background label
    vb, vl, vo = V.place(boxes), V.place(labels), V.place_out(B * Dn * 20, off)
    n0 = launches()
    V.must("rn_detection_rois_forward", vb.ptr, vl.ptr, B, Dn, vo.ptr)
    assert launches() == n0 + 1
    V.check_guards("rn_detection_rois_forward inputs", vb, vl)
    got = V.fetch(vo, F, "rois", written=True).reshape(B * Dn, 5)
    assert np.array_equal(bits(got), bits(MK.detection_rois_ref(boxes, labels)))
    if off == 0:
        assert np.array_equal(bits(ops.detection_rois(boxes, labels)), bits(got))
        n0 = launches()
        for args, text in (((None, vl.ptr, B, Dn, vo.ptr), "boxes is NULL"), ((vb.ptr, None, B, Dn, vo.ptr), "labels is NULL"),
                           ((vb.ptr, vl.ptr, B, Dn, None), "rois is NULL"), ((vb.ptr, vl.ptr, B, Dn, vb.ptr), "overlaps"),
                           ((vb.ptr, vl.ptr, B, Dn, vo.ptr + 2), "rois is off")):
            st, msg = V.call("rn_detection_rois_forward", *args)
            assert st == L.RN_ERR_INVALID and text in msg, (st, msg, text)
        assert V.call("rn_detection_rois_forward", vb.ptr, vl.ptr, 0, Dn, vo.ptr)[0] == L.RN_OK
        assert launches() == n0, "a refusal launches nothing"


# =====================================================================================================================
# 3. the class-selected predictor
# =====================================================================================================================
def prob_bound(p64, e_z):
    """How far the fp32 probability may lie from float64's, first order in u = 2^-24, derived as test_rpn_host.decode_bound
    is.  With z the fp32 logit, |z - z64| <= e_z:
        e = expf(-z)        the argument's absolute error e_z is a relative error e_z of the exponential; expf itself is
                            within EXPF_ULP units in the last place, at most 2 EXPF_ULP u relative
        s = 1 + e           u relative
        p = 1 / s           u relative (a correctly rounded division)
    dp/de = -1 / (1 + e)^2, so a relative error d of e moves p by e / (1 + e)^2 d = p (1 - p) d; the two roundings move
    it by 2 u p, taken as 3 u p.  Hence |p - p64| <= p64 (1 - p64) (e_z + 2 EXPF_ULP u) + 3 u p64."""
    return p64 * (1.0 - p64) * (e_z + 2 * EXPF_ULP * U) + 3 * U * p64


def run_predict(t, labels, w, b, C):
    K, M, Cr = t.shape[0], t.shape[1], w.shape[1]
    vt, vl, vw, vb = V.place(t), V.place(labels), V.place(w), V.place(b)
    vo = V.place_out(K * 4 * M * M * 4)
    n0 = launches()
    V.must("rn_mask_predict_forward", vt.ptr, vl.ptr, vw.ptr, vb.ptr, K, M, Cr, C, vo.ptr)
    assert launches() == n0 + 1
    V.check_guards("rn_mask_predict_forward inputs", vt, vl, vw, vb)
    return V.fetch(vo, F, f"probs Cr={Cr} M={M} C={C}", written=True).reshape(K, 2 * M, 2 * M)


@pytest.mark.parametrize("Cr,M,C", [(64, 1, 2), (64, 2, 5), (256, 14, 91)])
def test_mask_predict_against_float64(Cr, M, C):
    """The probability within prob_bound of predict_ref, with e_z = tol_f32(z64, Cr) the bound of the fp32 logit (the
    logit itself never leaves the kernel: the probability's bound divided by p (1 - p) IS the statement about it).  Rows
    of a label outside [1, C) are exactly zero, every output is written over the poison, and the same rows at another
    row offset inside a larger K return the same bits."""
    K = 12
    t, labels, w, b = predict_case(Cr, M, C, K)
    assert {0, -1, C, C - 1, 1} <= set(labels.tolist())
    got = run_predict(t, labels, w, b, C)
    p64, z64 = MK.predict_ref(MK.panel_to_nchw(t), labels, w, b, return_logits=True)
    ok = (labels >= 1) & (labels < C)
    assert not got[~ok].any() and ok.sum() >= K - 4 and got[ok].min() > 0
    bound = prob_bound(p64[ok], tol_f32(z64[ok], Cr))
    err = np.abs(got[ok].astype(np.float64) - p64[ok])
    assert (err <= bound).all(), float((err / bound).max())
    assert p64[ok].min() < 0.2 and p64[ok].max() > 0.8, "the probabilities spread over (0, 1)"
    record(f"mask_predict Cr {Cr} M {M} C {C}: max error {err.max():.3e}, largest share of the bound {float((err / bound).max()):.3e}")
    # position independence: rows 3.. of the case as rows 20.. of 29 rows
    big_t = np.concatenate([np.ones((20,) + t.shape[1:], F), t[3:]])
    big_l = np.concatenate([np.full(20, 1, np.int32), labels[3:]])
    again = run_predict(big_t, big_l, w, b, C)
    assert np.array_equal(bits(again[20:]), bits(got[3:]))
    if M == 2:
        assert np.array_equal(bits(ops.mask_predict(t, labels, w, b)), bits(got))


def test_mask_predict_refusals_launch_nothing():
    t, labels, w, b = predict_case(64, 2, 5, 4)
    vt, vl, vw, vb, vo = V.place(t), V.place(labels), V.place(w), V.place(b), V.place_out(4 * 16 * 4)
    good = dict(t=vt.ptr, l=vl.ptr, w=vw.ptr, b=vb.ptr, K=4, M=2, Cr=64, C=5, o=vo.ptr)

    def call(**kw):
        a = {**good, **kw}
        return V.call("rn_mask_predict_forward", a["t"], a["l"], a["w"], a["b"], a["K"], a["M"], a["Cr"], a["C"], a["o"])

    n0 = launches()
    for kw, text in ((dict(Cr=96), "Cr must be"), (dict(Cr=2048), "Cr must be"), (dict(M=0), "M must be"), (dict(M=33), "M must be"),
                     (dict(C=1), "C must be"), (dict(C=1025), "C must be"), (dict(t=None), "t is NULL"), (dict(l=None), "labels is NULL"),
                     (dict(w=None), "weight or bias"), (dict(o=None), "probs is NULL"), (dict(t=vt.ptr + 4), "t is off a 16-byte"),
                     (dict(w=vw.ptr + 4), "weight is off a 16-byte"), (dict(o=vo.ptr + 2), "probs is off"), (dict(o=vt.ptr), "overlaps"),
                     (dict(o=vl.ptr), "overlaps")):
        st, msg = call(**kw)
        assert st == L.RN_ERR_INVALID and text in msg, (kw, st, msg)
    assert call(K=0)[0] == L.RN_OK and launches() == n0
    V.assert_untouched(vo, "refused calls")


# =====================================================================================================================
# 4. the paste
# =====================================================================================================================
def paste_case(H, W, Mo):
    """the host test's boxes, then three rows that must be all zeros: a label of -1, a NaN and an infinity"""
    boxes = np.concatenate([paste_boxes(H, W), np.array([[1, 1, W - 1, H - 1], [1, np.nan, W - 1, H - 1], [0, 0, np.inf, H]], F)])
    labels = np.ones(boxes.shape[0], np.int32)
    labels[-3], labels[2] = -1, 7
    return paste_probs(boxes.shape[0], Mo, seed=H), boxes, labels


def run_paste(probs, boxes, labels, H, W, thr=0.5, masks=True, bits_=True, moff=0, boff=0):
    K, Mo = probs.shape[0], probs.shape[1]
    vp, vb, vl = V.place(probs), V.place(boxes), V.place(labels) if labels is not None else None
    vm = V.place_out(K * H * W * 4, moff) if masks else None
    vbits = V.place_out(K * H * W, boff) if bits_ else None
    n0 = launches()
    V.must("rn_paste_masks_forward", vp.ptr, vb.ptr, vl.ptr if vl else None, K, Mo, H, W, thr, vm.ptr if vm else None,
           vbits.ptr if vbits else None)
    assert launches() == n0 + 1
    V.check_guards("rn_paste_masks_forward inputs", vp, vb, vl)
    what = f"paste {H}x{W} Mo={Mo} +{moff}/+{boff}"
    return (V.fetch(vm, F, what + " masks", written=True).reshape(K, H, W) if masks else None,
            V.fetch(vbits, np.uint8, what + " bits", written=True).reshape(K, H, W) if bits_ else None)


@pytest.mark.parametrize("Mo", [2, 4, 28])
@pytest.mark.parametrize("size", [(5, 3), (37, 53), (64, 64), (96, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_paste_is_the_contract_bit_for_bit(size, Mo):
    """masks bit for bit paste_masks_ref and bits == (masks > threshold); (96, 131): more than one block to a plane and an
    odd width.  Both outputs from one launch, behind guard bands, over the poison."""
    H, W = size
    probs, boxes, labels = paste_case(H, W, Mo)
    want = MK.paste_masks_ref(probs, boxes, size, labels)
    assert want.any() and not want[-3:].any() and not want[10].any()
    masks, got_bits = run_paste(probs, boxes, labels, H, W)
    assert np.array_equal(bits(masks), bits(want)), np.flatnonzero(bits(masks) != bits(want))[:8]
    assert np.array_equal(got_bits, (want > F(0.5)).astype(np.uint8))
    assert got_bits.any() and not got_bits.all()


def test_paste_offsets_single_outputs_and_threshold():
    """masks 0, 4, 8 and 12 bytes off a 16-byte boundary, bits 0..3 bytes off a word; either output alone; labels NULL; a
    threshold below zero sets every bit"""
    H, W, Mo = 37, 53, 4
    probs, boxes, labels = paste_case(H, W, Mo)
    want = MK.paste_masks_ref(probs, boxes, (H, W), labels)
    for moff, boff in ((0, 0), (4, 1), (8, 2), (12, 3)):
        masks, b = run_paste(probs, boxes, labels, H, W, moff=moff, boff=boff)
        assert np.array_equal(bits(masks), bits(want)) and np.array_equal(b, (want > F(0.5)).astype(np.uint8)), (moff, boff)
        only_m, none = run_paste(probs, boxes, labels, H, W, bits_=False, moff=moff)
        none2, only_b = run_paste(probs, boxes, labels, H, W, masks=False, boff=boff)
        assert none is None and none2 is None and np.array_equal(bits(only_m), bits(want)) and np.array_equal(only_b, b)
    free = MK.paste_masks_ref(probs, boxes, (H, W))
    masks, b = run_paste(probs, boxes, None, H, W, thr=-1.0)
    assert np.array_equal(bits(masks), bits(free)) and free[-3].any() and b.all()
    py_m, py_b = ops.paste_masks(probs, boxes, (H, W), labels, 0.25, masks=True, bits=True)
    assert np.array_equal(bits(py_m), bits(want)) and np.array_equal(py_b, (want > F(0.25)).astype(np.uint8))


def test_paste_refusals_launch_nothing():
    H, W, Mo = 5, 3, 2
    probs, boxes, labels = paste_case(H, W, Mo)
    K = probs.shape[0]
    vp, vb, vl = V.place(probs), V.place(boxes), V.place(labels)
    vm, vbits = V.place_out(K * H * W * 4), V.place_out(K * H * W)
    good = dict(p=vp.ptr, b=vb.ptr, l=vl.ptr, K=K, Mo=Mo, H=H, W=W, thr=0.5, m=vm.ptr, bits=vbits.ptr)

    def call(**kw):
        a = {**good, **kw}
        return V.call("rn_paste_masks_forward", a["p"], a["b"], a["l"], a["K"], a["Mo"], a["H"], a["W"], a["thr"], a["m"], a["bits"])

    n0 = launches()
    for kw, text in ((dict(Mo=0), "Mo must be"), (dict(Mo=65), "Mo must be"), (dict(H=0), "H and W"), (dict(W=1 << 24), "H and W"),
                     (dict(thr=np.nan), "NaN"), (dict(m=None, bits=None), "both NULL"), (dict(p=None), "probs is NULL"),
                     (dict(b=None), "boxes is NULL"), (dict(m=vm.ptr + 2), "masks is off"), (dict(m=vp.ptr), "overlaps"),
                     (dict(bits=vm.ptr + 5), "overlaps"), (dict(bits=vb.ptr + 1), "overlaps")):
        st, msg = call(**kw)
        assert st == L.RN_ERR_INVALID and text in msg, (kw, st, msg)
    assert call(K=0)[0] == L.RN_OK and launches() == n0
    V.assert_untouched(vm, "refused calls")
    V.assert_untouched(vbits, "refused calls")


# =====================================================================================================================
# 5. the object
# =====================================================================================================================
@pytest.mark.parametrize("in_channels,layers,Cr,M", [(64, (64,), 64, 2), (256, (256,) * 4, 256, 14)])
def test_object_against_float64(in_channels, layers, Cr, M):
    """probs against mask_head_ref followed by predict_ref.  The logit's bound accumulates layer by layer as the box head's
    does: a layer amplifies its input's error by at most the largest L1 norm of a row of its weights and adds its own
    tol_f32(output, products); ReLU moves no two values apart; the label's row of mask_fcn_logits amplifies by its own L1
    norm.  Then prob_bound.  The paste of the returned probs: bit for bit ops.paste_masks on them."""
    C, K = 5, 6
    st = MK.generate_mask_head_state(in_channels, layers, Cr, C, seed=M)
    g = np.random.default_rng(in_channels + M)
    pooled = np.maximum(g.standard_normal((K, in_channels, M, M)), 0).astype(F)
    labels = np.array([1, 4, -1, 2, 3, 1], np.int32)
    boxes = np.concatenate([paste_boxes(*SIZE)[[0, 2, 6, 7, 8]], [[3, 2, 30, 60]]]).astype(F)
    mh = R.MaskHead(in_channels, layers, Cr, C, {"roi_heads." + k: v for k, v in st.items()}, resolution=M)
    mh.poison = True
    try:
        n0 = launches()
        out = mh(np.ascontiguousarray(pooled.transpose(0, 2, 3, 1)), labels, boxes, SIZE, masks=("probs", "image", "bits"))
        n = len(layers) + 1
        assert n + 2 <= launches() - n0 <= 2 * n + 2, "n_layers + 1 contractions of one or two launches, the predict, the paste"
        for k, v in out.items():
            V.check_written(np.ascontiguousarray(v).view(np.uint8), v.dtype.itemsize, k)
        probs = out["mask_probs"][0]
        outs = MK.mask_head_ref(pooled, st, layers=True)
        l1 = lambda w: np.abs(w.reshape(w.shape[0], -1)).sum(axis=1).max()  # noqa: E731
        e, cin = 0.0, in_channels
        for i, c in enumerate(layers):
            e = e * l1(st[f"mask_head.{i}.0.weight"].astype(np.float64)) + tol_f32(outs[i], 9 * cin)
            cin = c
        rows, _ = MK.deconv_panel(st[MK.PREDICTOR_KEYS[0]].astype(np.float64), st[MK.PREDICTOR_KEYS[1]])
        e_t = e * l1(rows) + tol_f32(outs[-1], cin)
        wl = st[MK.PREDICTOR_KEYS[2]].reshape(C, Cr).astype(np.float64)
        p64, z64 = MK.predict_ref(outs[-1], labels, wl, st[MK.PREDICTOR_KEYS[3]], return_logits=True)
        ok = labels >= 1
        e_z = (e_t * np.abs(wl[np.clip(labels, 0, C - 1)]).sum(axis=1))[:, None, None] + tol_f32(z64[ok], Cr)
        bound = prob_bound(p64[ok], e_z[ok])
        err = np.abs(probs[ok].astype(np.float64) - p64[ok])
        assert (err <= bound).all(), float((err / bound).max())
        assert not probs[~ok].any() and 0 < probs[ok].min() and probs[ok].max() < 1
        record(f"mask head in {in_channels} layers {layers} Cr {Cr} M {M}: prob error {err.max():.3e}, largest share of the bound "
               f"{float((err / bound).max()):.3e} (logit bound {float(e_z[ok].max()):.3e})")
        masks, b = ops.paste_masks(probs, boxes, SIZE, labels, 0.5, masks=True, bits=True)
        assert same(out["masks"][0], masks) and np.array_equal(out["mask_bits"][0], b) and masks.any() and not masks[2].any()
        only = mh(np.ascontiguousarray(pooled.transpose(0, 2, 3, 1)), labels, boxes, SIZE, masks=("bits",))    # probs in the scratch
        assert sorted(only) == ["mask_bits"] and np.array_equal(only["mask_bits"][0], b)
        assert same(mh(np.ascontiguousarray(pooled.transpose(0, 2, 3, 1)), labels)["mask_probs"][0], probs)   # no boxes: no paste
    finally:
        mh.close()


def test_object_refusals():
    lib, ctx = L.lib(), R.get_ctx()
    h = ctypes.c_void_p()
    u64s = lambda *v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731
    n0 = launches()
    for args in ((100, 1, u64s(64), 64, 5, 2), (64, 0, u64s(64), 64, 5, 2), (64, 9, u64s(*[64] * 9), 64, 5, 2), (64, 1, u64s(96), 64, 5, 2),
                 (64, 1, u64s(64), 32, 5, 2), (64, 1, u64s(64), 2048, 5, 2), (64, 1, u64s(64), 64, 1, 2), (64, 1, u64s(64), 64, 5, 0),
                 (64, 1, u64s(64), 64, 5, 33), (64, 1, None, 64, 5, 2)):
        assert lib.rn_mask_head_create(ctx.handle, ctypes.byref(h), *args) == L.RN_ERR_INVALID, args[:2] + args[3:]
    assert launches() == n0, "a refusal launches nothing"
    assert lib.rn_mask_head_create(ctx.handle, ctypes.byref(h), 64, 1, u64s(64), 64, 5, 2) == L.RN_OK
    w = np.zeros(64 * 64 * 9, F)
    assert lib.rn_mask_head_set_tensor(h, b"mask_head.0.0.weight", w.ctypes.data, w.size) == L.RN_OK
    assert lib.rn_mask_head_set_tensor(h, b"roi_heads.mask_head.mask_fcn1.bias", w.ctypes.data, 64) == L.RN_OK
    assert lib.rn_mask_head_set_tensor(h, b"mask_head.0.0.bias", w.ctypes.data, 63) == L.RN_ERR_INVALID
    assert lib.rn_mask_head_set_tensor(h, b"mask_head.1.0.weight", w.ctypes.data, w.size) == L.RN_ERR_INVALID   # one layer only
    assert lib.rn_mask_head_set_tensor(h, b"mask_predictor.conv6_mask.weight", w.ctypes.data, 64) == L.RN_ERR_INVALID
    assert b"unknown key" in lib.rn_last_error(ctx.handle)
    assert lib.rn_mask_head_finalize(h) == L.RN_ERR_INVALID and b"is not set" in lib.rn_last_error(ctx.handle)
    assert launches() == n0, "a refusal launches nothing"
    assert lib.rn_mask_head_destroy(h) == L.RN_OK
    mh = R.MaskHead(64, (64,), 64, 5, MK.generate_mask_head_state(64, (64,), 64, 5, seed=1), resolution=2)
    try:
        K = 4
        pooled, labels, boxes = V.place(np.zeros((K, 2, 2, 64), F)), V.place(np.ones(K, np.int32)), V.place(np.zeros((K, 4), F))
        spec, bufs = mh.buffers(1, K, SIZE, ("probs", "image", "bits"))

        def fwd(q, p=pooled.ptr, l=labels.ptr, b=boxes.ptr, image=SIZE, K=K):
            s = lib.rn_mask_head_forward(mh.handle, p, l, b, K, image[0], image[1], ctypes.byref(q) if q is not None else None)
            return s, (lib.rn_last_error(ctx.handle) or b"").decode()

        def req(**kw):
            q = mh.request(bufs)
            for k, v in kw.items():
                setattr(q, k, v)
            return q

        n0 = launches()
        cases = [(fwd(None), "request is NULL"), (fwd(req(probs=None, masks=None, bits=None)), "all NULL"),
                 (fwd(req(), b=None), "boxes is NULL"), (fwd(req(), p=None), "pooled_nhwc is NULL"), (fwd(req(), l=None), "labels is NULL"),
                 (fwd(req(), p=pooled.ptr + 4), "16-byte"), (fwd(req(), image=(0, 5)), "H and W"), (fwd(req(threshold=np.nan)), "NaN"),
                 (fwd(req(probs=pooled.ptr)), "overlaps"), (fwd(req(bits=bufs["masks"].ptr + 3)), "overlaps"),
                 (fwd(req(masks=bufs["masks"].ptr + 2)), "masks is off")]
        for i, ((s, msg), text) in enumerate(cases):
            assert s == L.RN_ERR_INVALID and text in msg, (i, s, msg, text)
        assert fwd(req(), K=0)[0] == L.RN_OK
        assert launches() == n0, "a refusal launches nothing"
        s, msg = fwd(req())
        assert s == L.RN_OK, msg
        ctx.sync()
        assert launches() > n0
    finally:
        mh.close()


# =====================================================================================================================
# 6. behind the neck and inside a forward
# =====================================================================================================================
MASKS = ("probs", "image", "bits")
MASK_KEYS = ("mask_rois", "mask_pooled", "mask_probs", "masks", "mask_bits")
MM = 2     # the resolution of the model tests' mask heads


def model_mask(arch, in_channels=None):
    a = in_channels or WIDTH[arch]
    mh = R.MaskHead(a, (64,), 64, MC, MK.generate_mask_head_state(a, (64,), 64, MC, seed=8), resolution=MM)
    mh.poison = True
    return mh


def check_masks(got, mh, levels=None):
    """mask_rois is the contract on the call's own detections; mask_pooled is ops.roi_align_nhwc on the exported levels
    (where the call exported them); every other entry is the stand-alone MaskHead run on that mask_pooled, the labels and
    the boxes, bit for bit; no output keeps its poison"""
    B, Dn = got["labels"].shape
    for k in MASK_KEYS:
        V.check_written(np.ascontiguousarray(got[k]).view(np.uint8), got[k].dtype.itemsize, k)
    assert same(got["mask_rois"], MK.detection_rois_ref(got["boxes"], got["labels"]))
    if levels is not None:
        maps = [np.ascontiguousarray(got[k].transpose(0, 2, 3, 1)) for k in levels]
        scales = RO.infer_scales([m.shape[1:3] for m in maps], SIZE)
        want = ops.roi_align_nhwc(maps, got["mask_rois"], scales, MM, mh.pooler.sampling_ratio, False, mh.pooler.thresholds(scales),
                                  validate=False)
        assert same(got["mask_pooled"], want)
    alone = mh(got["mask_pooled"], got["labels"].reshape(-1), got["boxes"].reshape(-1, 4), SIZE, masks=MASKS)
    for k in ("mask_probs", "masks", "mask_bits"):
        assert same_entry(got[k], alone[k].reshape(got[k].shape)), k
    none = got["labels"] < 1
    assert not got["mask_probs"][none].any() and not got["masks"][none].any() and not got["mask_bits"][none].any()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_model_route_bit_for_bit(nets, arch, dtype):
    m, neck = nets(arch, dtype)
    x = np.array(images())
    net, bh, mh, pooler = model_rpn(arch), model_head(arch), model_mask(arch), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2)
    kw = dict(rpn=net, pooler=pooler, box_head=bh, detect_intermediates=True)
    try:
        n0 = launches()
        plain = m.forward_fpn(x, neck, roi_levels=True, candidates=True, **kw)
        n1 = launches()
        got = m.forward_fpn(x, neck, roi_levels=True, candidates=True, mask_head=mh, masks=MASKS, mask_pooled=True, **kw)
        added = (launches() - n1) - (n1 - n0)
        assert 2 + 2 + 2 <= added <= 2 + 4 + 2, "the RoI former, the pooler, two contractions of one or two launches, predict, paste"
        for k in plain:
            assert same_entry(plain[k], got[k]), k
        assert sorted(set(got) - set(plain)) == sorted(MASK_KEYS)
        check_masks(got, mh, levels=("0", "1", "2", "3"))
        assert got["detections"].max() > 0 and got["masks"].any() and got["mask_bits"].any(), "something was pasted"
        record(f"model route {arch} {dtype}: counts {got['detections'].tolist()}, {int(got['mask_bits'].sum())} mask pixels set")
        few = m.forward_fpn(x, neck, levels=(), mask_head=mh, **kw)                    # probs alone, pooled and rois in the scratch
        assert sorted(k for k in few if k.startswith("mask")) == ["mask_probs", "mask_rois"] and same_entry(few["mask_probs"], got["mask_probs"])
        if dtype == "f32" and arch == "resnet18":
            px = np.random.default_rng(9).integers(0, 256, (2,) + SIZE + (3,), dtype=np.uint8)
            from resnet_c_amd import preprocess
            u8 = m.forward_fpn_u8(px, neck, mask_head=mh, masks=MASKS, mask_pooled=True, **kw)
            fl = m.forward_fpn(preprocess.normalize_u8(px), neck, mask_head=mh, masks=MASKS, mask_pooled=True, **kw)
            for k in MASK_KEYS + ("boxes", "labels"):
                assert same_entry(u8[k], fl[k]), k
            check_masks(u8, mh, levels=("0", "1", "2", "3"))
            # the neck route: the same stage behind rn_fpn_forward_masks on the exported stage maps, held to the same statement
            maps = m.forward_maps(x, R.NativeModel.STAGES)
            nhwc = [np.ascontiguousarray(maps[s].transpose(0, 2, 3, 1)) for s in R.NativeModel.STAGES]
            via = neck.forward(nhwc, image_size=SIZE, mask_head=mh, masks=MASKS, mask_pooled=True, **kw)
            check_masks(via, mh, levels=("0", "1", "2", "3"))
            assert via["detections"].max() > 0 and via["masks"].any()
    finally:
        net.close()
        bh.close()
        mh.close()


def test_model_parts_sub_batches_and_profile(nets):
    """128 images as two parts on two streams, then one image more than a launch batch holds: every part runs the stage on
    its own detection rows and writes its own images' rows; the bits are those of one stream; one mask_stage record per
    part in the profile"""
    m, neck = nets()
    x = W.generate_input(128, seed=300 + SIZE[0] + SIZE[1], hw=SIZE)
    net, bh, mh, pooler = model_rpn("resnet50"), model_head("resnet50"), model_mask("resnet50"), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2)
    kw = dict(levels=(), rpn=net, pooler=pooler, box_head=bh, mask_head=mh, masks=MASKS, mask_pooled=True)
    try:
        m.set_streams(1)
        one = m.forward_fpn(x, neck, **kw)
        m.set_streams(2)
        assert m.parts(128) == 2
        two = m.forward_fpn(x, neck, **kw)
        m.set_streams(0)
        for k in MASK_KEYS:
            V.check_written(np.ascontiguousarray(two[k]).view(np.uint8), two[k].dtype.itemsize, k)
            assert same_entry(one[k], two[k]), k
        assert same(two["mask_rois"], MK.detection_rois_ref(two["boxes"], two["labels"]))
        assert two["masks"][64:].any() and two["masks"][:64].any()
    finally:
        m.set_streams(0)
        net.close()
        bh.close()
        mh.close()
    m18, neck18 = nets("resnet18")
    net18, bh18, mh18 = model_rpn("resnet18", post=20), model_head("resnet18", D_=4), model_mask("resnet18")
    kw = dict(levels=(), rpn=net18, pooler=pooler, box_head=bh18, mask_head=mh18, masks=("probs", "bits"))
    try:
        m18.set_input_size(32, 32)
        cap = m18.max_sub_batch()
        x = W.generate_input(cap + 1, seed=43, hw=(32, 32))
        whole = m18.forward_fpn(x, neck18, **kw)
        for k in ("mask_rois", "mask_probs", "mask_bits"):
            V.check_written(np.ascontiguousarray(whole[k]).view(np.uint8), whole[k].dtype.itemsize, k)
        pick = [0, 1, cap - 1, cap]
        few = m18.forward_fpn(x[pick], neck18, **kw)
        for k in ("mask_probs", "mask_bits"):
            assert same_entry(whole[k][pick], few[k]), k
        assert few["mask_bits"].any()
        m18.set_profiling(True)
        m18.forward_fpn(x[:2], neck18, **kw)
        recs = [(r["layer"], r["op"]) for r in m18.profile() if r["layer"] in ("fpn", "rpn", "roi_heads")]
        assert recs.count(("roi_heads", "mask_stage")) == 1 and recs[-1] == ("roi_heads", "mask_stage") and recs[-2] == ("roi_heads", "box_stage")
    finally:
        m18.set_profiling(False)
        m18.set_input_size(*SIZE)
        net18.close()
        bh18.close()
        mh18.close()


def test_model_draw_with_no_detection_beside_full_images(nets):
    """test_detect_gpu's draw: two images of zeros among 126 others under a head that turns every proposal of a zero image
    down.  Their detection rows are padding, so their RoI rows are (-1, 0, 0, 0, 0) and their masks all zeros, written by
    the part that holds them beside a neighbour's pasted masks."""
    m, neck = nets()
    x = W.generate_input(128, seed=300 + SIZE[0] + SIZE[1], hw=SIZE)
    x[3] = 0
    x[70] = 0
    st = D.generate_box_head_state(WIDTH["resnet50"] * 4, MREP, MC, seed=6)
    st["box_head.fc6.bias"][:] = 0
    st["box_head.fc7.bias"][:] = 0
    st["box_predictor.cls_score.bias"][:] = [4, 0, 0, 0, 0]
    net, pooler, mh = model_rpn("resnet50"), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2), model_mask("resnet50")
    bh = R.BoxHead(WIDTH["resnet50"], 2, MREP, MC, st, detections_per_img=4)
    bh.poison = True
    try:
        m.set_streams(2)
        assert m.parts(128) == 2
        got = m.forward_fpn(x, neck, levels=(), rpn=net, pooler=pooler, box_head=bh, mask_head=mh, masks=MASKS, mask_pooled=True)
        m.set_streams(0)
        zero = np.zeros(128, bool)
        zero[[3, 70]] = True
        assert (got["detections"][zero] == 0).all() and (got["detections"][~zero] == 4).all(), got["detections"].tolist()
        check_masks(got, mh)
        rois = got["mask_rois"].reshape(128, 4, 5)
        assert (rois[zero, :, 0] == -1).all() and not rois[zero, :, 1:].any() and (rois[~zero, :, 0] == np.arange(128)[~zero, None]).all()
        for k in ("mask_probs", "masks", "mask_bits"):
            assert not got[k][zero].any() and got[k][~zero].any(), k
        assert not got["mask_pooled"].reshape(128, -1)[zero].any()
        assert all(got["masks"][b].any() for b in (2, 4, 69, 71))
    finally:
        m.set_streams(0)
        net.close()
        bh.close()
        mh.close()


def test_model_route_refusals(nets):
    m, neck = nets("resnet18")
    x = np.array(images())
    net, bh, mh, pooler = model_rpn("resnet18"), model_head("resnet18"), model_mask("resnet18"), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2)
    wide = model_mask("resnet18", in_channels=128)
    kw = dict(rpn=net, pooler=pooler, box_head=bh)
    box_request, mask_request = bh.request, mh.request

    def without(name):
        def request(bufs):
            q = box_request(bufs)
            setattr(q.out, name, None)
            return q
        return request

    def sharing(bufs, names=None):
        q = mask_request(bufs, names)
        q.probs = bufs["mask_rois"].ptr
        return q

    def on_the_boxes(bufs, names=None):
        q = mask_request(bufs, names)
        q.probs = on_the_boxes.boxes
        return q

    try:
        n0 = launches()
        with pytest.raises(ValueError, match="box_head"):
            m.forward_fpn(x, neck, rpn=net, pooler=pooler, mask_head=mh)
        for name in ("boxes", "labels"):
            bh.request = without(name)
            with pytest.raises(L.RnError, match="boxes and labels"):
                m.forward_fpn(x, neck, mask_head=mh, **kw)
        bh.request = box_request
        mh.request = sharing
        with pytest.raises(L.RnError, match="overlaps"):
            m.forward_fpn(x, neck, mask_head=mh, **kw)
        spec, dbufs = bh.buffers(x.shape[0], 60)
        bh.buffers = lambda *a, **k: (spec, dbufs)
        on_the_boxes.boxes = dbufs["boxes"].ptr
        mh.request = on_the_boxes
        with pytest.raises(L.RnError, match="overlaps"):
            m.forward_fpn(x, neck, mask_head=mh, **kw)
        del bh.buffers
        mh.request = mask_request
        with pytest.raises(L.RnError, match="in_channels"):
            m.forward_fpn(x, neck, mask_head=wide, **kw)
        with pytest.raises(ValueError, match="unknown mask output"):
            m.forward_fpn(x, neck, mask_head=mh, masks=("pixels",), **kw)
        assert launches() == n0, "a refusal launches nothing"
        assert m.forward_fpn(x, neck, levels=(), mask_head=mh, **kw)["mask_probs"].any()
    finally:
        bh.request, mh.request = box_request, mask_request
        net.close()
        bh.close()
        mh.close()
        wide.close()
