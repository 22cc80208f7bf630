"""The keypoint head on the GPU (csrc/rn_keypoint.hip): the search and the predict launch against the numpy contracts bit
for bit, between guard bands and over poison (tests/views.py); the object against the float64 reference; the route behind
the neck and inside a forward against the stand-alone entry points, bit for bit."""
import ctypes

import numpy as np
import pytest

import views as V
import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import keypoint as KP
from resnet_c_amd import mask as MK
from resnet_c_amd import ops
from resnet_c_amd import roi as RO
from resnet_c_amd import weights as W
from test_detect_gpu import model_head, same, same_entry
from test_dilation_gpu import tol_f32
from test_fpn_gpu import SIZE, WIDTH, images, launches, nets  # noqa: F401  (nets: a fixture)
from test_keypoint_host import EDGE_OUT, EDGE_SIZE, edge_boxes, gaussian_heat, heat_bound, panel_case, same_bits
from test_mask_gpu import MASKS, model_mask
from test_rpn_gpu import model_rpn

pytestmark = pytest.mark.gpu

F = np.float32
H2K, PRED = "rn_heatmaps_to_keypoints_forward", "rn_keypoint_predict_forward"


# =====================================================================================================================
# 1. the search on a caller's heat maps
# =====================================================================================================================
def run_search(heat, boxes, labels, size, koff=0, soff=0):
    K, Kp, S = heat.shape[:3]
    vh, vb = V.place(heat), V.place(boxes)
    vl = V.place(labels) if labels is not None else None
    vk, vs = V.place_out(K * Kp * 12, koff), V.place_out(K * Kp * 4, soff)
    n0 = launches()
    V.must(H2K, vh.ptr, vb.ptr, vl.ptr if vl else None, K, Kp, S, size[0], size[1], vk.ptr, vs.ptr)
    assert launches() == n0 + 1
    V.check_guards(H2K + " inputs", vh, vb, vl)
    what = f"S={S} Kp={Kp} offsets {koff}, {soff}"
    return (V.fetch(vk, F, "keypoints " + what, written=True).reshape(K, Kp, 3),
            V.fetch(vs, F, "scores " + what, written=True).reshape(K, Kp))


def edge_case(S, Kp):
    """the host test's edge rows; maps 1 and 2 of every row are a constant and (S > 1) a map whose first value is a NaN"""
    boxes, labels, what = edge_boxes()
    heat = gaussian_heat(len(boxes), Kp, S, seed=S + Kp)
    if Kp >= 3:
        heat[:, 1] = 0.0
        heat[:, 2, 0, 0] = np.nan
    return heat, boxes, labels


@pytest.mark.parametrize("Kp", [1, 3, 17])
@pytest.mark.parametrize("S", [1, 4, 8, 56])
def test_search_is_the_contract_bit_for_bit(S, Kp):
    heat, boxes, labels = edge_case(S, Kp)
    kps, scores = run_search(heat, boxes, labels, EDGE_SIZE)
    want_k, want_s = KP.heatmaps_to_keypoints_ref(heat, boxes, EDGE_SIZE, labels)
    assert same_bits(kps, want_k) and same_bits(scores, want_s)
    assert not kps[list(EDGE_OUT)].any() and not scores[list(EDGE_OUT)].any()
    live = [k for k in range(len(boxes)) if k not in EDGE_OUT]
    assert np.all(kps[live][..., 2] == 1.0)
    if Kp >= 3:
        assert np.isnan(scores[4, 2]), "enlarged, pixel (0, 0) reads tap (0, 0): a NaN at index 0 stays"
        assert not scores[live, 1].any(), "a constant map of zeros: index 0 wins"
    # position independence: the same rows at another row offset inside a larger K
    K = len(boxes)
    big_h = np.concatenate([gaussian_heat(7, Kp, S, seed=99), heat])
    big_b = np.concatenate([np.tile(np.array([[1.0, 2.0, 50.0, 40.0]], F), (7, 1)), boxes])
    big_l = np.concatenate([np.ones(7, np.int32), labels])
    again_k, again_s = run_search(big_h, big_b, big_l, EDGE_SIZE)
    assert same_bits(again_k[7:], kps) and same_bits(again_s[7:], scores) and K == len(again_k) - 7
    if S == 8 and Kp == 3:
        got = ops.heatmaps_to_keypoints(heat, boxes, EDGE_SIZE, labels)
        assert same_bits(got[0], kps) and same_bits(got[1], scores)
        nolab = run_search(heat, boxes, None, EDGE_SIZE)
        want = KP.heatmaps_to_keypoints_ref(heat, boxes, EDGE_SIZE)
        assert same_bits(nolab[0], want[0]) and same_bits(nolab[1], want[1]) and nolab[0][9].any()


@pytest.mark.parametrize("off", [0, 4, 8, 12])
def test_search_output_offsets(off):
    heat, boxes, labels = edge_case(8, 3)
    want_k, want_s = KP.heatmaps_to_keypoints_ref(heat, boxes, EDGE_SIZE, labels)
    kps, scores = run_search(heat, boxes, labels, EDGE_SIZE, koff=off, soff=(off + 4) % 16)
    assert same_bits(kps, want_k) and same_bits(scores, want_s)


def test_search_refusals_launch_nothing():
    heat, boxes, labels = edge_case(8, 3)
    K = len(boxes)
    vh, vb, vl = V.place(heat), V.place(boxes), V.place(labels)
    vk, vs = V.place_out(K * 3 * 12), V.place_out(K * 3 * 4)
    good = dict(h=vh.ptr, b=vb.ptr, l=vl.ptr, K=K, Kp=3, S=8, mh=240, mw=320, k=vk.ptr, s=vs.ptr)

    def call(**kw):
        a = {**good, **kw}
        return V.call(H2K, a["h"], a["b"], a["l"], a["K"], a["Kp"], a["S"], a["mh"], a["mw"], a["k"], a["s"])

    n0 = launches()
    for kw, text in ((dict(S=0), "S must be"), (dict(S=65), "S must be"), (dict(Kp=0), "Kp must be"), (dict(Kp=257), "Kp must be"),
                     (dict(mh=0), "max_h and max_w"), (dict(mw=8193), "max_h and max_w"), (dict(K=1 << 24), "K must be"),
                     (dict(h=None), "heat is NULL"), (dict(b=None), "boxes is NULL"), (dict(k=None), "keypoints is NULL"),
                     (dict(s=None), "scores is NULL"), (dict(k=vk.ptr + 2), "keypoints is off"), (dict(h=vh.ptr + 1), "heat is off"),
                     (dict(s=vh.ptr), "overlaps"), (dict(k=vb.ptr), "overlaps"), (dict(k=vs.ptr), "overlaps")):
        st, msg = call(**kw)
        assert st == L.RN_ERR_INVALID and text in msg, (kw, st, msg)
    assert call(K=0)[0] == L.RN_OK and launches() == n0, "a refusal launches nothing"
    V.assert_untouched(vk, "refused calls")
    V.assert_untouched(vs, "refused calls")


# =====================================================================================================================
# 2. the predict launch
# =====================================================================================================================
def run_predict(t, bias, boxes, labels, size, heat=True, kps=True):
    K, M, Kp = t.shape[0], t.shape[1], bias.size
    S = 4 * M
    vt, vbias, vb, vl = V.place(t), V.place(bias), V.place(boxes), V.place(labels)
    vh = V.place_out(K * Kp * S * S * 4) if heat else None
    vk, vs = (V.place_out(K * Kp * 12), V.place_out(K * Kp * 4)) if kps else (None, None)
    n0 = launches()
    V.must(PRED, vt.ptr, vbias.ptr, vb.ptr, vl.ptr, K, M, Kp, size[0], size[1], vh.ptr if vh else None, vk.ptr if vk else None,
           vs.ptr if vs else None)
    assert launches() == n0 + 1, "one launch"
    V.check_guards(PRED + " inputs", vt, vbias, vb, vl)
    what = f"M={M} Kp={Kp}"
    return (V.fetch(vh, F, "heat " + what, written=True).reshape(K, Kp, S, S) if heat else None,
            V.fetch(vk, F, "keypoints " + what, written=True).reshape(K, Kp, 3) if kps else None,
            V.fetch(vs, F, "scores " + what, written=True).reshape(K, Kp) if kps else None)


@pytest.mark.parametrize("Kp", [1, 3, 17])
@pytest.mark.parametrize("M", [1, 2, 14])
def test_predict_is_the_contract_bit_for_bit(M, Kp):
    boxes, labels, _ = edge_boxes()
    K = len(boxes)
    t, bias = panel_case(Kp, M, K, seed=5)
    heat, kps, scores = run_predict(t, bias, boxes, labels, EDGE_SIZE)
    assert same_bits(heat, KP.heatmaps_ref(t, bias)), "heat is not heatmaps_ref's bits"
    again_k, again_s = run_search(heat, boxes, labels, EDGE_SIZE)
    assert same_bits(kps, again_k) and same_bits(scores, again_s), "the search on the device's heat map gives other bits"
    want_k, want_s = KP.heatmaps_to_keypoints_ref(heat, boxes, EDGE_SIZE, labels)
    assert same_bits(kps, want_k) and same_bits(scores, want_s)
    _, only_k, only_s = run_predict(t, bias, boxes, labels, EDGE_SIZE, heat=False)      # no heat map reaches memory
    assert same_bits(only_k, kps) and same_bits(only_s, scores)
    only_h, _, _ = run_predict(t, bias, boxes, labels, EDGE_SIZE, kps=False)
    assert same_bits(only_h, heat)
    if M == 2 and Kp == 3:
        got = ops.keypoint_predict(t, bias, boxes, EDGE_SIZE, labels)
        assert same_bits(got[0], heat) and same_bits(got[1], kps) and same_bits(got[2], scores)


def test_predict_refusals_launch_nothing():
    boxes, labels, _ = edge_boxes()
    K, M, Kp = len(boxes), 2, 3
    t, bias = panel_case(Kp, M, K)
    vt, vbias, vb, vl = V.place(t), V.place(bias), V.place(boxes), V.place(labels)
    vh, vk, vs = V.place_out(K * Kp * 64 * 4), V.place_out(K * Kp * 12), V.place_out(K * Kp * 4)
    good = dict(t=vt.ptr, bias=vbias.ptr, b=vb.ptr, l=vl.ptr, K=K, M=M, Kp=Kp, mh=240, mw=320, h=vh.ptr, k=vk.ptr, s=vs.ptr)

    def call(**kw):
        a = {**good, **kw}
        return V.call(PRED, a["t"], a["bias"], a["b"], a["l"], a["K"], a["M"], a["Kp"], a["mh"], a["mw"], a["h"], a["k"], a["s"])

    n0 = launches()
    for kw, text in ((dict(M=0), "M must be"), (dict(M=17), "M must be"), (dict(Kp=0), "Kp must be"), (dict(Kp=257), "Kp must be"),
                     (dict(mh=8193), "max_h and max_w"), (dict(mw=0), "max_h and max_w"), (dict(h=None, k=None, s=None), "all NULL"),
                     (dict(s=None), "come together"), (dict(k=None), "come together"), (dict(t=None), "t is NULL"),
                     (dict(bias=None), "bias is NULL"), (dict(b=None), "boxes is NULL"), (dict(t=vt.ptr + 4), "t is off a 16-byte"),
                     (dict(h=vh.ptr + 2), "heat is off"), (dict(h=vt.ptr), "overlaps"), (dict(k=vh.ptr), "overlaps"),
                     (dict(s=vb.ptr), "overlaps")):
        st, msg = call(**kw)
        assert st == L.RN_ERR_INVALID and text in msg, (kw, st, msg)
    assert call(K=0)[0] == L.RN_OK and launches() == n0, "a refusal launches nothing"
    for v in (vh, vk, vs):
        V.assert_untouched(v, "refused calls")


# =====================================================================================================================
# 3. the object
# =====================================================================================================================
@pytest.mark.parametrize("in_channels,layers,Kp,M", [(64, (64,), 3, 2), (256, (256,) * 2, 17, 14)])
def test_object_against_float64(in_channels, layers, Kp, M):
    """The heat map against keypoint_head_ref.  The bound accumulates layer by layer as the mask head's does: a layer
    amplifies its input's error by at most the largest L1 norm of a row of its weights and adds its own
    tol_f32(output, products); ReLU moves no two values apart.  The panel likewise; its error e_t per tap goes through the
    overlap-add and the resize as at most four taps per pixel under a convex combination: 4 e_t, plus heat_bound of the
    float64 panel output.  The keypoints: the contract on the device's own heat map, bit for bit."""
    K = 6
    st = KP.generate_keypoint_head_state(in_channels, layers, Kp, seed=M)
    g = np.random.default_rng(in_channels + M)
    pooled = np.maximum(g.standard_normal((K, in_channels, M, M)), 0).astype(F)
    labels = np.array([1, 1, -1, 1, 1, 1], np.int32)
    boxes = np.array([[1.5, 2.0, 30.0, 60.0], [0, 0, 40, 72], [1, 1, 9, 9], [3, 3, 3.5, 3.25], [2, 1, 12, 8], [5.25, 4.5, 37.0, 19.75]], F)
    kh = R.KeypointHead(in_channels, layers, Kp, {"roi_heads." + k: v for k, v in st.items()}, resolution=M)
    kh.poison = True
    nhwc = np.ascontiguousarray(pooled.transpose(0, 2, 3, 1))
    try:
        n0 = launches()
        out = kh(nhwc, labels, boxes, SIZE, keypoints=("keypoints", "heatmaps"))
        n = len(layers) + 1
        assert n + 1 <= launches() - n0 <= 2 * n + 1, "n_layers + 1 contractions of one or two launches and ONE predict launch"
        for k, v in out.items():
            V.check_written(np.ascontiguousarray(v).view(np.uint8), v.dtype.itemsize, k)
        heat = out["keypoint_heatmaps"][0]
        outs = KP.keypoint_head_ref(pooled, st, layers=True)
        l1 = lambda w: np.abs(w.reshape(w.shape[0], -1)).sum(axis=1).max()  # noqa: E731
        e, cin, x = 0.0, in_channels, pooled.astype(np.float64)
        for i, c in enumerate(layers):
            e = e * l1(st[f"keypoint_head.{2 * i}.weight"].astype(np.float64)) + tol_f32(outs[i], 9 * cin)
            cin, x = c, outs[i]
        rows = KP.deconv_panel(st[KP.PREDICTOR_KEYS[0]].astype(np.float64))
        t64 = np.einsum("kchw,oc->khwo", x, rows, optimize=True)
        e_t = e * l1(rows) + tol_f32(t64, cin)
        bound = 4 * e_t + heat_bound(t64, st[KP.PREDICTOR_KEYS[1]])
        err = np.abs(heat.astype(np.float64) - outs[-1])
        print(f"\n  keypoint head in {in_channels} layers {layers} Kp {Kp} M {M}: heat error {err.max():.3e}, largest share of the "
              f"bound {float((err / bound).max()):.3e}")
        assert (err <= bound).all(), float((err / bound).max())
        want_k, want_s = KP.heatmaps_to_keypoints_ref(heat, boxes, SIZE, labels)
        assert same_bits(out["keypoints"][0], want_k) and same_bits(out["keypoints_scores"][0], want_s)
        assert not out["keypoints"][0][2].any() and (out["keypoints"][0][[0, 1, 3, 4, 5], :, 2] == 1).all()
        only = kh(nhwc, labels, boxes, SIZE)                                               # no heat map reaches memory
        assert sorted(only) == ["keypoints", "keypoints_scores"] and same_bits(only["keypoints"], out["keypoints"])
        assert same_bits(kh(nhwc, keypoints=("heatmaps",))["keypoint_heatmaps"][0], heat)   # no boxes, no labels: heat alone
    finally:
        kh.close()


def test_object_refusals_and_scratch_growth_under_a_graph():
    lib, ctx = L.lib(), R.get_ctx()
    h = ctypes.c_void_p()
    u64s = lambda *v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731
    n0 = launches()
    for args in ((100, 1, u64s(64), 3, 2), (64, 0, u64s(64), 3, 2), (64, 9, u64s(*[64] * 9), 3, 2), (64, 1, u64s(96), 3, 2),
                 (64, 1, u64s(64), 0, 2), (64, 1, u64s(64), 257, 2), (64, 1, u64s(64), 3, 0), (64, 1, u64s(64), 3, 17), (64, 1, None, 3, 2)):
        assert lib.rn_keypoint_head_create(ctx.handle, ctypes.byref(h), *args) == L.RN_ERR_INVALID, args[:2] + args[3:]
    assert lib.rn_keypoint_head_create(ctx.handle, ctypes.byref(h), 64, 1, u64s(64), 3, 2) == L.RN_OK
    w = np.zeros(64 * 64 * 9, F)
    assert lib.rn_keypoint_head_set_tensor(h, b"keypoint_head.0.weight", w.ctypes.data, w.size) == L.RN_OK
    assert lib.rn_keypoint_head_set_tensor(h, b"roi_heads.keypoint_head.0.bias", w.ctypes.data, 64) == L.RN_OK
    assert lib.rn_keypoint_head_set_tensor(h, b"keypoint_head.0.bias", w.ctypes.data, 63) == L.RN_ERR_INVALID
    assert b"has 63 elements, not 64" in lib.rn_last_error(ctx.handle)
    assert lib.rn_keypoint_head_set_tensor(h, b"keypoint_head.2.weight", w.ctypes.data, w.size) == L.RN_ERR_INVALID   # one layer only
    assert lib.rn_keypoint_head_set_tensor(h, b"keypoint_head.1.weight", w.ctypes.data, w.size) == L.RN_ERR_INVALID   # a ReLU
    assert b"unknown key" in lib.rn_last_error(ctx.handle)
    assert lib.rn_keypoint_head_finalize(h) == L.RN_ERR_INVALID
    assert b"keypoint_predictor.kps_score_lowres.weight is not set" in lib.rn_last_error(ctx.handle)
    assert launches() == n0, "a refusal launches nothing"
    assert lib.rn_keypoint_head_destroy(h) == L.RN_OK
    kh = R.KeypointHead(64, (64,), 3, KP.generate_keypoint_head_state(64, (64,), 3, seed=1), resolution=2)
    m = R.NativeModel("resnet18", state=W.generate_state("resnet18", seed=1), input_size=(32, 32))
    g = None
    try:
        K = 4
        pooled, labels, boxes = V.place(np.zeros((K + 2, 2, 2, 64), F)), V.place(np.ones(K + 2, np.int32)), V.place(np.ones((K + 2, 4), F))
        spec, bufs = kh.buffers(1, K + 2, ("keypoints", "heatmaps"))

        def fwd(q, p=pooled.ptr, l=labels.ptr, b=boxes.ptr, image=SIZE, K=K):
            s = lib.rn_keypoint_head_forward(kh.handle, p, l, b, K, image[0], image[1], ctypes.byref(q) if q is not None else None)
            return s, (lib.rn_last_error(ctx.handle) or b"").decode()

        def req(**kw):
            q = kh.request(bufs)
            for k, v in kw.items():
                setattr(q, k, v)
            return q

        n0 = launches()
        cases = [(fwd(None), "request is NULL"), (fwd(req(heat=None, keypoints=None, scores=None)), "all NULL"),
                 (fwd(req(scores=None)), "come together"), (fwd(req(), b=None), "boxes is NULL"), (fwd(req(), p=None), "pooled_nhwc is NULL"),
                 (fwd(req(), p=pooled.ptr + 4), "16-byte"), (fwd(req(), image=(0, 5)), "max_h and max_w"),
                 (fwd(req(), image=(5, 8193)), "max_h and max_w"), (fwd(req(heat=pooled.ptr)), "overlaps"),
                 (fwd(req(scores=bufs["keypoints"].ptr + 4)), "overlaps"), (fwd(req(keypoints=bufs["keypoints"].ptr + 2)), "keypoints is off")]
        for i, ((s, msg), text) in enumerate(cases):
            assert s == L.RN_ERR_INVALID and text in msg, (i, s, msg, text)
        assert fwd(req(), K=0)[0] == L.RN_OK
        assert launches() == n0, "a refusal launches nothing"
        # the scratch: reserved for K rows; while a captured graph of the context lives it does not grow
        x = W.generate_input(1, seed=7, hw=(32, 32))
        m.forward(x, fused=True)
        xd, out = R.FloatTensor.from_numpy(x, R.Device.GPU), R.FloatTensor((1, 1000), R.Device.GPU)
        s, msg = fwd(req())
        assert s == L.RN_OK, msg
        ctx.sync()
        assert launches() > n0
        g = R.Graph(m, xd.data(), 1, out.data(), True)
        n0 = launches()
        s, msg = fwd(req(), K=K + 2)
        assert s == L.RN_ERR_INVALID and msg.endswith("rn_keypoint_head: the scratch cannot grow while a captured graph lives"), (s, msg)
        assert launches() == n0, "a refusal launches nothing"
        g.close()
        g = None
        s, msg = fwd(req(), K=K + 2)
        assert s == L.RN_OK, msg
        ctx.sync()
    finally:
        if g is not None:
            g.close()
        m.close()
        kh.close()


# =====================================================================================================================
# 4. behind the neck and inside a forward
# =====================================================================================================================
KPS = ("keypoints", "heatmaps", "rois", "pooled")
KP_KEYS = ("keypoint_rois", "keypoint_pooled", "keypoint_heatmaps", "keypoints", "keypoints_scores")
KM, KN = 2, 3     # the resolution and the keypoints of the model tests' heads


def model_keypoint(arch, in_channels=None):
    a = in_channels or WIDTH[arch]
    kh = R.KeypointHead(a, (64,), KN, KP.generate_keypoint_head_state(a, (64,), KN, seed=9), resolution=KM)
    kh.poison = True
    return kh


def check_keypoints(got, kh, levels=None):
    """keypoint_rois is the contract on the call's own detections; keypoint_pooled is ops.roi_align_nhwc on the exported
    levels (where the call exported them); every other entry is the stand-alone KeypointHead run on that pooled, the
    labels and the boxes, bit for bit; no output keeps its poison"""
    for k in KP_KEYS:
        V.check_written(np.ascontiguousarray(got[k]).view(np.uint8), got[k].dtype.itemsize, k)
    assert same(got["keypoint_rois"], MK.detection_rois_ref(got["boxes"], got["labels"]))
    if levels is not None:
        maps = [np.ascontiguousarray(got[k].transpose(0, 2, 3, 1)) for k in levels]
        scales = RO.infer_scales([m.shape[1:3] for m in maps], SIZE)
        want = ops.roi_align_nhwc(maps, got["keypoint_rois"], scales, KM, kh.pooler.sampling_ratio, False, kh.pooler.thresholds(scales),
                                  validate=False)
        assert same(got["keypoint_pooled"], want)
    alone = kh(got["keypoint_pooled"], got["labels"].reshape(-1), got["boxes"].reshape(-1, 4), SIZE, keypoints=("keypoints", "heatmaps"))
    for k in ("keypoint_heatmaps", "keypoints", "keypoints_scores"):
        assert same_entry(got[k], alone[k].reshape(got[k].shape)), k
    want_k, want_s = KP.heatmaps_to_keypoints_ref(got["keypoint_heatmaps"].reshape((-1,) + got["keypoint_heatmaps"].shape[2:]),
                                                  got["boxes"].reshape(-1, 4), SIZE, got["labels"].reshape(-1))
    assert same_bits(got["keypoints"].reshape(want_k.shape), want_k) and same_bits(got["keypoints_scores"].reshape(want_s.shape), want_s)
    none = got["labels"] < 1
    assert not got["keypoints"][none].any() and not got["keypoints_scores"][none].any()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_model_route_bit_for_bit(nets, arch, dtype):
    m, neck = nets(arch, dtype)
    x = np.array(images())
    net, bh, mh, kh = model_rpn(arch), model_head(arch), model_mask(arch), model_keypoint(arch)
    pooler = RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2)
    kw = dict(rpn=net, pooler=pooler, box_head=bh, detect_intermediates=True)
    try:
        n0 = launches()
        plain = m.forward_fpn(x, neck, roi_levels=True, candidates=True, **kw)
        n1 = launches()
        masked = m.forward_fpn(x, neck, roi_levels=True, candidates=True, mask_head=mh, masks=MASKS, mask_pooled=True, **kw)
        n2 = launches()
        got = m.forward_fpn(x, neck, roi_levels=True, candidates=True, keypoint_head=kh, keypoints=KPS, **kw)
        n3 = launches()
        both = m.forward_fpn(x, neck, roi_levels=True, candidates=True, mask_head=mh, masks=MASKS, mask_pooled=True, keypoint_head=kh,
                             keypoints=KPS, **kw)
        n4 = launches()
        again = m.forward_fpn(x, neck, roi_levels=True, candidates=True, **kw)
        assert launches() - n4 == n1 - n0, "every other forward kind issues the launches it issued"
        added = (n3 - n2) - (n1 - n0)
        assert 2 + 2 + 1 <= added <= 2 + 4 + 1, "the RoI former, the pooler, two contractions of one or two launches, ONE predict launch"
        assert (n4 - n3) - (n2 - n1) == added, "the same stage behind a mask head"
        for k in plain:
            assert same_entry(plain[k], got[k]) and same_entry(plain[k], again[k]), k
        for k in masked:
            assert same_entry(masked[k], both[k]), k
        assert sorted(set(got) - set(plain)) == sorted(KP_KEYS) and sorted(set(both) - set(masked)) == sorted(KP_KEYS)
        for k in KP_KEYS:
            assert same_entry(got[k], both[k]), k
        check_keypoints(got, kh, levels=("0", "1", "2", "3"))
        assert got["detections"].max() > 0 and got["keypoints"].any()
        few = m.forward_fpn(x, neck, levels=(), keypoint_head=kh, **kw)               # keypoints alone: rois, pooled, heat nowhere
        assert sorted(k for k in few if k.startswith("keypoint")) == ["keypoints", "keypoints_scores"]
        assert same_entry(few["keypoints"], got["keypoints"]) and same_entry(few["keypoints_scores"], got["keypoints_scores"])
        if dtype == "f32" and arch == "resnet18":
            px = np.random.default_rng(9).integers(0, 256, (2,) + SIZE + (3,), dtype=np.uint8)
            from resnet_c_amd import preprocess
            u8 = m.forward_fpn_u8(px, neck, keypoint_head=kh, keypoints=KPS, **kw)
            fl = m.forward_fpn(preprocess.normalize_u8(px), neck, keypoint_head=kh, keypoints=KPS, **kw)
            for k in KP_KEYS + ("boxes", "labels"):
                assert same_entry(u8[k], fl[k]), k
            check_keypoints(u8, kh, levels=("0", "1", "2", "3"))
            # the neck route: the same stage behind rn_fpn_forward_keypoints on the exported stage maps
            maps = m.forward_maps(x, R.NativeModel.STAGES)
            nhwc = [np.ascontiguousarray(maps[s].transpose(0, 2, 3, 1)) for s in R.NativeModel.STAGES]
            via = neck.forward(nhwc, image_size=SIZE, keypoint_head=kh, keypoints=KPS, **kw)
            check_keypoints(via, kh, levels=("0", "1", "2", "3"))
            via2 = neck.forward(nhwc, image_size=SIZE, mask_head=mh, masks=MASKS, keypoint_head=kh, keypoints=KPS, **kw)
            for k in KP_KEYS:
                assert same_entry(via[k], via2[k]), k
            assert via["detections"].max() > 0 and via["keypoints"].any() and via2["masks"].any()
    finally:
        net.close()
        bh.close()
        mh.close()
        kh.close()


def test_model_parts_sub_batches_and_profile(nets):
    """128 images as two parts on two streams, then one image more than a launch batch holds: every part runs the stage on
    its own detection rows and writes its own images' rows; the bits are those of one stream; one keypoint_stage record per
    part in the profile, behind the mask head's"""
    m, neck = nets()
    x = W.generate_input(128, seed=300 + SIZE[0] + SIZE[1], hw=SIZE)
    net, bh, kh, pooler = model_rpn("resnet50"), model_head("resnet50"), model_keypoint("resnet50"), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2)
    kw = dict(levels=(), rpn=net, pooler=pooler, box_head=bh, keypoint_head=kh, keypoints=KPS)
    try:
        m.set_streams(1)
        one = m.forward_fpn(x, neck, **kw)
        m.set_streams(2)
        assert m.parts(128) == 2
        two = m.forward_fpn(x, neck, **kw)
        m.set_streams(0)
        for k in KP_KEYS:
            V.check_written(np.ascontiguousarray(two[k]).view(np.uint8), two[k].dtype.itemsize, k)
            assert same_entry(one[k], two[k]), k
        assert same(two["keypoint_rois"], MK.detection_rois_ref(two["boxes"], two["labels"]))
        assert two["keypoints"][64:].any() and two["keypoints"][:64].any()
    finally:
        m.set_streams(0)
        net.close()
        bh.close()
        kh.close()
    m18, neck18 = nets("resnet18")
    net18, bh18, mh18, kh18 = model_rpn("resnet18", post=20), model_head("resnet18", D_=4), model_mask("resnet18"), model_keypoint("resnet18")
    kw = dict(levels=(), rpn=net18, pooler=pooler, box_head=bh18, keypoint_head=kh18, keypoints=("keypoints", "heatmaps", "rois"))
    try:
        m18.set_input_size(32, 32)
        cap = m18.max_sub_batch()
        x = W.generate_input(cap + 1, seed=43, hw=(32, 32))
        whole = m18.forward_fpn(x, neck18, **kw)
        for k in ("keypoint_rois", "keypoint_heatmaps", "keypoints", "keypoints_scores"):
            V.check_written(np.ascontiguousarray(whole[k]).view(np.uint8), whole[k].dtype.itemsize, k)
        pick = [0, 1, cap - 1, cap]
        few = m18.forward_fpn(x[pick], neck18, **kw)
        for k in ("keypoint_heatmaps", "keypoints", "keypoints_scores"):
            assert same_entry(whole[k][pick], few[k]), k
        assert few["keypoints"].any()
        m18.set_profiling(True)
        m18.forward_fpn(x[:2], neck18, mask_head=mh18, masks=("probs",), **kw)
        recs = [(r["layer"], r["op"]) for r in m18.profile() if r["layer"] in ("fpn", "rpn", "roi_heads")]
        assert recs.count(("roi_heads", "keypoint_stage")) == 1 and recs[-1] == ("roi_heads", "keypoint_stage")
        assert recs[-2] == ("roi_heads", "mask_stage") and recs[-3] == ("roi_heads", "box_stage")
    finally:
        m18.set_profiling(False)
        m18.set_input_size(*SIZE)
        net18.close()
        bh18.close()
        mh18.close()
        kh18.close()


def test_model_draw_with_no_detection_beside_full_images(nets):
    """test_detect_gpu's draw: two images of zeros among 126 others under a head that turns every proposal of a zero image
    down.  Their detection rows are padding: their RoI rows are (-1, 0, 0, 0, 0), their pooled features zeros, their
    keypoints and scores zeros, written by the part that holds them beside a neighbour's keypoints."""
    from resnet_c_amd import detection as D
    from test_detect_gpu import MC, MREP
    m, neck = nets()
    x = W.generate_input(128, seed=300 + SIZE[0] + SIZE[1], hw=SIZE)
    x[3] = 0
    x[70] = 0
    st = D.generate_box_head_state(WIDTH["resnet50"] * 4, MREP, MC, seed=6)
    st["box_head.fc6.bias"][:] = 0
    st["box_head.fc7.bias"][:] = 0
    st["box_predictor.cls_score.bias"][:] = [4, 0, 0, 0, 0]
    net, pooler, kh = model_rpn("resnet50"), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2), model_keypoint("resnet50")
    bh = R.BoxHead(WIDTH["resnet50"], 2, MREP, MC, st, detections_per_img=4)
    bh.poison = True
    try:
        m.set_streams(2)
        assert m.parts(128) == 2
        got = m.forward_fpn(x, neck, levels=(), rpn=net, pooler=pooler, box_head=bh, keypoint_head=kh, keypoints=KPS)
        m.set_streams(0)
        zero = np.zeros(128, bool)
        zero[[3, 70]] = True
        assert (got["detections"][zero] == 0).all() and (got["detections"][~zero] == 4).all(), got["detections"].tolist()
        check_keypoints(got, kh)
        rois = got["keypoint_rois"].reshape(128, 4, 5)
        assert (rois[zero, :, 0] == -1).all() and not rois[zero, :, 1:].any() and (rois[~zero, :, 0] == np.arange(128)[~zero, None]).all()
        for k in ("keypoints", "keypoints_scores"):
            assert not got[k][zero].any() and got[k][~zero].any(), k
        assert not got["keypoint_pooled"].reshape(128, -1)[zero].any()
        assert all((got["keypoints"][b][..., 2] == 1).all() for b in (2, 4, 69, 71))
    finally:
        m.set_streams(0)
        net.close()
        bh.close()
        kh.close()


def test_model_route_refusals(nets):
    m, neck = nets("resnet18")
    x = np.array(images())
    net, bh, kh, pooler = model_rpn("resnet18"), model_head("resnet18"), model_keypoint("resnet18"), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2)
    wide = model_keypoint("resnet18", in_channels=128)
    kw = dict(rpn=net, pooler=pooler, box_head=bh)
    box_request, kp_request = bh.request, kh.request

    def without(name):
        def request(bufs):
            q = box_request(bufs)
            setattr(q.out, name, None)
            return q
        return request

    def sharing(bufs, names=None):
        q = kp_request(bufs, names)
        q.heat = bufs["keypoints"].ptr
        return q

    def nothing(bufs, names=None):
        q = kp_request(bufs, names)
        q.heat = q.keypoints = q.scores = None
        return q

    def on_the_boxes(bufs, names=None):
        q = kp_request(bufs, names)
        q.scores = on_the_boxes.boxes
        return q

    try:
        n0 = launches()
        with pytest.raises(ValueError, match="box_head"):
            m.forward_fpn(x, neck, rpn=net, pooler=pooler, keypoint_head=kh)
        for name in ("boxes", "labels"):
            bh.request = without(name)
            with pytest.raises(L.RnError, match="boxes and labels"):
                m.forward_fpn(x, neck, keypoint_head=kh, **kw)
        bh.request = box_request
        kh.request = sharing
        with pytest.raises(L.RnError, match="overlaps"):
            m.forward_fpn(x, neck, keypoint_head=kh, keypoints=("keypoints", "heatmaps"), **kw)
        kh.request = nothing
        with pytest.raises(L.RnError, match="all NULL"):
            m.forward_fpn(x, neck, keypoint_head=kh, **kw)
        spec, dbufs = bh.buffers(x.shape[0], 60)
        bh.buffers = lambda *a, **k: (spec, dbufs)
        on_the_boxes.boxes = dbufs["boxes"].ptr
        kh.request = on_the_boxes
        with pytest.raises(L.RnError, match="overlaps"):
            m.forward_fpn(x, neck, keypoint_head=kh, **kw)
        del bh.buffers
        kh.request = kp_request
        with pytest.raises(L.RnError, match="in_channels"):
            m.forward_fpn(x, neck, keypoint_head=wide, **kw)
        with pytest.raises(ValueError, match="unknown keypoint output"):
            m.forward_fpn(x, neck, keypoint_head=kh, keypoints=("pixels",), **kw)
        assert launches() == n0, "a refusal launches nothing"
        assert m.forward_fpn(x, neck, levels=(), keypoint_head=kh, **kw)["keypoints"].any()
    finally:
        bh.request, kh.request = box_request, kp_request
        net.close()
        bh.close()
        kh.close()
        wide.close()
