"""The box head behind the pooler on the GPU: the post-processing alone on views between guard bands -- outputs pre-filled
with 0xA5 and checked written everywhere -- against the numpy statement of the contract (resnet_c_amd/detection.py).
The probabilities are compared bit for bit with ops.softmax, the class boxes with the float64 decode within
test_rpn_host.decode_bound, and everything behind them bit for bit on the probabilities and boxes the device itself
returned.  Then the object against float64 and the model route against the stand-alone launches."""
import ctypes

import numpy as np
import pytest

import views as V
import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import detection as D
from resnet_c_amd import ops, rpn
from test_detect_host import IMAGE, detect_case
from test_dilation_gpu import bits, tol_f32
from test_fpn_gpu import launches
from test_rpn_host import chain_cases, decode_bound

pytestmark = pytest.mark.gpu

F = np.float32
LAUNCHES = 3   # score + decode, per-class sort + NMS, merge: whatever B, R and C
OUT = (("boxes", F, 4), ("scores", F, 1), ("labels", np.int32, 1), ("roi", np.int32, 1))
MID = (("probs", F, 1), ("class_boxes", F, 4), ("valid", np.uint8, 1), ("keep", np.uint8, 1))
ALL = tuple(k for k, _, _ in OUT) + ("count",) + tuple(k for k, _, _ in MID)


def record(line):
    """print a measured error beside its bound and, where RN_DETECT_ERRORS_FILE names a file, append it there: that is
    how profiles/detect/errors_and_bounds.txt is written"""
    import os
    print(line)
    path = os.environ.get("RN_DETECT_ERRORS_FILE")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def out_views(B, Rn, C, Dn, want=None, offs=None):
    offs = offs or {}
    sizes = {k: B * Dn * n * np.dtype(t).itemsize for k, t, n in OUT}
    sizes["count"] = B * 4
    sizes.update({k: B * Rn * C * n * np.dtype(t).itemsize for k, t, n in MID})
    return {k: V.place_out(sizes[k], offs.get(k, 0)) for k in ALL if want is None or k in want}


def request(vo, Dn, st=0.05, nt=0.5, ms=D.MIN_SIZE, wgt=D.BOX_WEIGHTS):
    return D.make_request(vo, st, nt, ms, Dn, wgt)


def fetch_all(vo, B, Rn, C, Dn):
    shapes = {k: (B, Dn) + ((4,) if n == 4 else ()) for k, _, n in OUT}
    shapes["count"] = (B,)
    shapes.update({k: (B * Rn, C) + ((4,) if n == 4 else ()) for k, _, n in MID})
    types = {k: t for k, t, _ in OUT + MID}
    types["count"] = np.int32
    return {k: V.fetch(v, types[k], f"out.{k}", written=True).reshape(shapes[k]) for k, v in vo.items()}


def postprocess(head, rois, B, C, Dn, want=None, offs=None, **kw):
    """ONE rn_detect_postprocess_forward on views: input guards intact, every requested output written everywhere"""
    Rn = head.shape[0] // B
    vh, vr = V.place(head, (offs or {}).get("head", 0)), V.place(rois, (offs or {}).get("rois", 0))
    vo = out_views(B, Rn, C, Dn, want, offs)
    req = request(vo, Dn, **kw)
    n0 = launches()
    V.must("rn_detect_postprocess_forward", vh.ptr, vr.ptr, B, Rn, C, IMAGE[0], IMAGE[1], ctypes.byref(req))
    assert launches() - n0 == LAUNCHES, (B, Rn, C)
    V.check_guards("rn_detect_postprocess_forward inputs", vh, vr)
    return fetch_all(vo, B, Rn, C, Dn)


def same(a, b):
    return np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)


def check_contract(got, head, rois, B, C, Dn, st=0.05, nt=0.5):
    """probs bit for bit ops.softmax; class boxes within the bound; valid, keep and the detections bit for bit the numpy
    contract on the device's own probabilities and boxes.  Returns (the reference, the largest box error / bound)."""
    logits, deltas = D.unpack_head(head, C)
    assert same(got["probs"], ops.softmax(np.ascontiguousarray(logits))), "probs are not rn_softmax_forward's bits"
    worst = 0.0
    assert not got["class_boxes"][:, 0].any()
    for c in range(1, C):
        ref = rpn.decode_f64(rois[:, 1:], deltas[:, c], D.BOX_WEIGHTS, IMAGE)
        err = np.abs(got["class_boxes"][:, c].astype(np.float64) - ref)
        bound = decode_bound(rois[:, 1:], deltas[:, c], D.BOX_WEIGHTS)
        assert (err <= bound).all(), f"class {c}: box error {(err / bound).max():.3f} of the bound"
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    want = D.postprocess_ref(head, rois, B, C, IMAGE, st, nt, Dn, probs=got["probs"], class_boxes=got["class_boxes"])
    for k in ("valid", "keep", "count", "labels", "roi", "scores", "boxes"):
        assert same(got[k], want[k]), (k, B, head.shape[0] // B, C, np.flatnonzero((got[k] != want[k]).reshape(-1))[:8])
    return want, worst


@pytest.mark.parametrize("kind", ["random", "quantised", "special"])
@pytest.mark.parametrize("C", [2, 5, 91])
def test_postprocess_against_the_contract(C, kind):
    """The whole grid of the shapes: B in (1, 3) x R in (1, 2, 63, 64, 65, 100, 1000), for every C and kind.  Over the grid
    of every (C, kind): both outcomes of every clause of Valid, at least one suppressed candidate and at least one chain
    case.  With two classes a probability below 0.05 needs a logit gap of 2.94 against the raised class, so there the
    score threshold is 0.5, which both outcomes straddle."""
    st = 0.5 if C == 2 else 0.05
    seen, suppressed, chains, worst = np.zeros((4, 2), bool), 0, 0, 0.0
    for B in (1, 3):
        for Rn in (1, 2, 63, 64, 65, 100, 1000):
            head, rois = detect_case(3, B, Rn, C, kind)
            Dn = 7 if Rn == 100 else 100
            got = postprocess(head, rois, B, C, Dn, offs={"head": 4, "boxes": 4, "keep": 1, "valid": 3} if Rn == 65 else None, st=st)
            want, w = check_contract(got, head, rois, B, C, Dn, st=st)
            worst = max(worst, w)
            bx, p = got["class_boxes"][:, 1:], got["probs"][:, 1:]
            real = rois[:, 0] == np.repeat(np.arange(B), Rn)
            with np.errstate(invalid="ignore"):
                for i, cl in enumerate((np.broadcast_to(real[:, None], p.shape), p > F(st), bx[..., 2] - bx[..., 0] >= F(1e-2),
                                        bx[..., 3] - bx[..., 1] >= F(1e-2))):
                    seen[i] |= [cl.any(), not cl.all()]
            valid, keep = got["valid"].astype(bool), got["keep"].astype(bool)
            suppressed += int(valid.sum() - keep.sum())
            if Rn in (100, 1000):
                for c in range(1, min(C, 9)):
                    r = np.flatnonzero(valid[:Rn, c])
                    r = r[rpn.select_ref(got["probs"][:Rn, c][r], r.size)]
                    chains += chain_cases(got["class_boxes"][:Rn, c][r], keep[:Rn, c][r], 0.5)
            if Rn == 100 and kind == "random":
                assert (got["count"] == 7).all(), got["count"]
    assert suppressed >= 1 and chains >= 1, (suppressed, chains)
    assert seen.all(), seen.tolist()
    record(f"post-processing C = {C} ({kind}): largest class-box error {worst:.3f} of the decode bound")


def test_postprocess_4096_rois_partial_outputs_and_no_survivor():
    head, rois = detect_case(5, 1, 4096, 5)
    got = postprocess(head, rois, 1, 5, 1024)
    want, w = check_contract(got, head, rois, 1, 5, 1024)
    valid, keep = int(got["valid"].sum()), int(got["keep"].sum())
    assert 0.05 * valid <= keep <= 0.60 * valid and got["count"][0] == min(keep, 1024), (valid, keep)
    record(f"post-processing R = 4096: {valid} valid candidates, {keep} survivors; box error {w:.3f} of the bound")
    # only labels and count: the same as the full call, on 4-byte offsets
    head, rois = detect_case(6, 3, 100, 5)
    full = postprocess(head, rois, 3, 5, 20)
    part = postprocess(head, rois, 3, 5, 20, want=("labels", "count"), offs={"labels": 4, "count": 8, "rois": 4})
    assert sorted(part) == ["count", "labels"] and same(part["labels"], full["labels"]) and same(part["count"], full["count"])
    # a threshold nothing passes gives count 0 and every row padded; one that lets everything through fills D
    none = postprocess(head, rois, 3, 5, 20, st=1.0)
    assert not none["count"].any() and (none["labels"] == -1).all() and (none["roi"] == -1).all()
    assert not none["boxes"].any() and not none["scores"].any() and not none["valid"].any() and not none["keep"].any()
    every = postprocess(head, rois, 3, 5, 20, st=-1.0, nt=2.0)
    check_contract(every, head, rois, 3, 5, 20, st=-1.0, nt=2.0)
    assert (every["count"] == 20).all() and same(every["valid"], every["keep"])
    # one call: an image of padding rows only gives count 0 while its neighbours fill D
    rois1 = rois.copy()
    rois1[100:200] = [-1, 0, 0, 0, 0]
    mixed = postprocess(head, rois1, 3, 5, 5)
    check_contract(mixed, head, rois1, 3, 5, 5)
    assert mixed["count"].tolist() == [5, 0, 5] and (mixed["labels"][1] == -1).all() and not mixed["boxes"][1].any()
    # the Python op: the same three launches
    py = ops.detect_postprocess(head, rois, 3, 5, IMAGE, detections_per_img=20, intermediates=True)
    for k in full:
        assert same(py[k], full[k]), k


def test_refusals_launch_nothing():
    B, Rn, C, Dn = 2, 16, 5, 8
    head, rois = detect_case(0, B, Rn, C)
    vh, vr = V.place(head), V.place(rois)
    vo = out_views(B, Rn, C, Dn)

    def call(h=vh.ptr, r=vr.ptr, B=B, Rn=Rn, C=C, image=IMAGE, req=None, **kw):
        q = req if req is not None else request(vo, kw.pop("Dn", Dn), **kw)
        return V.call("rn_detect_postprocess_forward", h, r, B, Rn, C, image[0], image[1], ctypes.byref(q) if q is not False else None)

    def outs(**kw):
        q = request(vo, Dn)
        for k, v in kw.items():
            setattr(q.out, k, v)
        return q

    only_mid = request({k: vo[k] for k in ("probs", "class_boxes", "valid", "keep")}, Dn)
    n0 = launches()
    refused = [
        (call(req=False), "request is NULL"), (call(Rn=0), "R must be"), (call(Rn=4097), "R must be"), (call(C=1), "C must be"),
        (call(C=1025), "C must be"), (call(Dn=0), "detections_per_img"), (call(Dn=1025), "detections_per_img"),
        (call(st=np.nan), "NaN"), (call(nt=np.nan), "NaN"), (call(ms=np.nan), "NaN"), (call(image=(0, 72)), "image_h"),
        (call(wgt=(10, 10, 0, 5)), "weights"), (call(wgt=(10, np.inf, 5, 5)), "weights"), (call(B=65536), "B must be"),
        (call(req=only_mid), "every output"), (call(h=None), "head is NULL"), (call(r=None), "rois is NULL"),
        (call(h=vh.ptr + 2), "head is off"), (call(req=outs(scores=vo["scores"].ptr + 2)), "out.scores is off"),
        (call(req=outs(labels=vo["boxes"].ptr)), "overlaps"), (call(req=outs(probs=vh.ptr)), "overlaps"),
        (call(req=outs(keep=vo["valid"].ptr + 1)), "overlaps"), (call(req=outs(count=vr.ptr)), "overlaps"),
    ]
    for i, ((st, msg), text) in enumerate(refused):
        assert st == L.RN_ERR_INVALID and text in msg, (i, st, msg, text)
    assert call(B=0)[0] == L.RN_OK
    assert launches() == n0
    for v in vo.values():
        V.assert_untouched(v, "refused calls")
    assert call()[0] == L.RN_OK and launches() - n0 == LAUNCHES
    fetch_all(vo, B, Rn, C, Dn)


# =====================================================================================================================
# the object
# =====================================================================================================================
@pytest.mark.parametrize("in_channels,res,rep", [(64, 2, 64), (256, 7, 1024)])
def test_object_against_float64(in_channels, res, rep):
    """The head output against box_head_ref.  The bound accumulates over the three layers as the RPN object's does: a
    layer amplifies its input's error by at most the largest L1 norm of a row of its weights and adds its own
    tol_f32(output, products); ReLU moves no two values apart."""
    C, B, Rn = 5, 2, 24
    Fi = in_channels * res * res
    st = D.generate_box_head_state(Fi, rep, C, seed=4)
    g = np.random.default_rng(Fi)
    pooled = np.maximum(g.standard_normal((B * Rn, in_channels, res, res)), 0).astype(F)
    _, rois = detect_case(9, B, Rn, C)
    bh = R.BoxHead(in_channels, res, rep, C, {"roi_heads." + k: v for k, v in st.items()}, detections_per_img=10)
    try:
        n0 = launches()
        out = bh(pooled, rois, B, IMAGE, intermediates=True, return_head=True)
        # a contraction is one launch, or two where its plan finishes a chunked K sum in a second pass (12544 -> 1024 on 48 rows)
        assert launches() - n0 == 3 + LAUNCHES if Fi == 256 else 3 + LAUNCHES <= launches() - n0 <= 6 + LAUNCHES
        w64 = [st[k].astype(np.float64) for k in D.HEAD_KEYS]
        x = pooled.reshape(B * Rn, -1).astype(np.float64)
        t6 = np.maximum(x @ w64[0].T + w64[1], 0)
        t7 = np.maximum(t6 @ w64[2].T + w64[3], 0)
        ref = D.box_head_ref(pooled, st, C)
        l1 = lambda w: np.abs(w).sum(axis=1).max()  # noqa: E731
        e6 = tol_f32(t6, Fi)
        e7 = e6 * l1(w64[2]) + tol_f32(t7, rep)
        e_h = e7 * max(l1(w64[4]), l1(w64[6])) + tol_f32(ref, rep)
        err = np.abs(out["head"].astype(np.float64) - ref).max()
        assert err <= e_h, (err, e_h)
        assert not out["head"][:, 5 * C:].any()
        record(f"box head in_features {Fi} representation {rep}: head error {err:.3e}, {err / e_h:.2e} of the bound {e_h:.3e}")
        # behind the head: the stand-alone post-processing of the head output the same call returned, bit for bit
        alone = ops.detect_postprocess(out["head"], rois, B, C, IMAGE, detections_per_img=10, intermediates=True)
        for k, v in alone.items():
            assert same(out[{"count": "detections", "roi": "detection_rois"}.get(k, k)], v), k
        assert out["detections"].max() > 0
    finally:
        bh.close()


def test_object_refusals():
    lib, ctx = L.lib(), R.get_ctx()
    h = ctypes.c_void_p()
    assert lib.rn_box_head_create(ctx.handle, ctypes.byref(h), 100, 64, 5) == L.RN_ERR_INVALID
    assert lib.rn_box_head_create(ctx.handle, ctypes.byref(h), 256, 96, 5) == L.RN_ERR_INVALID
    assert lib.rn_box_head_create(ctx.handle, ctypes.byref(h), 256, 64, 1) == L.RN_ERR_INVALID
    assert lib.rn_box_head_create(ctx.handle, ctypes.byref(h), 256, 64, 5) == L.RN_OK
    w = np.zeros(256 * 64, F)
    assert lib.rn_box_head_set_tensor(h, b"box_head.fc6.weight", w.ctypes.data, w.size) == L.RN_OK
    assert lib.rn_box_head_set_tensor(h, b"box_head.fc6.bias", w.ctypes.data, 63) == L.RN_ERR_INVALID
    assert lib.rn_box_head_set_tensor(h, b"box_head.fc8.weight", w.ctypes.data, 64) == L.RN_ERR_INVALID
    assert lib.rn_box_head_finalize(h) == L.RN_ERR_INVALID and b"is not set" in lib.rn_last_error(ctx.handle)
    assert lib.rn_box_head_destroy(h) == L.RN_OK
    st = D.generate_box_head_state(256, 64, 5, seed=1)
    bh = R.BoxHead(64, 2, 64, 5, st, detections_per_img=4)
    try:
        pooled, rois = V.place(np.zeros((8, 256), F)), V.place(np.zeros((8, 5), F))
        spec, bufs = bh.buffers(2, 4)

        def fwd(q, p=pooled.ptr, r=rois.ptr, image=IMAGE):
            s = lib.rn_box_head_forward(bh.handle, p, r, 2, 4, image[0], image[1], ctypes.byref(q) if q is not None else None, None)
            return s, (lib.rn_last_error(ctx.handle) or b"").decode()

        on_pooled, bad_d = bh.request(bufs), bh.request(bufs)
        on_pooled.out.scores = pooled.ptr
        bad_d.detections_per_img = 0
        n0 = launches()
        cases = [(fwd(None), "request is NULL"), (fwd(bad_d), "detections_per_img"), (fwd(on_pooled), "overlaps"),
                 (fwd(bh.request(bufs), p=None), "pooled is NULL"), (fwd(bh.request(bufs), p=pooled.ptr + 4), "16-byte"),
                 (fwd(bh.request(bufs), image=(0, 5)), "image_h")]
        for i, ((s, msg), text) in enumerate(cases):
            assert s == L.RN_ERR_INVALID and text in msg, (i, s, msg, text)
        assert launches() == n0, "a refusal launches nothing"
        s, msg = fwd(bh.request(bufs))
        assert s == L.RN_OK, msg
        ctx.sync()
    finally:
        bh.close()


# =====================================================================================================================
# the model route
# =====================================================================================================================
from resnet_c_amd import roi as RO  # noqa: E402
from resnet_c_amd import weights as W  # noqa: E402
from test_fpn_gpu import SIZE, WIDTH, images, nets  # noqa: E402,F401  (nets: a fixture)
from test_rpn_gpu import model_rpn  # noqa: E402

DET = ("boxes", "scores", "labels", "detections", "detection_rois")
MIDS = ("probs", "class_boxes", "valid", "keep")
MC, MD, MREP = 5, 10, 64   # classes, detections per image, representation of the model tests' box heads


def model_head(arch, D_=MD, score_thresh=0.05):
    bh = R.BoxHead(WIDTH[arch], 2, MREP, MC, D.generate_box_head_state(WIDTH[arch] * 4, MREP, MC, seed=6), score_thresh=score_thresh,
                   detections_per_img=D_)
    bh.poison = True
    return bh


def same_entry(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_entry(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(same_entry(a[k], b[k]) for k in a)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_detections(got, bh, B, post):
    """the detections of a forward are those of the stand-alone object run on the pooled and rois the same call
    exported, bit for bit, and no output row kept its poison"""
    for k in DET + MIDS:
        V.check_written(np.ascontiguousarray(got[k]).view(np.uint8), got[k].dtype.itemsize, k)
    alone = bh(got["pooled"], got["rois"], B, SIZE, intermediates=True)
    for k in DET + MIDS:
        assert same_entry(got[k], alone[k]), k
    want = D.merge_ref(got["probs"], got["class_boxes"], got["keep"], B, bh.detections_per_img)
    assert same(got["detections"], want["count"]) and same(got["labels"], want["labels"]) and same(got["boxes"], want["boxes"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_model_route_bit_for_bit(nets, arch, dtype):
    m, neck = nets(arch, dtype)
    x = np.array(images())
    B = x.shape[0]
    net, bh, pooler = model_rpn(arch), model_head(arch), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2)
    try:
        n0 = launches()
        plain = m.forward_fpn(x, neck, rpn=net, pooler=pooler, roi_levels=True, candidates=True)
        n1 = launches()
        got = m.forward_fpn(x, neck, rpn=net, pooler=pooler, roi_levels=True, candidates=True, box_head=bh, detect_intermediates=True)
        added = (launches() - n1) - (n1 - n0)
        assert 3 + LAUNCHES <= added <= 6 + LAUNCHES, "the box stage adds three contractions (one or two launches each) and three launches"
        check_detections(got, bh, B, 60)
        assert got["detections"].max() > 0
        record(f"model route {arch} {dtype}: {int(got['valid'].sum())} valid candidates, {int(got['keep'].sum())} survivors, "
               f"counts {got['detections'].tolist()}")
        # every other entry is the same call's without the box head
        got["scores"] = got.pop("proposal_scores")
        for k in plain:
            assert same_entry(plain[k], got[k]), k
        if dtype == "f32" and arch == "resnet18":
            px = np.random.default_rng(9).integers(0, 256, (2,) + SIZE + (3,), dtype=np.uint8)
            from resnet_c_amd import preprocess
            u8 = m.forward_fpn_u8(px, neck, levels=(), rpn=net, pooler=pooler, box_head=bh, detect_intermediates=True)
            fl = m.forward_fpn(preprocess.normalize_u8(px), neck, levels=(), rpn=net, pooler=pooler, box_head=bh, detect_intermediates=True)
            for k in DET + MIDS + ("pooled", "rois"):
                assert same_entry(u8[k], fl[k]), k
            check_detections(u8, bh, 2, 60)
            # the neck route: the same stage behind rn_fpn_forward_detections on the exported stage maps, held to the same
            # statement (its pyramid is computed by other launches than the model's: no bits are shared with `got`)
            maps = m.forward_maps(x, R.NativeModel.STAGES)
            nhwc = [np.ascontiguousarray(maps[s].transpose(0, 2, 3, 1)) for s in R.NativeModel.STAGES]
            via = neck.forward(nhwc, levels=(), rpn=net, image_size=SIZE, pooler=pooler, box_head=bh, detect_intermediates=True)
            check_detections(via, bh, B, 60)
            assert via["detections"].max() > 0
    finally:
        net.close()
        bh.close()


def test_model_parts_sub_batches_and_profile(nets):
    """128 images as two parts on two streams, then one image more than a launch batch holds: every part runs the head on
    its own rows and writes its own images' detections; the bits are those of one stream"""
    m, neck = nets()
    x = W.generate_input(128, seed=300 + SIZE[0] + SIZE[1], hw=SIZE)
    net, bh, pooler = model_rpn("resnet50"), model_head("resnet50"), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2)
    try:
        m.set_streams(1)
        one = m.forward_fpn(x, neck, levels=(), rpn=net, pooler=pooler, box_head=bh, detect_intermediates=True)
        m.set_streams(2)
        assert m.parts(128) == 2
        two = m.forward_fpn(x, neck, levels=("0",), rpn=net, pooler=pooler, box_head=bh, detect_intermediates=True)
        m.set_streams(0)
        for k in DET + MIDS + ("pooled", "rois"):
            V.check_written(np.ascontiguousarray(two[k]).view(np.uint8), two[k].dtype.itemsize, k)
            assert same_entry(one[k], two[k]), k
        part = slice(60 * 64, 60 * 70)           # six images of the second part, alone
        alone = bh(two["pooled"][part], np.concatenate([two["rois"][part, :1] - 64, two["rois"][part, 1:]], axis=1), 6, SIZE)
        for k in DET:
            assert same_entry(two[k][64:70], alone[k]), k
        assert two["detections"][64:].max() > 0
    finally:
        m.set_streams(0)
        net.close()
        bh.close()
    m18, neck18 = nets("resnet18")
    net18, bh18 = model_rpn("resnet18", post=20), model_head("resnet18", D_=4)
    try:
        m18.set_input_size(32, 32)
        cap = m18.max_sub_batch()
        x = W.generate_input(cap + 1, seed=43, hw=(32, 32))
        whole = m18.forward_fpn(x, neck18, levels=(), rpn=net18, pooler=pooler, box_head=bh18)
        for k in DET:
            V.check_written(np.ascontiguousarray(whole[k]).view(np.uint8), whole[k].dtype.itemsize, k)
        pick = [0, 1, cap - 1, cap]
        few = m18.forward_fpn(x[pick], neck18, levels=(), rpn=net18, pooler=pooler, box_head=bh18)
        for k in DET:
            assert same_entry(whole[k][pick], few[k]), k
        assert few["detections"].max() > 0
        m18.set_profiling(True)
        m18.forward_fpn(x[:2], neck18, levels=("0",), rpn=net18, pooler=pooler, box_head=bh18)
        recs = [(r["layer"], r["op"]) for r in m18.profile() if r["layer"] in ("fpn", "rpn", "roi_heads")]
        assert recs.count(("roi_heads", "box_stage")) == 1 and recs[-1] == ("roi_heads", "box_stage") and recs[-2][1] == "roi_align"
    finally:
        m18.set_profiling(False)
        m18.set_input_size(*SIZE)
        net18.close()
        bh18.close()


def test_model_draw_with_no_detection_beside_full_images(nets):
    """Two images of zeros among 126 others, one in each part of a two-stream forward, under a head whose fc biases are
    zero and whose background bias is 4: the head is positively homogeneous, a zero image's pooled features are the
    smallest, and its every foreground probability stays under half the score threshold (largest: 0.025 of 0.05), while
    every other image has ten rows above 0.09.  So count is 0 for the two and D for all the others inside one call: each
    part writes its own padding rows beside a neighbour's full rows."""
    m, neck = nets()
    x = W.generate_input(128, seed=300 + SIZE[0] + SIZE[1], hw=SIZE)
    x[3] = 0
    x[70] = 0
    st = D.generate_box_head_state(WIDTH["resnet50"] * 4, MREP, MC, seed=6)
    st["box_head.fc6.bias"][:] = 0
    st["box_head.fc7.bias"][:] = 0
    st["box_predictor.cls_score.bias"][:] = [4, 0, 0, 0, 0]
    net, pooler = model_rpn("resnet50"), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2)
    bh = R.BoxHead(WIDTH["resnet50"], 2, MREP, MC, st, detections_per_img=4)
    bh.poison = True
    try:
        m.set_streams(2)
        assert m.parts(128) == 2
        got = m.forward_fpn(x, neck, levels=(), rpn=net, pooler=pooler, box_head=bh, detect_intermediates=True)
        m.set_streams(0)
        zero = np.zeros(128, bool)
        zero[[3, 70]] = True
        p = np.where(got["rois"].reshape(128, 60, 5)[:, :, :1] >= 0, got["probs"].reshape(128, 60, MC)[:, :, 1:], 0).reshape(128, -1)
        assert p[zero].max() < 0.03 and np.sort(p[~zero], axis=1)[:, -10].min() > 0.08, "the condition on the inputs"
        assert got["proposal_count"][zero].min() > 0, "the zero images do have proposals: the head turns them down"
        assert (got["detections"][zero] == 0).all() and (got["detections"][~zero] == 4).all(), got["detections"].tolist()
        check_detections(got, bh, 128, 60)
        for b in (3, 70):
            assert (got["labels"][b] == -1).all() and (got["detection_rois"][b] == -1).all()
            assert not got["boxes"][b].any() and not got["scores"][b].any() and not got["valid"][60 * b:60 * b + 60].any()
        assert (got["labels"][~zero] >= 1).all() and (got["scores"][~zero] > 0.05).all()
        one = m.forward_fpn(x, neck, levels=(), rpn=net, pooler=pooler, box_head=bh, detect_intermediates=True)
        for k in DET + MIDS:
            assert same_entry(one[k], got[k]), k
    finally:
        m.set_streams(0)
        net.close()
        bh.close()


def test_model_route_refusals(nets):
    m, neck = nets("resnet18")
    x = np.array(images())
    net, bh, pooler = model_rpn("resnet18"), model_head("resnet18"), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2)
    wrong = RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 3, 2)     # 64 * 9 values per RoI: not the head's in_features
    bad = model_head("resnet18", D_=2000)
    try:
        n0 = launches()
        with pytest.raises(L.RnError, match="in_features"):
            m.forward_fpn(x, neck, rpn=net, pooler=wrong, box_head=bh)
        with pytest.raises(ValueError):
            m.forward_fpn(x, neck, rpn=net, box_head=bh)
        with pytest.raises(ValueError):
            m.forward_fpn(x, neck, rpn=net, pooler=pooler, rois=np.zeros((4, 5), F), box_head=bh)
        with pytest.raises(L.RnError, match="detections_per_img"):
            m.forward_fpn(x, neck, rpn=net, pooler=pooler, box_head=bad)
        assert launches() == n0, "a refusal launches nothing"
    finally:
        net.close()
        bh.close()
        bad.close()
