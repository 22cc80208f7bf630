"""RPN proposals behind the head on the GPU: each launch alone on views between guard bands -- outputs pre-filled with
0xA5 and checked written everywhere -- against the numpy statement of the contract (resnet_c_amd/rpn.py).  Everything
behind the one operation that is not bit-defined (the decode's expf) is compared bit for bit on the boxes the device
itself returned; the boxes against the float64 decode within test_rpn_host.decode_bound."""
import ctypes

import numpy as np
import pytest

import views as V
from resnet_c_amd import _lib as L
from resnet_c_amd import ops, rpn
from test_dilation_gpu import bits
from test_fpn_gpu import launches
from test_rpn_host import KNOWN, chain_cases, clustered_boxes, decode_bound, random_heads

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(13, 17), (2, 3), (1, 1)]
IMAGE = (104, 136)          # strides 8 x 8, 52 x 45, 104 x 136
AG = rpn.AnchorGenerator(((32,), (64,), (128,)), (0.5, 1.0, 2.0))
CAND = (("index", np.int32, 1), ("logit", np.float32, 1), ("box", np.float32, 4), ("valid", np.uint8, 1))
PROP = (("boxes", np.float32, 4), ("logits", np.float32, 1), ("levels", np.int32, 1))


def record(line):
    """print a measured error beside its bound and, where RN_RPN_ERRORS_FILE names a file, append it there: that is how
    profiles/rpn/errors_and_bounds.txt is written"""
    import os
    print(line)
    path = os.environ.get("RN_RPN_ERRORS_FILE")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def u64s(v):
    return (ctypes.c_uint64 * len(v))(*[int(x) for x in v])


def select_decode(heads, base, image, pre, min_size=1e-3, logit_thresh=-np.inf, want=None, offs=None):
    """ONE rn_rpn_select_decode_forward on views: input guards intact, every requested output written everywhere"""
    offs = offs or {}
    n_levels, A = base.shape[:2]
    B = heads[0].shape[0]
    vh = [V.place(hd) for hd in heads]
    rows = B * n_levels * pre
    vo = {k: V.place_out(rows * c * np.dtype(t).itemsize, offs.get(k, 0)) for k, t, c in CAND if want is None or k in want}
    if want is None or "count" in want:
        vo["count"] = V.place_out(B * n_levels * 4, offs.get("count", 0))
    cand = L.RpnCandidates(*[vo[k].ptr if k in vo else None for k in ("index", "logit", "box", "valid", "count")])
    n0 = launches()
    V.must("rn_rpn_select_decode_forward", n_levels, (ctypes.c_void_p * n_levels)(*[v.ptr for v in vh]), B,
           u64s([hd.shape[1] for hd in heads]), u64s([hd.shape[2] for hd in heads]), A,
           np.ascontiguousarray(base, F).ctypes.data_as(ctypes.POINTER(ctypes.c_float)), image[0], image[1], pre,
           float(min_size), float(logit_thresh), ctypes.byref(cand))
    assert launches() - n0 == 1
    V.check_guards("select + decode inputs", *vh)
    out = {}
    for k, t, c in CAND + (("count", np.int32, 0),):
        if k in vo:
            shape = (B, n_levels) if k == "count" else (B, n_levels, pre) + ((4,) if c == 4 else ())
            out[k] = V.fetch(vo[k], t, f"cand.{k}", written=True).reshape(shape)
    return out


def check_candidates(got, heads, base, image, pre, min_size, logit_thresh):
    """index, logit, count, valid bit for bit; box within the bound of decode_f64; returns max error / bound"""
    want = rpn.select_decode_ref(heads, base, image, pre, min_size, logit_thresh, boxes=got["box"])
    assert np.array_equal(got["count"], want["count"])
    assert np.array_equal(got["index"], want["index"])
    assert np.array_equal(bits(got["logit"]), bits(want["logit"]))
    assert np.array_equal(got["valid"], want["valid"])
    A = base.shape[1]
    anchors = rpn.grid_anchors(base, [hd.shape[1:3] for hd in heads], image)
    worst_err, worst_ratio = 0.0, 0.0
    for l, hd in enumerate(heads):
        _, deltas = rpn.unpack_head(hd, A)
        for b in range(hd.shape[0]):
            k = int(got["count"][b, l])
            idx = got["index"][b, l, :k]
            ref = rpn.decode_f64(anchors[l][idx], deltas[b][idx], image_size=image)
            bound = decode_bound(anchors[l][idx], deltas[b][idx])
            dev = got["box"][b, l, :k].astype(np.float64)
            assert np.array_equal(np.isnan(dev), np.isnan(ref))
            fin = ~np.isnan(ref)               # a NaN delta gives a NaN box on both sides and has no bound
            err, bound = np.abs(dev - ref)[fin], bound[fin]
            assert (err <= bound).all(), f"level {l} image {b}: box error {(err / bound).max():.3f} of the bound"
            assert not got["box"][b, l, k:].any()
            if err.size:
                worst_err, worst_ratio = max(worst_err, float(err.max())), max(worst_ratio, float((err / bound).max()))
    return worst_err, worst_ratio


@pytest.mark.parametrize("kind", ["random", "quantised", "special"])
def test_select_decode_bit_for_bit_and_boxes_within_the_bound(kind):
    g = np.random.default_rng({"random": 1, "quantised": 2, "special": 3}[kind])
    base = AG.base_anchors()
    heads = random_heads(g, 2, SIZES, 3, kind)
    heads[0][0, 2, 3, 3 + 4 * 1 + 2] = 7.0       # a dw above the clip
    heads[0][1, 5, 5, 3 + 4 * 2 + 0] = np.nan    # a NaN delta: the candidate is invalid
    worst = (0.0, 0.0)
    for pre in (1, 2, 64, 65, 100, 1000):        # 1000 is above every segment's 663 anchors
        got = select_decode(heads, base, IMAGE, pre, min_size=12.0, logit_thresh=-0.25)
        worst = max(worst, check_candidates(got, heads, base, IMAGE, pre, 12.0, -0.25), key=lambda t: t[1])
        if pre >= 100:
            assert got["valid"].any() and not got["valid"][got["index"] >= 0].all(), "both outcomes of the validity rule"
    record(f"select + decode ({kind}): max |box - decode_f64| = {worst[0]:.3e}, {worst[1]:.3f} of the bound")


def test_select_decode_segment_above_4096_anchors_and_partial_outputs():
    g = np.random.default_rng(4)
    base = AG.base_anchors()[:2]
    heads = random_heads(g, 2, [(40, 40), (3, 2)], 3, "quantised")   # 4800 anchors: the k-th key sits inside a mass tie
    for pre in (100, 4096):
        got = select_decode(heads, base, (160, 160), pre)
        err, ratio = check_candidates(got, heads, base, (160, 160), pre, 1e-3, -np.inf)
        record(f"select + decode (4800 anchors, k = {pre}): max |box - decode_f64| = {err:.3e}, {ratio:.3f} of the bound")
    full = select_decode(heads, base, (160, 160), 100)
    part = select_decode(heads, base, (160, 160), 100, want=("index", "count"), offs={"index": 4})
    assert np.array_equal(part["index"], full["index"]) and np.array_equal(part["count"], full["count"])


def nms_call(boxes, thr, valid=None, offs=None):
    """ONE rn_nms_forward (two launches) on views"""
    offs = offs or {}
    S, n = boxes.shape[:2]
    vb = V.place(boxes, offs.get("boxes", 0))
    vv = V.place(np.ascontiguousarray(valid, np.uint8), offs.get("valid", 0)) if valid is not None else None
    vk, vc = V.place_out(S * n, offs.get("keep", 0)), V.place_out(S * 4)
    n0 = launches()
    V.must("rn_nms_forward", vb.ptr, vv.ptr if vv else None, S, n, float(thr), vk.ptr, vc.ptr)
    assert launches() - n0 == 2
    V.check_guards("rn_nms_forward inputs", vb, vv)
    keep = V.fetch(vk, np.uint8, "keep", written=True).reshape(S, n)
    count = V.fetch(vc, np.int32, "keep_count", written=True)
    assert np.array_equal(count, keep.sum(axis=1)) and set(np.unique(keep)) <= {0, 1}
    return keep.astype(bool)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 300, 1000])
def test_nms_bit_for_bit_on_clustered_boxes(n):
    boxes = np.stack([clustered_boxes(n), clustered_boxes(n, seed=n + 7919)])
    chains = []
    for thr in (0.3, 0.5, 0.7):
        want = ops.nms_segments_ref(boxes, thr)
        if n >= 63:   # the cases bite, on the reference
            for s in range(2):
                assert 0.05 * n <= want[s].sum() <= 0.60 * n, (n, thr, s, int(want[s].sum()))
            chains.append(chain_cases(boxes[0], want[0], thr))
        got = nms_call(boxes, thr, offs={"boxes": 4, "keep": 1} if thr == 0.5 else None)
        assert np.array_equal(got, want), f"n {n} threshold {thr}: {np.flatnonzero(got != want)[:8]}"
    assert n < 63 or max(chains) >= 1, chains
    # a mask that removes the first box of a segment, one that removes all of them
    valid = np.ones((2, n), np.uint8)
    valid[0, 0] = 0
    valid[1, :] = 0
    got = nms_call(boxes, 0.5, valid)
    assert np.array_equal(got, ops.nms_segments_ref(boxes, 0.5, valid)) and not got[0, 0] and not got[1].any()


def test_nms_known_answers_and_the_python_op():
    two = np.stack([KNOWN, np.zeros((4, 4), F)])
    assert nms_call(two, 0.5).tolist() == [[True, True, True, False], [True] * 4]
    assert nms_call(two, np.nextafter(F(0.5), F(0))).tolist() == [[True, False, False, False], [True] * 4]
    g = np.random.default_rng(11)
    boxes, scores = clustered_boxes(200), np.round(g.standard_normal(200) * 4).astype(F)   # tied scores
    order = rpn.select_ref(scores, 200)
    want = order[rpn.nms_ref(boxes[order], 0.5)]
    assert np.array_equal(ops.nms(boxes, scores, 0.5), want)
    assert ops.nms(np.zeros((0, 4), F), np.zeros(0, F), 0.5).size == 0


def test_box_decode_with_the_box_heads_weights():
    g = np.random.default_rng(12)
    a = rpn.grid_anchors(AG.base_anchors(), SIZES, IMAGE)[0]
    d = (g.standard_normal(a.shape) * 2).astype(F)
    d[::13, 3] = 30.0
    for wgt, image in (((10.0, 10.0, 5.0, 5.0), IMAGE), ((1.0, 1.0, 1.0, 1.0), (np.inf, np.inf))):
        va, vd, vo = V.place(a, 4), V.place(d), V.place_out(a.size * 4, 8)
        n0 = launches()
        V.must("rn_box_decode_forward", va.ptr, vd.ptr, a.shape[0], *wgt, float(image[0]), float(image[1]), vo.ptr)
        assert launches() - n0 == 1
        V.check_guards("rn_box_decode_forward inputs", va, vd)
        got = V.fetch(vo, np.float32, "boxes", written=True).reshape(-1, 4)
        err = np.abs(got.astype(np.float64) - rpn.decode_f64(a, d, wgt, image))
        bound = decode_bound(a, d, wgt)
        assert (err <= bound).all(), (err / bound).max()
        record(f"box decode weights {wgt}: max error {err.max():.3e}, {(err / bound).max():.3f} of the bound")
        assert np.array_equal(bits(ops.box_decode(a, d, wgt, image)), bits(got))


def merge_call(cand, post, thr, want=None, offs=None):
    """ONE rn_rpn_nms_merge_forward (two launches) on views, candidates given"""
    offs = offs or {}
    B, n_levels, pre = cand["logit"].shape
    vi = {k: V.place(np.ascontiguousarray(cand[k], t)) for k, t in (("logit", F), ("box", F), ("valid", np.uint8), ("count", np.int32))}
    vo = {k: V.place_out(B * post * c * 4, offs.get(k, 0)) for k, _, c in PROP if want is None or k in want}
    if want is None or "count" in want:
        vo["count"] = V.place_out(B * 4)
    if want is None or "rois" in want:
        vo["rois"] = V.place_out(B * post * 20, offs.get("rois", 0))
    if want is None or "cand_keep" in want:
        vo["cand_keep"] = V.place_out(B * n_levels * pre, offs.get("cand_keep", 0))
    ci = L.RpnCandidates(None, vi["logit"].ptr, vi["box"].ptr, vi["valid"].ptr, vi["count"].ptr)
    co = L.RpnProposals(*[vo[k].ptr if k in vo else None for k in ("boxes", "logits", "levels", "count", "rois", "cand_keep")])
    n0 = launches()
    V.must("rn_rpn_nms_merge_forward", ctypes.byref(ci), B, n_levels, pre, post, float(thr), ctypes.byref(co))
    assert launches() - n0 == 2
    V.check_guards("rn_rpn_nms_merge_forward inputs", *vi.values())
    shapes = {"boxes": (B, post, 4), "logits": (B, post), "levels": (B, post), "count": (B,), "rois": (B * post, 5),
              "cand_keep": (B, n_levels, pre)}
    types = {"levels": np.int32, "count": np.int32, "cand_keep": np.uint8}
    return {k: V.fetch(v, types.get(k, np.float32), f"out.{k}", written=True).reshape(shapes[k]) for k, v in vo.items()}


def assert_proposals(got, want):
    for k, v in got.items():
        w = want[k]
        assert np.array_equal(bits(v) if v.dtype == np.float32 else v, bits(w) if v.dtype == np.float32 else w), k


def test_merge_ties_across_levels_padding_and_count():
    # disjoint unit boxes: nothing is suppressed; logits tie inside and across the levels
    B, n_levels, pre = 2, 3, 5
    g = np.random.default_rng(13)
    corner = np.arange(B * n_levels * pre, dtype=F).reshape(B, n_levels, pre) * 2
    cand = {"box": np.stack([corner, corner, corner + 1, corner + 1], axis=-1),
            "logit": np.sort(np.round(g.standard_normal((B, n_levels, pre))).astype(F), axis=2)[..., ::-1].copy(),
            "valid": np.ones((B, n_levels, pre), np.uint8), "count": np.full((B, n_levels), pre, np.int32)}
    cand["count"][1, 2] = 3                       # a short segment: its ranks 3, 4 are padding
    cand["valid"][1, 2, 3:] = 0
    cand["valid"][0, 1, 0] = 0                    # an invalid candidate
    for post in (4, 14, 15, 20):                  # below, at and above the survivor counts (14 and 13)
        want = rpn.nms_merge_ref(cand, post, 0.7)
        got = merge_call(cand, post, 0.7)
        assert_proposals(got, want)
        assert got["count"].tolist() == [min(post, 14), min(post, 13)]
        for b in range(B):
            c = got["count"][b]
            lv, lg = got["levels"][b, :c], got["logits"][b, :c]
            assert (np.diff(lg) <= 0).all()
            tie = np.flatnonzero(np.diff(lg) == 0)
            assert (lv[tie] <= lv[tie + 1]).all(), "a tie resolves by position: the lower level first"
            assert (got["levels"][b, c:] == -1).all() and np.isneginf(got["logits"][b, c:]).all()
            assert not got["boxes"][b, c:].any() and (got["rois"].reshape(B, post, 5)[b, c:, 0] == -1).all()
            assert (got["rois"].reshape(B, post, 5)[b, :c, 0] == b).all()
    part = merge_call(cand, 14, 0.7, want=("rois",), offs={"rois": 4})
    assert np.array_equal(bits(part["rois"]), bits(rpn.nms_merge_ref(cand, 14, 0.7)["rois"]))


@pytest.mark.parametrize("pre,post", [(100, 60), (1000, 1000), (300, 4096)])
def test_the_three_launches_against_the_contract(pre, post):
    """select + decode, mask, scan + merge on random heads; the proposals bit for bit nms_ref + merge_ref of the
    candidates the same run returned"""
    g = np.random.default_rng(pre)
    base = AG.base_anchors()
    heads = random_heads(g, 2, SIZES, 3, "random", delta_std=0.2)
    heads[0][..., :3] += 1.0                       # the fine level wins most of the merge, not all of it
    cand = select_decode(heads, base, IMAGE, pre, min_size=12.0)
    check_candidates(cand, heads, base, IMAGE, pre, 12.0, -np.inf)
    want = rpn.nms_merge_ref(cand, post, 0.5)
    got = merge_call(cand, post, 0.5)
    assert_proposals(got, want)
    # (0.5: neighbouring anchors of the 8-pixel grid overlap by 0.6, so the suppression bites)
    valid, kept = cand["valid"].sum(), got["cand_keep"].sum()
    assert 0.1 * valid <= kept <= 0.9 * valid, (int(valid), int(kept))
    if (pre, post) == (100, 60):
        assert (got["count"] == 60).all() and (cand["count"][:, 0] == 100).all() and (cand["count"][:, 1:] < 100).all()
    # the Python route: the same three launches, nothing leaving the device in between
    res = rpn.filter_proposals(heads, AG, IMAGE, pre, post, 0.5, 0.0, 12.0, return_candidates=True)
    assert np.array_equal(bits(res["rois"]), bits(got["rois"])) and np.array_equal(res["cand"]["keep"], got["cand_keep"])
    for b in range(2):
        c = got["count"][b]
        assert np.array_equal(bits(res["boxes"][b]), bits(got["boxes"][b, :c])) and res["levels"][b].tolist() == got["levels"][b, :c].tolist()
        assert np.allclose(res["scores"][b], 1 / (1 + np.exp(-got["logits"][b, :c].astype(np.float64))), rtol=1e-6)


def test_refusals_launch_nothing():
    base = np.ascontiguousarray(AG.base_anchors(), F)
    heads = random_heads(np.random.default_rng(0), 2, SIZES, 3)
    vh = [V.place(hd) for hd in heads]
    B, nl, pre, post = 2, 3, 64, 32
    rows = B * nl * pre
    vc = {"index": V.place_out(rows * 4), "logit": V.place_out(rows * 4), "box": V.place_out(rows * 16),
          "valid": V.place_out(rows), "count": V.place_out(B * nl * 4)}
    vp = {"boxes": V.place_out(B * post * 16), "logits": V.place_out(B * post * 4), "levels": V.place_out(B * post * 4),
          "count": V.place_out(B * 4), "rois": V.place_out(B * post * 20), "cand_keep": V.place_out(rows)}

    def cand(**kw):
        p = {k: v.ptr for k, v in vc.items()}
        p.update(kw)
        return L.RpnCandidates(p["index"], p["logit"], p["box"], p["valid"], p["count"])

    def prop(**kw):
        p = {k: v.ptr for k, v in vp.items()}
        p.update(kw)
        return L.RpnProposals(p["boxes"], p["logits"], p["levels"], p["count"], p["rois"], p["cand_keep"])

    def select(c=None, **kw):
        a = dict(L=nl, heads=[v.ptr for v in vh], B=B, h=[s[0] for s in SIZES], w=[s[1] for s in SIZES], A=3, image=IMAGE,
                 pre=pre, min_size=1e-3, thresh=-np.inf)
        a.update(kw)
        c = c or cand()
        return V.call("rn_rpn_select_decode_forward", a["L"], (ctypes.c_void_p * 5)(*(a["heads"] + [None] * 5)[:5]), a["B"],
                      u64s((a["h"] + [1] * 5)[:5]), u64s((a["w"] + [1] * 5)[:5]), a["A"],
                      base.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a["image"][0], a["image"][1], a["pre"],
                      float(a["min_size"]), float(a["thresh"]), ctypes.byref(c))

    def merge(c=None, o=None, **kw):
        a = dict(B=B, L=nl, pre=pre, post=post, thr=0.7)
        a.update(kw)
        c, o = c or cand(), o or prop()
        return V.call("rn_rpn_nms_merge_forward", ctypes.byref(c), a["B"], a["L"], a["pre"], a["post"], float(a["thr"]),
                      ctypes.byref(o))

    boxes, keep = V.place(np.zeros((2, 8, 4), F)), V.place_out(16)
    n0 = launches()
    refused = [
        (select(L=0), "L must be"), (select(L=6), "L must be"), (select(A=13), "A must be"), (select(pre=0), "pre_nms_top_n"),
        (select(pre=4097), "pre_nms_top_n"), (select(heads=[vh[0].ptr, None, vh[2].ptr]), "head output is NULL"),
        (select(c=L.RpnCandidates()), "every output"), (select(c=cand(logit=vc["logit"].ptr + 2)), "cand.logit is off"),
        (select(c=cand(box=vc["logit"].ptr + 16)), "overlaps"), (select(c=cand(index=vh[0].ptr)), "overlaps"),
        (select(thresh=np.nan), "NaN"), (select(h=[200, 2, 1]), "h and w"), (select(image=(0, 136)), "image_h"),
        (merge(L=0), "L must be"), (merge(pre=5000), "pre_nms_top_n"), (merge(post=0), "post_nms_top_n"),
        (merge(post=4097), "post_nms_top_n"), (merge(thr=np.nan), "NaN"), (merge(c=cand(valid=None)), "is NULL"),
        (merge(o=L.RpnProposals()), "every output"), (merge(o=prop(rois=vp["rois"].ptr + 1)), "out.rois is off"),
        (merge(o=prop(boxes=vc["box"].ptr)), "overlaps"), (merge(o=prop(levels=vp["logits"].ptr)), "overlaps"),
        (V.call("rn_nms_forward", boxes.ptr, None, 2, 4097, 0.5, keep.ptr, None), "n must be"),
        (V.call("rn_nms_forward", None, None, 2, 8, 0.5, keep.ptr, None), "boxes is NULL"),
        (V.call("rn_nms_forward", boxes.ptr, None, 2, 8, 0.5, None, None), "keep is NULL"),
        (V.call("rn_nms_forward", boxes.ptr + 2, None, 2, 4, 0.5, keep.ptr, None), "boxes is off"),
        (V.call("rn_nms_forward", boxes.ptr, None, 2, 8, 0.5, boxes.ptr + 32, None), "overlaps"),
        (V.call("rn_nms_forward", boxes.ptr, None, 2, 8, float("nan"), keep.ptr, None), "NaN"),
        (V.call("rn_box_decode_forward", boxes.ptr, boxes.ptr, 16, 1.0, 1.0, 0.0, 1.0, 10.0, 10.0, vp["boxes"].ptr), "weights"),
        (V.call("rn_box_decode_forward", boxes.ptr, boxes.ptr, 16, 1.0, 1.0, 1.0, 1.0, 0.0, 10.0, vp["boxes"].ptr), "image_h"),
        (V.call("rn_box_decode_forward", boxes.ptr, None, 16, 1.0, 1.0, 1.0, 1.0, 10.0, 10.0, vp["boxes"].ptr), "deltas is NULL"),
        (V.call("rn_box_decode_forward", boxes.ptr, boxes.ptr, 16, 1.0, 1.0, 1.0, 1.0, 10.0, 10.0, boxes.ptr + 64), "overlaps"),
    ]
    for i, ((st, msg), text) in enumerate(refused):
        assert st == L.RN_ERR_INVALID and text in msg, (i, st, msg, text)
    # nothing to do is no refusal, and launches nothing either
    assert select(B=0)[0] == L.RN_OK and merge(B=0)[0] == L.RN_OK
    assert V.call("rn_nms_forward", boxes.ptr, None, 0, 8, 0.5, keep.ptr, None)[0] == L.RN_OK
    assert V.call("rn_box_decode_forward", boxes.ptr, boxes.ptr, 0, 1.0, 1.0, 1.0, 1.0, 10.0, 10.0, vp["boxes"].ptr)[0] == L.RN_OK
    assert launches() == n0
    for v in list(vc.values()) + list(vp.values()) + [keep]:
        V.assert_untouched(v, "refused calls")
    # and the calls they all almost were: the stage behind the head is three launches, whatever B
    assert select()[0] == L.RN_OK and merge()[0] == L.RN_OK
    assert launches() - n0 == 3
    for k, v in list(vc.items()) + list(vp.items()):
        V.fetch(v, np.uint8 if k in ("valid", "cand_keep") else np.float32, k, written=True)


# =====================================================================================================================
# the object and the neck route
# =====================================================================================================================
# The FPN tests' geometry: a 72 x 40 image, levels 18x10, 9x5, 5x3, 3x2 and the pooled 2x1, on a neck of its own
# (random stage maps; the model route is not carried).  HEAD_STD = 0.03: on this pyramid the seeded head's deltas have a
# standard deviation of 0.42 and its logits one of 0.38 (chosen on the float64 reference, asserted below).
import resnet_c_amd as R  # noqa: E402
from resnet_c_amd import fpn as P  # noqa: E402
from resnet_c_amd import roi as RO  # noqa: E402
from test_dilation_gpu import tol_f32  # noqa: E402
from test_fpn_host import products  # noqa: E402

OSIZE, OCIN, OA, OSIZES = (72, 40), (64, 64, 128, 128), 64, [(18, 10), (9, 5), (5, 3), (3, 2)]
OAG = rpn.AnchorGenerator(((16,), (32,), (64,), (128,), (256,)), (0.5, 1.0, 2.0))
HEAD_STD, PRE, THR = 0.03, 100, 0.7
NAMES5 = ("0", "1", "2", "3", "pool")


@pytest.fixture(scope="module")
def stage():
    g = np.random.default_rng(77)
    maps = [g.standard_normal((2, c, h, w)).astype(F) for c, (h, w) in zip(OCIN, OSIZES)]
    fstate, hstate = P.generate_fpn_state(OCIN, OA, seed=5), rpn.generate_rpn_state(OA, 3, seed=1, std=HEAD_STD)
    neck = P.FeaturePyramidNetwork(OCIN, OA, fstate, extra="pool")
    nets = {post: R.RegionProposalNetwork(OA, OAG, {"rpn." + k: v for k, v in hstate.items()}, PRE, post, THR) for post in (1000, 60)}
    ref = P.fpn_ref([m.astype(np.float64) for m in maps], fstate, "pool")
    yield dict(maps=maps, nhwc=[np.ascontiguousarray(m.transpose(0, 2, 3, 1)) for m in maps], fstate=fstate, hstate=hstate,
               neck=neck, nets=nets, ref=ref, head64=rpn.rpn_head_ref([ref[k] for k in NAMES5], hstate, 3))
    neck.close()
    for n in nets.values():
        n.close()


def assert_contract(out, post):
    """the final outputs are nms_ref + merge_ref of the candidates the same call returned, bit for bit"""
    cand = dict(out["cand"])
    want = rpn.nms_merge_ref(cand, post, THR)
    assert np.array_equal(cand["keep"], want["cand_keep"])
    assert np.array_equal(out["proposal_count"], want["count"])
    assert np.array_equal(bits(out["proposal_logits"]), bits(want["logits"])) and np.array_equal(bits(out["rois"]), bits(want["rois"]))
    for b, c in enumerate(want["count"]):
        assert np.array_equal(bits(out["proposals"][b]), bits(want["boxes"][b, :c]))
        assert out["proposal_levels"][b].tolist() == want["levels"][b, :c].tolist()
        assert np.array_equal(bits(out["scores"][b]), bits(rpn.sigmoid(want["logits"][b, :c])))
    return cand, want


def flat(out):
    r = {"proposal_logits": out["proposal_logits"], "proposal_count": out["proposal_count"], "rois": out["rois"]}
    r.update({"cand_" + k: v for k, v in out["cand"].items()})
    return r


@pytest.mark.parametrize("post", [1000, 60])
def test_object_and_neck_route_bit_for_bit(stage, post):
    net, neck = stage["nets"][post], stage["neck"]
    n0 = launches()
    via_neck = neck.forward(stage["nhwc"], rpn=net, image_size=OSIZE, candidates=True)
    # the neck's 4 laterals, 3 top-down steps, 4 3x3s, the pool and 5 exports, then the stage: 2 L + 3
    assert launches() - n0 == 17 + 2 * 5 + 3
    feats = {k: via_neck[k] for k in NAMES5}
    n0 = launches()
    alone = net(feats, OSIZE, return_candidates=True)
    assert launches() - n0 == 2 * 5 + 3, "the stage is 2 L + 3 launches"
    alone.update(proposal_logits=alone["raw"]["logits"], proposal_count=alone["raw"]["count"], rois=alone["raw"]["rois"])
    cand, want = assert_contract(via_neck, post)
    assert_contract(alone, post)
    a, b = flat(via_neck), flat(alone)   # the exported levels are the bits the neck route read in place
    for k in a:
        assert np.array_equal(a[k].view(np.uint8) if a[k].dtype != np.uint8 else a[k], b[k].view(np.uint8) if b[k].dtype != np.uint8 else b[k]), k
    # an image alone: the same rows (B does not reach any bit)
    one = neck.forward([m[1:2] for m in stage["nhwc"]], levels=(), rpn=net, image_size=OSIZE)
    assert np.array_equal(bits(one["proposals"][0]), bits(via_neck["proposals"][1]))
    # the conditions, on the reference applied to the returned candidates
    cnt, valid, kept = cand["count"], cand["valid"].sum(), want["cand_keep"].sum()
    assert (cnt == PRE).any() and (cnt < PRE).any(), cnt.tolist()
    assert 0.1 * valid <= valid - kept and 0.1 * valid <= kept, (int(valid), int(kept))
    assert (cand["index"] >= 0).sum() > valid, "at least one candidate fails min_size"
    if post == 60:
        assert (want["count"] == 60).all() and kept > 120
    record(f"rpn on the pyramid (post {post}): {int(valid)} valid candidates, {int(kept)} survivors, counts {want['count'].tolist()}")


def test_object_against_float64(stage):
    """logits and boxes of the device's selected anchors against rpn_head_ref + decode_f64 on the neck's float64
    reference.  The bound: the FPN tests' level bound e_l = tol_f32(level, products), carried through the head --
    the 3x3 amplifies an input error by at most the largest L1 norm of a filter and adds its own tol_f32(t, 9 C); the
    1x1 panel likewise with tol_f32(head, C) -- and, for a box, through the decode to first order (dx moves x by wa,
    dw by pw / 2, the exponential's excess exp(e) - 1 - e included) plus the decode bound."""
    out = stage["nets"][1000](dict(zip(NAMES5, stage["neck"].forward(stage["nhwc"]).values())), OSIZE, return_candidates=True)
    st, cand = stage["hstate"], out["cand"]
    w3 = np.abs(st["head.conv.0.0.weight"].astype(np.float64)).reshape(OA, -1).sum(axis=1).max()
    wp = np.abs(np.concatenate([st["head.cls_logits.weight"].reshape(3, -1), st["head.bbox_pred.weight"].reshape(12, -1)])
                .astype(np.float64)).sum(axis=1).max()
    anchors = rpn.grid_anchors(OAG.base_anchors(), OSIZES + [(2, 1)], OSIZE)
    for l, name in enumerate(NAMES5):
        lev = stage["ref"][name]
        e_l = tol_f32(lev, products(OCIN, OA, min(l, 3)))
        t_max = float(np.abs(lev).max()) * w3 + 1.0                 # |t| <= |x| L1(w3) + |b|
        e_t = e_l * w3 + tol_f32(np.array([t_max]), 9 * OA)
        head = stage["head64"][l]
        e_h = e_t * wp + tol_f32(head, OA)
        lg64, d64 = rpn.unpack_head(head, 3)
        for b in range(2):
            k = int(cand["count"][b, l])
            idx = cand["index"][b, l, :k]
            err = np.abs(cand["logit"][b, l, :k] - lg64[b][idx]).max()
            assert err <= e_h, (name, b, err, e_h)
            rest = np.delete(lg64[b], idx)
            assert rest.size == 0 or rest.max() <= lg64[b][idx].min() + 2 * e_h, "an unselected anchor ranks above a selected one"
            a, d = anchors[l][idx].astype(np.float64), d64[b][idx]
            ref = rpn.decode_f64(a, d, image_size=OSIZE)
            wa, ha = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
            pw, ph = np.exp(np.minimum(d[:, 2], float(rpn.BBOX_XFORM_CLIP))) * wa, np.exp(np.minimum(d[:, 3], float(rpn.BBOX_XFORM_CLIP))) * ha
            grow = np.expm1(e_h)
            bx, by = e_h * wa + 0.5 * pw * grow, e_h * ha + 0.5 * ph * grow
            bound = decode_bound(a, d) * (1 + grow) + np.stack([bx, by, bx, by], axis=1)
            berr = np.abs(cand["box"][b, l, :k].astype(np.float64) - ref)
            assert (berr <= bound).all(), (name, b, float((berr / bound).max()))
            record(f"rpn level {name} image {b}: logit error {err:.3e} of bound {e_h:.3e}; box error {(berr / bound).max():.2e} of its bound")
    d = np.concatenate([h[..., 3:15].reshape(-1) for h in stage["head64"]])
    lg = np.concatenate([h[..., :3].reshape(-1) for h in stage["head64"]])
    assert 0.1 <= d.std() <= 0.5 and np.unique(lg.astype(F)).size > lg.size // 2, (d.std(), lg.std())


def test_neck_route_chains_into_the_pooler(stage):
    """with a pooler and no rois the pooler pools the proposals of the same call: the same bits as pooling the
    returned RoIs in a second call; the padding rows come back as zeros"""
    net, neck = stage["nets"][60], stage["neck"]
    pooler = RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 3, 2)
    got = neck.forward(stage["nhwc"], levels=("0",), rpn=net, image_size=OSIZE, pooler=pooler, roi_levels=True)
    assert got["pooled"].shape == (2 * 60, OA, 3, 3) and got["rois"].shape == (120, 5)
    again = neck.forward(stage["nhwc"], levels=(), rois=got["rois"], pooler=pooler, image_size=OSIZE, roi_levels=True, validate=False)
    assert np.array_equal(bits(got["pooled"]), bits(again["pooled"])) and np.array_equal(got["roi_levels"], again["roi_levels"])
    assert got["pooled"].any()
    short = neck.forward(stage["nhwc"], levels=(), rpn=stage["nets"][1000], image_size=OSIZE, pooler=pooler, roi_levels=True)
    pad = short["rois"][:, 0] < 0
    assert pad.any() and not short["pooled"][pad].any() and (short["roi_levels"][pad] == -1).all() and short["pooled"][~pad].any()


def test_object_refusals(stage):
    net, neck = stage["nets"][60], stage["neck"]
    lib, ctx = L.lib(), R.get_ctx()
    spec, bufs = net.buffers(2, True)
    vx = [V.place(m) for m in stage["nhwc"]] + [V.place(np.zeros((2, 2, 1, OA), F))]
    hs, ws = u64s([18, 9, 5, 3, 2]), u64s([10, 5, 3, 2, 1])
    xp = (ctypes.c_void_p * 5)(*[v.ptr for v in vx])

    def fwd(req, image=OSIZE, x=xp):
        st = lib.rn_rpn_forward(net.handle, x, 2, hs, ws, image[0], image[1], ctypes.byref(req) if req is not None else None)
        return st, (lib.rn_last_error(ctx.handle) or b"").decode()

    def req(**kw):
        r = net.request(bufs)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    n0 = launches()
    bad_out, overl, onmap = req(), req(), req()
    bad_out.out = L.RpnProposals()
    overl.out.logits = bufs["boxes"].ptr
    onmap.out.rois = vx[0].ptr
    cases = [(fwd(None), "request is NULL"), (fwd(req(pre_nms_top_n=0)), "pre_nms_top_n"), (fwd(req(post_nms_top_n=4097)), "post_nms_top_n"),
             (fwd(req(nms_thresh=float("nan"))), "NaN"), (fwd(req(), image=(0, 40)), "image_h"), (fwd(bad_out), "every output"),
             (fwd(overl), "overlaps"), (fwd(onmap), "overlaps"), (fwd(req(), image=(10, 40)), "h and w"),
             (fwd(req(), x=(ctypes.c_void_p * 5)(vx[0].ptr, None, vx[2].ptr, vx[3].ptr, vx[4].ptr)), "map is NULL")]
    for i, ((st, msg), text) in enumerate(cases):
        assert st == L.RN_ERR_INVALID and text in msg, (i, st, msg, text)
    assert launches() == n0, "a refusal launches nothing"
    four = P.FeaturePyramidNetwork(OCIN, OA, stage["fstate"], extra=None)
    n0 = launches()
    with pytest.raises(L.RnError, match="level count"):      # an rpn of five levels behind a neck of four outputs
        four.forward(stage["nhwc"], rpn=net, image_size=OSIZE)
    assert launches() == n0
    four.close()
    h = ctypes.c_void_p()
    base = np.ascontiguousarray(OAG.base_anchors())
    fp = base.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.rn_rpn_create(ctx.handle, ctypes.byref(h), 100, 5, 3, fp) == L.RN_ERR_INVALID      # in_channels % 64
    assert lib.rn_rpn_create(ctx.handle, ctypes.byref(h), 64, 6, 3, fp) == L.RN_ERR_INVALID
    assert lib.rn_rpn_create(ctx.handle, ctypes.byref(h), 64, 5, 3, fp) == L.RN_OK
    w = np.zeros(64 * 64 * 9, F)
    assert lib.rn_rpn_set_tensor(h, b"head.conv.weight", w.ctypes.data, w.size) == L.RN_OK       # the older spelling
    assert lib.rn_rpn_set_tensor(h, b"head.conv.0.0.bias", w.ctypes.data, 63) == L.RN_ERR_INVALID
    assert lib.rn_rpn_set_tensor(h, b"head.nothing", w.ctypes.data, 64) == L.RN_ERR_INVALID
    assert lib.rn_rpn_finalize(h) == L.RN_ERR_INVALID and b"is not set" in lib.rn_last_error(ctx.handle)
    assert lib.rn_rpn_destroy(h) == L.RN_OK
    st, msg = fwd(req())
    assert st == L.RN_OK, msg
    ctx.sync()


# =====================================================================================================================
# the model route
# =====================================================================================================================
from resnet_c_amd import weights as W  # noqa: E402
from test_fpn_gpu import SIZE, WIDTH, images, nets  # noqa: E402,F401  (nets: a fixture)


def model_rpn(arch, post=60, std=0.01):
    net = R.RegionProposalNetwork(WIDTH[arch], OAG, rpn.generate_rpn_state(WIDTH[arch], 3, seed=3, std=std), PRE, post, THR)
    net.poison = True
    return net


def no_poison(out):
    for k, v in flat(out).items():
        V.check_written(np.ascontiguousarray(v).view(np.uint8), v.dtype.itemsize, k)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_model_route_bit_for_bit(nets, arch, dtype):
    m, neck = nets(arch, dtype)
    x = np.array(images())
    net = model_rpn(arch)
    try:
        got = m.forward_fpn(x, neck, rpn=net, candidates=True)
        no_poison(got)
        cand, want = assert_contract(got, 60)
        assert (cand["count"] == PRE).any() and (cand["count"] < PRE).any() and want["count"].max() > 0
        # the stage alone on the levels the same forward exported: the same bits (the head is fp32 on fp32 levels)
        alone = net({k: got[k] for k in NAMES5}, SIZE, return_candidates=True)
        alone.update(proposal_logits=alone["raw"]["logits"], proposal_count=alone["raw"]["count"], rois=alone["raw"]["rois"])
        a, b = flat(got), flat(alone)
        for k in a:
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k
        plain = m.forward_fpn(x, neck)       # and the pyramid keeps its bits
        assert all(np.array_equal(bits(plain[k]), bits(got[k])) for k in NAMES5)
        if dtype == "f32" and arch == "resnet18":
            px = np.random.default_rng(9).integers(0, 256, (2,) + SIZE + (3,), dtype=np.uint8)
            from resnet_c_amd import preprocess
            u8 = m.forward_fpn_u8(px, neck, levels=(), rpn=net)
            fl = m.forward_fpn(preprocess.normalize_u8(px), neck, levels=(), rpn=net)
            assert np.array_equal(bits(u8["rois"]), bits(fl["rois"]))
    finally:
        net.close()


def test_model_parts_sub_batches_and_the_chain(nets):
    """128 images as two parts on two streams, then one image more than a launch batch holds; the pooler takes the
    proposals of the same forward.  Outputs are filled with 0xA5 before every forward: every row is written, and the
    bits are those of one stream."""
    m, neck = nets()
    x = W.generate_input(128, seed=300 + SIZE[0] + SIZE[1], hw=SIZE)
    net, pooler = model_rpn("resnet50"), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 3, 2)
    try:
        m.set_streams(1)
        one = m.forward_fpn(x, neck, levels=(), rpn=net, pooler=pooler, roi_levels=True, candidates=True)
        m.set_streams(2)
        assert m.parts(128) == 2
        two = m.forward_fpn(x, neck, levels=("0",), rpn=net, pooler=pooler, roi_levels=True, candidates=True)
        m.set_streams(0)
        no_poison(two)
        assert_contract(two, 60)
        a, b = flat(one), flat(two)
        for k in a:
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k
        assert np.array_equal(bits(one["pooled"]), bits(two["pooled"])) and np.array_equal(one["roi_levels"], two["roi_levels"])
        assert (two["rois"].reshape(128, 60, 5)[64:, 0, 0] == np.arange(64, 128)).all(), "the second part's rows name its images"
        again = m.forward_fpn(x, neck, levels=(), rois=two["rois"], pooler=pooler, roi_levels=True, validate=False)
        assert np.array_equal(bits(again["pooled"]), bits(two["pooled"])) and np.array_equal(again["roi_levels"], two["roi_levels"])
        assert two["pooled"][60 * 64:].any()
    finally:
        m.set_streams(0)
        net.close()
    m18, neck18 = nets("resnet18")
    net18 = model_rpn("resnet18", post=20)
    try:
        m18.set_input_size(32, 32)
        cap = m18.max_sub_batch()
        x = W.generate_input(cap + 1, seed=43, hw=(32, 32))
        whole = m18.forward_fpn(x, neck18, levels=(), rpn=net18, pooler=pooler, roi_levels=True)
        V.check_written(whole["rois"].view(np.uint8), 4, "rois")
        pick = [0, 1, cap - 1, cap]
        few = m18.forward_fpn(x[pick], neck18, levels=(), rpn=net18, pooler=pooler, roi_levels=True)
        rw, rf = whole["rois"].reshape(cap + 1, 20, 5), few["rois"].reshape(4, 20, 5)
        pw, pf = whole["pooled"].reshape(cap + 1, 20, -1), few["pooled"].reshape(4, 20, -1)
        assert whole["proposal_count"].min() >= 0 and few["proposal_count"].max() > 0
        for i, b in enumerate(pick):
            c = few["proposal_count"][i]
            assert whole["proposal_count"][b] == c and np.array_equal(bits(rw[b, :, 1:]), bits(rf[i, :, 1:]))
            assert (rw[b, :c, 0] == b).all() and (rw[b, c:, 0] == -1).all()
            assert np.array_equal(bits(pw[b]), bits(pf[i]))
        m18.set_profiling(True)
        m18.forward_fpn(x[:2], neck18, levels=("0",), rpn=net18)
        names = [r["op"] for r in m18.profile() if r["layer"] in ("fpn", "rpn")]
        assert names.count("rpn_stage") == 1 and names[-1] == "rpn_stage" and names.count("fpn_layer3") == 1
    finally:
        m18.set_profiling(False)
        m18.set_input_size(*SIZE)
        net18.close()
