"""What the six objects behind the backbone share (csrc/rn_stage.hip), on every kind of object: the neck, the RPN, the
box head, the mask head, the keypoint head and the segmentation head (FCN and DeepLab).  A tensor set twice, scratch growth, the two
messages that name a key, and the growth guard while a captured graph lives.  Everything is compared bit for bit: an
object that went through the bookkeeping against a fresh one on the same input, every output between guard bands
(tests/views.py) taken as raw bytes.  Shapes are the smallest each object accepts.  Last, the two RoI heads in one call
with two different poolers: each head's outputs are those of the call with that head alone."""
import ctypes
import re

import numpy as np
import pytest

import resnet_c_amd as R
import views as V
from resnet_c_amd import _lib as L
from resnet_c_amd import detection as D
from resnet_c_amd import fpn as P
from resnet_c_amd import keypoint as KP
from resnet_c_amd import mask as MK
from resnet_c_amd import ops
from resnet_c_amd import roi as RO
from resnet_c_amd import rpn as RP
from resnet_c_amd import weights as W
from test_segmentation_gpu import small_head

pytestmark = pytest.mark.gpu

F = np.float32
IMAGE = (32, 32)


def launches():
    return int(L.lib().rn_ctx_launch_count(R.get_ctx().handle))


def u64s(*v):
    return (ctypes.c_uint64 * len(v))(*v)


def ptrs(*views):
    return (ctypes.c_void_p * len(views))(*[v.ptr for v in views])


def out_views(spec):
    """one poisoned view between guard bands per output of a spec name -> (dtype, shape)"""
    return {k: V.place_out(int(np.prod(sh)) * np.dtype(t).itemsize) for k, (t, sh) in spec.items()}


def finish(st, outs):
    ctx = R.get_ctx()
    msg = (L.lib().rn_last_error(ctx.handle) or b"").decode() if st != L.RN_OK else ""
    ctx.sync()
    return st, msg, outs


class Neck:
    """(64, 128) -> 64 with the pooled level, on 2x2 and 1x1 maps; larger: more images and more pixels on every level"""
    prefix, twice, grow = "rn_fpn", ("inner_blocks.1.0.weight", "layer_blocks.0.0.bias"), 1
    steps = ((1, ((2, 2), (1, 1))), (2, ((4, 3), (3, 2))), (1, ((2, 2), (1, 1))))

    def make(self):
        return P.FeaturePyramidNetwork((64, 128), 64, P.generate_fpn_state((64, 128), 64, seed=5), extra="pool")

    def call(self, obj, step):
        B, hw = self.steps[step]
        g = np.random.default_rng(100 + step)
        xs = [V.place(g.standard_normal((B, h, w, c), dtype=F)) for (h, w), c in zip(hw, (64, 128))]
        sizes = hw + (((hw[1][0] - 1) // 2 + 1, (hw[1][1] - 1) // 2 + 1),)
        outs = {n: V.place_out(B * 64 * h * w * 4) for n, (h, w) in zip(obj.names, sizes)}
        st = L.lib().rn_fpn_forward(obj.handle, ptrs(*xs), B, u64s(*[h for h, _ in hw]), u64s(*[w for _, w in hw]),
                                    ptrs(*outs.values()))
        return finish(st, outs)


class Rpn:
    """C = 64, one level, one anchor, on a 2x2 map; larger: images, pixels and pre_nms_top_n"""
    prefix, twice, grow = "rn_rpn", ("head.conv.0.0.weight", "head.bbox_pred.bias"), 1
    steps = ((1, 2, 2, 2), (2, 3, 3, 4), (1, 2, 2, 2))

    def make(self):
        return RP.RegionProposalNetwork(64, RP.AnchorGenerator(sizes=((16,),), aspect_ratios=(1.0,)),
                                        RP.generate_rpn_state(64, 1, seed=5, std=0.05), pre_nms_top_n=2, post_nms_top_n=2)

    def call(self, obj, step):
        B, h, w, obj.pre = self.steps[step]
        x = V.place(np.random.default_rng(110 + step).standard_normal((B, h, w, 64), dtype=F))
        outs = out_views(obj.buffers(B, True)[0])
        req = obj.request(outs)
        st = L.lib().rn_rpn_forward(obj.handle, ptrs(x), B, u64s(h), u64s(w), *IMAGE, ctypes.byref(req))
        return finish(st, outs)


class BoxHead:
    """F = 64, M = 64, C = 2, R = 2; larger: images and R"""
    prefix, twice, grow = "rn_box_head", ("box_head.fc7.weight", "box_predictor.cls_score.bias"), 1
    steps = ((1, 2), (2, 3), (1, 2))

    def make(self):
        return D.BoxHead(64, 1, 64, 2, D.generate_box_head_state(64, 64, 2, seed=5), score_thresh=0.0, detections_per_img=2)

    def call(self, obj, step):
        B, Rn = self.steps[step]
        g = np.random.default_rng(120 + step)
        K = B * Rn
        lo = g.uniform(0, 12, (K, 2)).astype(F)
        rois = np.concatenate([np.repeat(np.arange(B, dtype=F), Rn)[:, None], lo, lo + g.uniform(4, 16, (K, 2)).astype(F)], axis=1)
        x, r = V.place(np.maximum(g.standard_normal((K, 64), dtype=F), 0)), V.place(rois)
        outs = out_views(D.output_spec(B, Rn, 2, obj.detections_per_img, True))
        req = obj.request(outs)
        st = L.lib().rn_box_head_forward(obj.handle, x.ptr, r.ptr, B, Rn, *IMAGE, ctypes.byref(req), None)
        return finish(st, outs)


def small_tail():
    """this file's neck, an rpn over its three levels and its box head: what a RoI head runs behind"""
    net = RP.RegionProposalNetwork(64, RP.AnchorGenerator(sizes=((8,), (16,), (32,)), aspect_ratios=(1.0,)),
                                   RP.generate_rpn_state(64, 1, seed=6, std=0.05), pre_nms_top_n=4, post_nms_top_n=3)
    return Neck().make(), net, BoxHead().make()


def behind(tail, seed, levels=(), **heads):
    """2 images of 2 detections each through the tail (maps of 4x4 and 2x2) and the RoI heads given"""
    neck, net, bh = tail
    g = np.random.default_rng(seed)
    maps = [g.standard_normal((2, 4, 4, 64), dtype=F), g.standard_normal((2, 2, 2, 128), dtype=F)]
    return neck.forward(maps, levels=levels, image_size=IMAGE, rpn=net, pooler=RO.MultiScaleRoIAlign(["0", "1"], 1, 2), box_head=bh,
                        **heads)


MASK_KEYS = ("mask_rois", "mask_pooled", "mask_probs", "masks", "mask_bits")
KEYPOINT_KEYS = ("keypoint_rois", "keypoint_pooled", "keypoint_heatmaps", "keypoints", "keypoints_scores")


class MaskHead:
    """Cin = 64, one layer of 64, Cr = 64, C = 2, M = 2; larger: rows, then rows with the RoI rows and pooled features of a
    forward behind a neck (rn_fpn_forward_masks: step "pool")"""
    prefix, twice, grow = "rn_mask_head", ("mask_head.0.0.weight", "mask_predictor.conv5_mask.bias"), 1
    steps = (1, 3, "pool", 1)

    def __init__(self):
        self.tail = None

    def make(self):
        return MK.MaskHead(64, (64,), 64, 2, MK.generate_mask_head_state(64, (64,), 64, 2, seed=5), resolution=2,
                           featmap_names=("0", "1"))

    def call(self, obj, step):
        K = self.steps[step]
        g = np.random.default_rng(130 + step)
        lo = g.uniform(0, 12, (K, 2)).astype(F)
        x = V.place(np.maximum(g.standard_normal((K, 2, 2, 64), dtype=F), 0))
        lab, box = V.place(np.ones(K, np.int32)), V.place(np.concatenate([lo, lo + g.uniform(4, 16, (K, 2)).astype(F)], axis=1))
        outs = out_views(MK.output_spec(1, K, 2, 64, IMAGE, ("probs", "image", "bits")))
        req = obj.request(outs)
        st = L.lib().rn_mask_head_forward(obj.handle, x.ptr, lab.ptr, box.ptr, K, *IMAGE, ctypes.byref(req))
        return finish(st, outs)

    def behind_a_neck(self, obj):
        """2 images of 2 detections each through a neck, an rpn and a box head of this test's: 4 rows with pool"""
        self.tail = self.tail or small_tail()
        out = behind(self.tail, 139, mask_head=obj, masks=("probs", "image", "bits"), mask_pooled=True)
        return {k: np.ascontiguousarray(out[k]).view(np.uint8) for k in MASK_KEYS}

    def close(self):
        for o in self.tail or ():
            o.close()
        self.tail = None


class KeypointHead(MaskHead):
    """Cin = 64, one layer of 64, Kp = 2, M = 2; larger: rows, then rows with the RoI rows and pooled features of a forward
    behind a neck (rn_fpn_forward_keypoints: step "pool")"""
    prefix, twice = "rn_keypoint_head", ("keypoint_head.0.weight", "keypoint_predictor.kps_score_lowres.bias")

    def make(self):
        return KP.KeypointHead(64, (64,), 2, KP.generate_keypoint_head_state(64, (64,), 2, seed=5), resolution=2,
                               featmap_names=("0", "1"))

    def call(self, obj, step):
        K = self.steps[step]
        g = np.random.default_rng(140 + step)
        lo = g.uniform(0, 12, (K, 2)).astype(F)
        x = V.place(np.maximum(g.standard_normal((K, 2, 2, 64), dtype=F), 0))
        lab, box = V.place(np.ones(K, np.int32)), V.place(np.concatenate([lo, lo + g.uniform(4, 16, (K, 2)).astype(F)], axis=1))
        outs = out_views(KP.output_spec(1, K, 2, 64, 2, ("keypoints", "heatmaps")))
        req = obj.request(outs)
        st = L.lib().rn_keypoint_head_forward(obj.handle, x.ptr, lab.ptr, box.ptr, K, *IMAGE, ctypes.byref(req))
        return finish(st, outs)

    def behind_a_neck(self, obj):
        self.tail = self.tail or small_tail()
        out = behind(self.tail, 149, keypoint_head=obj, keypoints=KP.KEYPOINT_OUTPUTS)
        return {k: np.ascontiguousarray(out[k]).view(np.uint8) for k in KEYPOINT_KEYS}


class SegHead:
    """small_head of test_segmentation_gpu.py as it is: 64 channels, 5 classes; larger: images and pixels"""
    prefix, grow = "rn_seg_head", 1
    steps = ((1, 2, 2), (2, 4, 3), (1, 2, 2))
    written = {"scores": np.float32, "labels": np.uint8}   # no element of either keeps the outputs' fill

    def __init__(self, kind, dtype, rates, twice):
        self.kind, self.dtype, self.rates, self.twice = kind, dtype, rates, twice

    def make(self):
        return small_head(self.kind, self.dtype, self.rates)[0]()

    def call(self, obj, step):
        B, h, w = self.steps[step]
        H, Wd = 2 * h + 1, 3 * w
        x = np.random.default_rng(40 + step).standard_normal((B, h, w, 64), dtype=F)
        vi = V.place(ops.to_bf16_bits(x).reshape(x.shape) if self.dtype == "bf16" else x)
        outs = {"scores": V.place_out(B * 5 * H * Wd * 4), "labels": V.place_out(B * H * Wd)}
        st = L.lib().rn_seg_head_forward(obj.handle, vi.ptr, B, h, w, H, Wd, outs["scores"].ptr, outs["labels"].ptr)
        return finish(st, outs)


# the DeepLab case of the set-twice test: bf16 on a 2 x 2 map with rates (2, 3), where both dilated branches run on their
# centre tap, so a centre-tap copy of the garbage would show
KINDS = {"neck": Neck, "rpn": Rpn, "box_head": BoxHead, "mask_head": MaskHead, "keypoint_head": KeypointHead,
         "fcn": lambda: SegHead("fcn", "f32", (1, 2), ("classifier.0.weight", "classifier.1.running_var")),
         "deeplab": lambda: SegHead("deeplab", "bf16", (2, 3), ("classifier.0.convs.1.0.weight", "classifier.0.convs.2.1.bias"))}


@pytest.fixture(params=list(KINDS))
def kind(request):
    k = KINDS[request.param]()
    yield k
    getattr(k, "close", lambda: None)()


def run(kind, obj, step):
    """one forward at steps[step] -> name -> the output's bytes; every guard intact"""
    if kind.steps[step] == "pool":
        return kind.behind_a_neck(obj)
    st, msg, outs = kind.call(obj, step)
    assert st == L.RN_OK, (step, st, msg)
    written = getattr(kind, "written", {})
    return {k: V.fetch(v, written.get(k, np.uint8), f"{kind.prefix} step {step}: {k}", written=k in written).view(np.uint8)
            for k, v in outs.items()}


def same(got, want):
    return sorted(got) == sorted(want) and all(np.array_equal(got[k], want[k]) for k in want)


def fresh_run(kind, step):
    obj = kind.make()
    try:
        return run(kind, obj, step)
    finally:
        obj.close()


def set_tensor(h, prefix, key, arr, numel=None):
    """one raw <prefix>_set_tensor -> (status, rn_last_error text)"""
    lib, ctx = L.lib(), R.get_ctx()
    arr = np.ascontiguousarray(arr, dtype=F)
    st = getattr(lib, prefix + "_set_tensor")(h, key.encode(), arr.ctypes.data, arr.size if numel is None else numel)
    return st, (lib.rn_last_error(ctx.handle) or b"").decode() if st != L.RN_OK else ""


def hook(monkeypatch, fn):
    """the objects' constructors give their tensors through L.set_tensors: fn(original, handle, prefix, ctx, shapes, state)
    runs in its place, on the created object before it is finalized"""
    orig = L.set_tensors
    monkeypatch.setattr(L, "set_tensors", lambda *a: fn(orig, *a))


def test_tensor_set_twice(kind, monkeypatch):
    """garbage (1e3) under a weight key and a bias or batch-norm key, then the right values, before finalize: the bits of
    an object that was set once"""
    want = fresh_run(kind, 0)
    seen = []

    def twice(orig, h, prefix, ctx, shapes, state):
        for key in kind.twice:
            assert set_tensor(h, prefix, key, np.full(int(np.prod(shapes[key])), 1e3, F)) == (L.RN_OK, ""), key
            seen.append(key)
        orig(h, prefix, ctx, shapes, state)

    hook(monkeypatch, twice)
    assert same(fresh_run(kind, 0), want)
    assert seen == list(kind.twice)


def test_scratch_growth_keeps_the_bits(kind):
    """one object on the small shape, then larger in every capacity it has, then the small shape again -- its scratch
    grows, then is larger than needed: every result is, bit for bit, that of a fresh object on the same input"""
    obj = kind.make()
    try:
        for step in range(len(kind.steps)):
            want = fresh_run(kind, step)
            assert same(run(kind, obj, step), want), (kind.prefix, step)
    finally:
        obj.close()


def test_numel_message(kind, monkeypatch):
    """a set_tensor with numel one short: RN_ERR_INVALID, and the text holds the key, the given count and the wanted
    count, in that order"""
    seen = []

    def short(orig, h, prefix, ctx, shapes, state):
        for key, shape in shapes.items():
            seen.append((key, int(np.prod(shape)), set_tensor(h, prefix, key, state[key], int(np.prod(shape)) - 1)))
        orig(h, prefix, ctx, shapes, state)

    hook(monkeypatch, short)
    kind.make().close()
    assert seen
    for key, n, (st, msg) in seen:
        assert st == L.RN_ERR_INVALID and msg.startswith(kind.prefix + "_set_tensor: "), (key, st, msg)
        assert re.search(rf"{re.escape(key)} has {n - 1} elements, not {n}$", msg), (key, n, msg)


def test_missing_key_is_named(kind, monkeypatch):
    """finalize with exactly one tensor left out (one from the middle of the table) names that tensor's key and
    launches nothing; the object finalizes once the tensor is there"""
    seen = []

    def one_left_out(orig, h, prefix, ctx, shapes, state):
        lib, out = L.lib(), list(shapes)[len(shapes) // 2]
        for key in shapes:
            if key != out:
                assert set_tensor(h, prefix, key, state[key]) == (L.RN_OK, ""), key
        n0 = launches()
        st = getattr(lib, prefix + "_finalize")(h)
        seen.append((out, st, (lib.rn_last_error(ctx.handle) or b"").decode(), launches() - n0))
        orig(h, prefix, ctx, shapes, state)

    hook(monkeypatch, one_left_out)
    kind.make().close()
    (out, st, msg, launched), = seen
    assert st == L.RN_ERR_INVALID and msg == f"{kind.prefix}_finalize: {out} is not set" and launched == 0, (out, st, msg, launched)


@pytest.fixture(scope="module")
def held():
    """a ResNet-18 at 32 x 32 on the shared context, its input and logits on the device: what a graph is captured from"""
    m = R.NativeModel("resnet18", state=W.generate_state("resnet18", seed=1), input_size=IMAGE)
    x = W.generate_input(1, seed=7, hw=IMAGE)
    m.forward(x, fused=True)
    xd, out = R.FloatTensor.from_numpy(x, R.Device.GPU), R.FloatTensor((1, 1000), R.Device.GPU)
    yield m, xd, out
    m.close()


def test_growth_is_refused_while_a_graph_lives(kind, held):
    """While a captured graph of the context lives an object may reserve its first scratch (nothing of it can be in the
    graph) but not grow it: RN_ERR_INVALID, no launch, no output byte touched.  Once the graph is gone the same call
    runs, with the bits of a fresh object.  The graph only lives; it is not replayed."""
    m, xd, out = held
    want = fresh_run(kind, kind.grow)
    obj = kind.make()
    g = R.Graph(m, xd.data(), 1, out.data(), True)
    try:
        st, msg, _ = kind.call(obj, 0)
        assert st == L.RN_OK, msg
        n0 = launches()
        st, msg, outs = kind.call(obj, kind.grow)
        assert st == L.RN_ERR_INVALID and msg.endswith(f"{kind.prefix}: the scratch cannot grow while a captured graph lives"), (st, msg)
        assert launches() == n0, "a refusal launches nothing"
        for k, v in outs.items():
            V.assert_untouched(v, f"{kind.prefix}: refused growth: {k}")
        g.close()
        assert same(run(kind, obj, kind.grow), want)
    finally:
        g.close()
        obj.close()


TWO_HEADS_SEED = 139   # at least one of the four detections has a label >= 1 (asserted below)


def test_two_heads_with_two_poolers_in_one_call():
    """A mask head on levels ("0", "1") at resolution 2, two samples, and a keypoint head on level ("1",) at resolution 1,
    one sample, in ONE forward: every output of either head holds the bytes of the same call with that head alone, each
    head's pooled features are ops.roi_align_nhwc on the exported levels with that head's own scales and thresholds, and
    no output keeps its poison.  A slot that read the other's scales, thresholds, resolution or scratch shows here."""
    tail = small_tail()
    mh = MaskHead().make()
    kh = KP.KeypointHead(64, (64,), 2, KP.generate_keypoint_head_state(64, (64,), 2, seed=5), resolution=1, featmap_names=("1",),
                         sampling_ratio=1)
    mh.poison = kh.poison = True
    mask_kw = dict(mask_head=mh, masks=("probs", "image", "bits"), mask_pooled=True)
    kp_kw = dict(keypoint_head=kh, keypoints=KP.KEYPOINT_OUTPUTS)
    try:
        both = behind(tail, TWO_HEADS_SEED, ("0", "1"), **mask_kw, **kp_kw)
        alone = {MASK_KEYS: behind(tail, TWO_HEADS_SEED, ("0", "1"), **mask_kw),
                 KEYPOINT_KEYS: behind(tail, TWO_HEADS_SEED, ("0", "1"), **kp_kw)}
    finally:
        for o in (mh, kh) + tail:
            o.close()
    print("labels", both["labels"].tolist(), "detections", both["detections"].tolist())
    assert (both["labels"] >= 1).any(), "the comparison would be of zeros"
    for (keys, one), head in zip(alone.items(), (mh, kh)):
        for k in keys:
            raw = np.ascontiguousarray(both[k]).view(np.uint8)
            V.check_written(raw, both[k].dtype.itemsize, k)
            assert np.array_equal(raw, np.ascontiguousarray(one[k]).view(np.uint8)), k
        maps = [np.ascontiguousarray(both[n].transpose(0, 2, 3, 1)) for n in head.pooler.featmap_names]
        scales = RO.infer_scales([m.shape[1:3] for m in maps], IMAGE)
        want = ops.roi_align_nhwc(maps, both[keys[0]], scales, head.resolution, head.pooler.sampling_ratio, False,
                                  head.pooler.thresholds(scales), validate=False)
        assert np.array_equal(both[keys[1]].view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), keys[1]
