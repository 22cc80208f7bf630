"""The detection tail behind the neck as ONE call description: the aliasing matrix over every operand group of both entry
families, the launch counts of every combination of stages, and the Python helper's refusals.

The matrix test builds every operand of rn_model_forward_detections / rn_fpn_forward_detections inside one device arena,
256 guard bytes between neighbours and a tail as long as the largest operand: wherever an output is pointed, its
extent stays inside the arena, so even a call that slipped through could write nothing it does not own."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest

import resnet_c_amd as R
import views as V
from resnet_c_amd import _lib as L
from resnet_c_amd import fpn as P
from resnet_c_amd import ops
from resnet_c_amd import roi as RO
from test_detect_gpu import MC, MD, model_head, same_entry
from test_fpn_gpu import SIZE, images, launches, nets  # noqa: F401  (nets: a fixture)
from test_rpn_gpu import NAMES5, model_rpn

gpu = pytest.mark.gpu
STAGES = R.NativeModel.STAGES
TOPK = 3


# =====================================================================================================================
# 1. the aliasing matrix
# =====================================================================================================================
class Arena:
    """one allocation, every operand GUARD bytes from its neighbours; `fill` 0xA5 (outputs) or given bytes (inputs)"""

    def __init__(self, sizes, tail, data=None):
        self.at, pos = {}, 0
        for key, n in sizes.items():
            self.at[key] = (pos, n)
            pos += -(-n // 16) * 16 + V.GUARD
        if data is None:
            self.view = V.place_out(pos + tail)
        else:
            image = np.full(pos + tail, 0xFF, np.uint8)
            for key, (lo, n) in self.at.items():
                image[lo:lo + n] = np.ascontiguousarray(data[key]).reshape(-1).view(np.uint8)
            self.view = V.place(image)

    def ptr(self, key):
        return self.view.ptr + self.at[key][0]

    def fetch(self, key, dtype):
        lo, n = self.at[key]
        return V._download(self.view)[self.view.lo + lo:self.view.lo + lo + n].view(dtype).copy()

    def restore(self):
        ctx = R.get_ctx()
        L.check(L.lib().rn_memcpy_h2d(ctx.handle, self.view.buf.ptr, self.view.image.ctypes.data, self.view.image.size), "h2d", ctx.handle)


@pytest.fixture(scope="module")
def rig(nets):
    m, neck = nets("resnet18")
    net, bh, pooler = model_rpn("resnet18"), model_head("resnet18"), RO.MultiScaleRoIAlign(["0", "1", "2", "3"], 2, 2)
    net.poison = bh.poison = False
    x = np.array(images())
    B, a, K = x.shape[0], neck.out_channels, x.shape[0] * net.post
    maps = m.forward_maps(x, STAGES)
    nhwc = {f"x{i}": np.ascontiguousarray(maps[s].transpose(0, 2, 3, 1)) for i, s in enumerate(STAGES)}
    shapes = [(B,) + neck.level_shape(n, *m.stage_shapes[STAGES[min(i, 3)]][1:]) for i, n in enumerate(NAMES5)]
    rows, C, Dn = B * net.n_levels * net.pre, MC, MD
    # group -> operand -> bytes, in the C order of each request; every one an output but the maps and rois_dev
    sizes = {
        "levels": {n: int(np.prod(s)) * 4 for n, s in zip(NAMES5, shapes)},
        "heads": {"logits": B * m.classes * 4, "features": B * m.features * 4, "probs": B * m.classes * 4,
                  "topk_prob": B * TOPK * 4, "topk_idx": B * TOPK * 8},
        "roi": {"pooled": K * a * 4 * 4, "levels_out": K * 4, "rois_dev": K * 20},
        "rpn": {"boxes": K * 16, "logits": K * 4, "levels": K * 4, "count": B * 4, "rois": K * 20, "cand_keep": rows,
                "cand_index": rows * 4, "cand_logit": rows * 4, "cand_box": rows * 16, "cand_valid": rows,
                "cand_count": B * net.n_levels * 4},
        "box": {"boxes": B * Dn * 16, "scores": B * Dn * 4, "labels": B * Dn * 4, "roi": B * Dn * 4, "count": B * 4,
                "probs": K * C * 4, "class_boxes": K * C * 16, "valid": K * C, "keep": K * C},
    }
    sizes["maps"] = {k: v.nbytes for k, v in nhwc.items()}
    tail = max(n for ops_ in sizes.values() for n in ops_.values()) + 16     # the largest operand fits behind any other
    outs = Arena({(g, k): n for g, ops_ in sizes.items() for k, n in ops_.items() if g != "maps" and k != "rois_dev"}, tail)
    ins = Arena({("maps", k): v.nbytes for k, v in nhwc.items()}, tail, {("maps", k): v for k, v in nhwc.items()})
    yield NS(m=m, neck=neck, net=net, bh=bh, pooler=pooler, x=x, xin=ops._up_raw(x), B=B, K=K, nhwc=list(nhwc.values()),
             sizes=sizes, outs=outs, ins=ins, shapes=shapes)
    net.close()
    bh.close()


def base_ptrs(rig):
    """every operand at its own place; the chain: the pooler reads the rpn's out.rois"""
    p = {key: rig.outs.ptr(key) for key in rig.outs.at}
    p.update({key: rig.ins.ptr(key) for key in rig.ins.at})
    p[("roi", "rois_dev")] = p[("rpn", "rois")]
    return p


def detections_call(rig, family, p):
    """one call of the family's detections entry point on the pointers p -> (status, text)"""
    lib, B = L.lib(), rig.B
    rreq = rig.net.request({k: NS(ptr=p[("rpn", k)]) for k in rig.sizes["rpn"]})
    dreq = rig.bh.request({k: NS(ptr=p[("box", k)]) for k in rig.sizes["box"]})
    roi = rig.pooler.request(rig.neck.names, p[("roi", "rois_dev")], rig.K, SIZE, p[("roi", "pooled")], p[("roi", "levels_out")])
    if family == "model":
        fo = L.FpnOutputs()
        for i, n in enumerate(NAMES5):
            fo.level[i] = p[("levels", n)]
        heads = L.ModelOutputs(*[p[("heads", k)] for k in rig.sizes["heads"]], TOPK)
        st = lib.rn_model_forward_detections(rig.m.handle, rig.neck.handle, rig.net.handle, rig.bh.handle, rig.xin.ptr, B,
                                             ctypes.byref(heads), (ctypes.c_int * 4)(1, 2, 3, 4), ctypes.byref(fo), ctypes.byref(rreq),
                                             ctypes.byref(roi), ctypes.byref(dreq), L.RN_FWD_FUSED)
        ctx = rig.m.ctx
    else:
        xp = (ctypes.c_void_p * 4)(*[p[("maps", k)] for k in rig.sizes["maps"]])
        op = (ctypes.c_void_p * 5)(*[p[("levels", n)] for n in NAMES5])
        hp = (ctypes.c_uint64 * 4)(*[v.shape[1] for v in rig.nhwc])
        wp = (ctypes.c_uint64 * 4)(*[v.shape[2] for v in rig.nhwc])
        st = lib.rn_fpn_forward_detections(rig.neck.handle, rig.net.handle, rig.bh.handle, xp, B, hp, wp, op, SIZE[0], SIZE[1],
                                           ctypes.byref(rreq), ctypes.byref(roi), ctypes.byref(dreq))
        ctx = rig.neck.ctx
    return st, (lib.rn_last_error(ctx.handle) or b"").decode()


def matrix_cases(rig, family):
    """(output, operand) over every ordered pair of two different groups of the family; leaves out none"""
    groups = ("levels", "heads" if family == "model" else "maps", "roi", "rpn", "box")
    inputs = {("roi", "rois_dev")} | {("maps", k) for k in rig.sizes["maps"]}
    for ga in groups:
        for xa in rig.sizes[ga]:
            if (ga, xa) in inputs:
                continue
            for gb in groups:
                if gb != ga:
                    for yb in rig.sizes[gb]:
                        yield (ga, xa), (gb, yb)


@gpu
@pytest.mark.parametrize("family", ["model", "neck"])
def test_aliasing_matrix(rig, family):
    """An output of one group pointed into an operand of another: RN_ERR_INVALID with a text that names an overlap, no
    launch, no byte changed.  Then the one legal alias, rois_dev == out.rois with K == B * post: the detections of the
    Python wrapper, bit for bit."""
    base, ctx = base_ptrs(rig), (rig.m.ctx if family == "model" else rig.neck.ctx)
    st, msg = detections_call(rig, family, base)        # sizes the scratch, so that no refused call could be told by it
    assert st == L.RN_OK, msg
    ctx.sync()
    rig.outs.restore()
    n0, wrong, cases = launches(ctx), [], 0
    for out, other in matrix_cases(rig, family):
        cases += 1
        p = dict(base)
        room = rig.sizes[other[0]][other[1]]
        # 4-byte aligned and inside the operand; pooled must stay on its 16-byte boundary to get as far as the matrix
        off = (16 if room > 16 else 0) if out == ("roi", "pooled") else 4
        p[out] = base[other] + off
        unchained = out == ("rpn", "rois") and other[0] == "roi"     # refused as well, as a box head without its chain
        if out == ("rpn", "rois") and not unchained:
            p[("roi", "rois_dev")] = p[out]             # the chain moves along: what is refused is the overlap, not the chain
        st, msg = detections_call(rig, family, p)
        why = None
        if st != L.RN_ERR_INVALID or not msg:
            why = f"status {st} ({msg!r})"
        elif "overlaps" not in msg and not unchained:
            why = f"refused for another reason: {msg!r}"
        elif launches(ctx) != n0:
            why = "launched"
        if why is None:
            ctx.sync()
            try:
                V.assert_untouched(rig.outs.view, "outputs")
                V.assert_untouched(rig.ins.view, "maps")
            except AssertionError as e:
                why = str(e)
        if why is not None:
            wrong.append(f"{'.'.join(out)} into {'.'.join(other)}: {why}")
            ctx.sync()
            rig.outs.restore(), rig.ins.restore()
            n0 = launches(ctx)
    assert not wrong, f"{len(wrong)} of {cases} pairs:\n" + "\n".join(wrong)
    print(f"{family}: {cases} pairs refused")
    st, msg = detections_call(rig, family, base)
    assert st == L.RN_OK, msg
    ctx.sync()
    if family == "model":
        want = rig.m.forward_fpn(rig.x, rig.neck, rpn=rig.net, pooler=rig.pooler, box_head=rig.bh, detect_intermediates=True)
    else:
        want = rig.neck.forward(rig.nhwc, rpn=rig.net, image_size=SIZE, pooler=rig.pooler, box_head=rig.bh, detect_intermediates=True)
    names = {"count": "detections", "roi": "detection_rois"}
    for k in rig.sizes["box"]:
        ref = want[names.get(k, k)]
        assert same_entry(rig.outs.fetch(("box", k), ref.dtype).reshape(ref.shape), ref), k
    assert want["detections"].max() > 0
    V.assert_untouched(rig.ins.view, "maps")


# =====================================================================================================================
# 2. launch counts
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("family", ["model", "neck"])
def test_launch_counts_add_up(rig, family):
    """Each stage behind the neck adds what its own stand-alone object launches on the same inputs, and a level nobody
    reads adds no 3x3: stated as differences between forwards, every figure measured here."""
    m, neck, net, bh, pooler, B = rig.m, rig.neck, rig.net, rig.bh, rig.pooler, rig.B
    ctx = m.ctx if family == "model" else neck.ctx
    first = RO.MultiScaleRoIAlign(["0"], 2, 2)

    def count(fn):
        n0 = launches(ctx)
        out = fn()
        return launches(ctx) - n0, out

    def fwd(levels, **kw):
        if family == "model":
            return count(lambda: m.forward_fpn(rig.x, neck, levels=levels, **kw))
        if "rpn" in kw or "rois" in kw:
            kw["image_size"] = SIZE
        return count(lambda: neck.forward(rig.nhwc, levels=levels, **kw))

    full, pyramid = fwd(NAMES5, rpn=net, pooler=pooler, box_head=bh)
    rois, K = pyramid["rois"], B * net.post
    user = np.ascontiguousarray(rois[rois[:, 0] >= 0][::7])     # RoIs of the caller's own: the unchained pooler
    feats = {k: pyramid[k] for k in NAMES5}
    rpn_alone, _ = count(lambda: net(feats, SIZE))
    roi_alone, _ = count(lambda: pooler(feats, user, SIZE))
    first_alone, _ = count(lambda: first(feats, user, SIZE))
    box_alone, _ = count(lambda: bh(pyramid["pooled"], rois, B, SIZE))
    assert rpn_alone > 0 and roi_alone > 0 and first_alone > 0 and box_alone > 0
    with pytest.raises(L.RnError, match="nothing wanted"):
        fwd(())                                         # neck only, no level: nothing to do, nothing launched
    both = {}
    for levels in ((), ("0", "pool")):
        n_rpn = fwd(levels, rpn=net)[0]
        n_both = both[levels] = fwd(levels, rpn=net, rois=user, pooler=pooler)[0]
        n_chain = fwd(levels, rpn=net, pooler=pooler)[0]
        n_det = fwd(levels, rpn=net, pooler=pooler, box_head=bh)[0]
        assert n_both - n_rpn == roi_alone, (levels, "the unchained pooler behind the rpn")
        assert n_chain - n_rpn == roi_alone, (levels, "the chained pooler")
        assert n_det - n_chain == box_alone, (levels, "the box stage")
    export = (fwd(("0", "pool"), rpn=net)[0] - fwd((), rpn=net)[0]) // 2
    assert fwd((), rpn=net)[0] == fwd(NAMES5)[0] - 5 * export + rpn_alone, "the rpn behind a neck that exports nothing"
    assert (fwd(("0", "pool"), rpn=net)[0] - fwd((), rpn=net)[0]) % 2 == 0
    # behind a pooler that reads every level the rpn adds itself, and the pool where nobody exported it
    pool = fwd(("3", "pool"))[0] - fwd(("3",))[0] - export
    assert both[("0", "pool")] - fwd(("0", "pool"), rois=user, pooler=pooler)[0] == rpn_alone
    assert both[()] - fwd((), rois=user, pooler=pooler)[0] == rpn_alone + pool
    assert full == fwd(NAMES5)[0] + rpn_alone + roi_alone + box_alone, "the whole tail behind the whole pyramid"
    # a level nobody reads adds no 3x3 launch: a pooler on level 0 alone adds its own launch to a forward that exports
    # level 0, and the pooler on four levels adds what exporting levels 1 and 2 adds, less their two exports
    lv = ("0", "pool")
    n_neck = fwd(lv)[0]
    assert fwd(lv, rois=user, pooler=first)[0] == n_neck + first_alone
    assert fwd(lv, rois=user, pooler=pooler)[0] - n_neck - roi_alone == fwd(("0", "1", "2", "pool"))[0] - n_neck - 2 * export
    assert fwd(("0",), rois=user, pooler=first)[0] < fwd(lv, rois=user, pooler=first)[0]


# =====================================================================================================================
# 3. the Python helper: the same ValueErrors from both callers, before anything touches a device
# =====================================================================================================================
class StubCtx:
    """a context nothing may reach: any use of it is the failure"""

    def __getattr__(self, name):
        raise AssertionError(f"the context was reached ({name}) before the arguments were refused")


class StubModel(R.NativeModel):
    input_size = (64, 64)

    def __init__(self):
        self.ctx, self.handle = StubCtx(), None


class StubNeck(P.FeaturePyramidNetwork):
    def __init__(self):
        self.ctx, self.handle = StubCtx(), None
        self.in_channels_list, self.out_channels, self.extra, self.dtype = (64, 128, 256, 512), 64, 1, "f32"


ROIS = np.zeros((2, 5), np.float32)
BAD = [
    dict(rois=ROIS),                                            # rois without a pooler
    dict(pooler="P"),                                           # a pooler without rois (and no rpn to chain behind)
    dict(box_head="H"),                                         # a box head alone
    dict(box_head="H", rois=ROIS, pooler="P"),                  # ... behind a pooler, still without an rpn
    dict(box_head="H", pooler="P"),
    dict(box_head="H", rois=ROIS),
    dict(rpn="N", rois=ROIS),                                   # the rpn's route: rois need a pooler
    dict(rpn="N", rois=ROIS, box_head="H"),
    dict(rpn="N", box_head="H"),                                # a box head without a pooler
    dict(rpn="N", box_head="H", pooler="P", rois=ROIS),         # a box head with rois: the pooler must chain
    dict(rpn="N", box_head="H", rois=ROIS, roi_levels=True),
    dict(rpn="N", box_head="H", detect_intermediates=True, candidates=True),
]


@pytest.mark.parametrize("kw", BAD, ids=[" ".join(sorted(k)) + f" #{i}" for i, k in enumerate(BAD)])
def test_bad_combinations_raise_before_any_device_work(kw):
    assert len(BAD) == 12
    neck, model = StubNeck(), StubModel()
    maps = [np.zeros((2, 4, 4, c), np.float32) for c in neck.in_channels_list]
    with pytest.raises(ValueError):
        neck.forward(maps, image_size=(64, 64), **kw)
    with pytest.raises(ValueError):
        model.forward_fpn(np.zeros((2, 3, 64, 64), np.float32), neck, **kw)


# =====================================================================================================================
# 4. the operand lists under the host sanitizers: a stand-alone program, nothing of it is loaded into this process
# =====================================================================================================================
def test_operand_lists_under_the_host_sanitizers(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "operands_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",   # the runtimes inside the program
                    f"-I{root}/resnet.c_amd/csrc", f"{root}/examples/operands_check.cpp", "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "every expectation holds" in r.stdout, r.stdout + r.stderr
