#!/usr/bin/env python3
"""What the proposals cost: the launches behind an RPN head on a detection-sized pyramid.

    python tools/rpn_rate.py [--rounds 5] [--reps 5] [--batches 1 4] [--pre 1000] [--post 1000]

Head outputs of the pyramid of an 800 x 1344 image (200 x 336, 100 x 168, 50 x 84, 25 x 42 and the pooled 13 x 21),
A = 3 anchors of torchvision's sizes 32 .. 512 and ratios 1/2, 1, 2 per position (P = 16 channels), N(0, 1) logits and
N(0, 0.2) deltas, NMS at 0.7.  Per entry point -- rn_rpn_select_decode_forward (one launch),
rn_rpn_nms_merge_forward (two: IoU mask, scan + merge) -- and for both together: ms, the best of `rounds` windows of
`reps` calls between two events, and the spread of the windows.  Beside the select, the bytes it has to read (the head
outputs, once) and the rate that makes: the launch walks every segment nine times (eight radix passes and the gather)
with one block per (image, level), so it is far from the rate of a streaming kernel; DESIGN.md says what it waits on.
Then the whole stage through the object (rn_rpn_forward on fp32 levels of C = 256: the head's two contractions per level
and the three launches, 2 L + 3), the head's contractions as the difference, and beside it the neck alone
(rn_fpn_forward on ResNet-50's stage maps of the same image, zero-filled, every level exported)."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import ops, rpn
from resnet_c_amd.tensor import _DeviceBuffer

IMAGE, SIZES, A = (800, 1344), ((200, 336), (100, 168), (50, 84), (25, 42), (13, 21)), 3


def elapsed(lib, ctx, events, body):
    e0, e1 = events
    lib.rn_event_record(ctx.handle, e0)
    body()
    lib.rn_event_record(ctx.handle, e1)
    ms = ctypes.c_float()
    L.check(lib.rn_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "elapsed", ctx.handle)
    return ms.value


def timed(lib, ctx, events, run, rounds, reps):
    run()
    ctx.sync()
    t = [elapsed(lib, ctx, events, lambda: [run() for _ in range(reps)]) / reps for _ in range(rounds)]
    return min(t), max(t) - min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 4])
    ap.add_argument("--pre", type=int, default=1000)
    ap.add_argument("--post", type=int, default=1000)
    a = ap.parse_args()
    lib, ctx = L.lib(), R.get_ctx()
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    lib.rn_event_create(ctx.handle, ctypes.byref(e0)), lib.rn_event_create(ctx.handle, ctypes.byref(e1))
    base = np.ascontiguousarray(rpn.AnchorGenerator().base_anchors())
    n_levels, P = len(SIZES), rpn.head_channels(A)
    g = np.random.default_rng(0)
    for B in a.batches:
        heads = []
        for h, w in SIZES:
            hd = np.zeros((B, h, w, P), np.float32)
            hd[..., :A] = g.standard_normal((B, h, w, A))
            hd[..., A:5 * A] = g.standard_normal((B, h, w, 4 * A)) * 0.2
            heads.append(ops._up_raw(hd))
        head_bytes = sum(B * h * w * P * 4 for h, w in SIZES)
        rows, prop = B * n_levels * a.pre, B * a.post
        cb = [_DeviceBuffer(ctx, n) for n in (rows * 4, rows * 4, rows * 16, rows, B * n_levels * 4)]
        pb = [_DeviceBuffer(ctx, n) for n in (prop * 16, prop * 4, prop * 4, B * 4, prop * 20, rows)]
        cand, out = L.RpnCandidates(*[b.ptr for b in cb]), L.RpnProposals(*[b.ptr for b in pb])
        hp = (ctypes.c_void_p * n_levels)(*[d.ptr for d in heads])
        hs, ws = (ctypes.c_uint64 * n_levels)(*[s[0] for s in SIZES]), (ctypes.c_uint64 * n_levels)(*[s[1] for s in SIZES])

        def select():
            L.check(lib.rn_rpn_select_decode_forward(ctx.handle, n_levels, hp, B, hs, ws, A,
                                                     base.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), IMAGE[0], IMAGE[1],
                                                     a.pre, 1e-3, float("-inf"), ctypes.byref(cand)), "select", ctx.handle)

        def merge():
            L.check(lib.rn_rpn_nms_merge_forward(ctx.handle, ctypes.byref(cand), B, n_levels, a.pre, a.post, 0.7,
                                                 ctypes.byref(out)), "merge", ctx.handle)

        def both():
            select(), merge()

        both()
        ctx.sync()
        count = ops._down_raw(pb[3], np.int32, B)
        kept = int(ops._down_raw(pb[5], np.uint8, rows).sum())
        t_sel, s_sel = timed(lib, ctx, (e0, e1), select, a.rounds, a.reps)
        t_mrg, s_mrg = timed(lib, ctx, (e0, e1), merge, a.rounds, a.reps)
        t_all, s_all = timed(lib, ctx, (e0, e1), both, a.rounds, a.reps)
        print(json.dumps({"B": B, "levels": SIZES, "A": A, "pre_nms_top_n": a.pre, "post_nms_top_n": a.post, "nms_thresh": 0.7,
                          "anchors_per_image": sum(h * w * A for h, w in SIZES), "survivors": kept, "proposals": count.tolist(),
                          "select_decode_ms": round(t_sel, 4), "select_decode_spread_ms": round(s_sel, 4),
                          "head_output_mb": round(head_bytes / 1e6, 2),
                          "select_decode_gb_per_s_of_one_read": round(head_bytes / t_sel / 1e6, 1),
                          "mask_and_merge_ms": round(t_mrg, 4), "mask_and_merge_spread_ms": round(s_mrg, 4),
                          "three_launches_ms": round(t_all, 4), "three_launches_spread_ms": round(s_all, 4)}), flush=True)
        del heads
        # the whole stage through the object, and the neck alone on the same image
        from resnet_c_amd import fpn as FPN
        C = 256
        net = rpn.RegionProposalNetwork(C, rpn.AnchorGenerator(), rpn.generate_rpn_state(C, A, seed=0), a.pre, a.post, 0.7)
        lv = [ops._up_raw(g.random((B, h, w, C), dtype=np.float32) - 0.5) for h, w in SIZES]
        spec, bufs = net.buffers(B)
        req = net.request(bufs)
        lp = (ctypes.c_void_p * n_levels)(*[d.ptr for d in lv])

        def stage():
            L.check(lib.rn_rpn_forward(net.handle, lp, B, hs, ws, IMAGE[0], IMAGE[1], ctypes.byref(req)), "rn_rpn_forward", ctx.handle)

        t_stage, s_stage = timed(lib, ctx, (e0, e1), stage, a.rounds, a.reps)
        cin = (256, 512, 1024, 2048)
        neck = FPN.FeaturePyramidNetwork(cin, C, FPN.generate_fpn_state(cin, C, seed=0))
        maps = [_DeviceBuffer(ctx, B * h * w * c * 4) for c, (h, w) in zip(cin, SIZES)]
        for d, c, (h, w) in zip(maps, cin, SIZES):
            L.check(lib.rn_memset(ctx.handle, d.ptr, 0, B * h * w * c * 4), "memset", ctx.handle)
        outs = [_DeviceBuffer(ctx, B * h * w * C * 4) for h, w in SIZES]
        mp = (ctypes.c_void_p * 4)(*[d.ptr for d in maps])
        op = (ctypes.c_void_p * 5)(*[d.ptr for d in outs])
        h4, w4 = (ctypes.c_uint64 * 4)(*[s[0] for s in SIZES[:4]]), (ctypes.c_uint64 * 4)(*[s[1] for s in SIZES[:4]])

        def neck_alone():
            L.check(lib.rn_fpn_forward(neck.handle, mp, B, h4, w4, op), "rn_fpn_forward", ctx.handle)

        t_neck, s_neck = timed(lib, ctx, (e0, e1), neck_alone, a.rounds, a.reps)
        print(json.dumps({"B": B, "C": C, "stage_2L_plus_3_launches_ms": round(t_stage, 4), "stage_spread_ms": round(s_stage, 4),
                          "head_contractions_ms_by_difference": round(t_stage - t_all, 4),
                          "neck_alone_ms": round(t_neck, 4), "neck_alone_spread_ms": round(s_neck, 4),
                          "neck_note": "every level and the pool exported, as tools/fpn_rate.py times it"}),
              flush=True)
        net.close(), neck.close()
        del lv, maps, outs


if __name__ == "__main__":
    main()
