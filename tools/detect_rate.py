#!/usr/bin/env python3
"""What the box head costs: the launches behind the pooler at the RPN profile's workload.

    python tools/detect_rate.py [--rounds 5] [--reps 5] [--batches 1 4] [--rois 1000] [--classes 91] [--detections 100]

An 800 x 1344 image, a = 256 channels pooled to 7 x 7 (in_features 12544), representation 1024, R = 1000 RoIs per image,
C = 91 classes, D = 100.  Per batch size, ms as the best of `rounds` windows of `reps` calls between two events and the
spread of the windows, for
  - each of the three contractions alone (rn_conv2d_nhwc_forward_dt as a 1x1 on [K,1,1,F] with the bias and ReLU the
    object gives it), beside its FLOPs and the TFLOP/s that makes;
  - rn_detect_postprocess_forward (three launches) on a head output whose scores and boxes resemble a detector's:
    clustered proposals, one raised class per cluster, so that most (image, class) pairs are empty and a few hold a
    cluster's worth of overlapping candidates; beside it the bytes the stage has to move once;
  - rn_box_head_forward, the six (to nine) launches through the object.
The three launches of the post-processing are one entry point; their separate times come from a kernel trace of this
tool (profiles/detect/README.md says how it was taken)."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import detection as D
from resnet_c_amd import ops
from resnet_c_amd.tensor import _DeviceBuffer

IMAGE, A, RES, REP = (800, 1344), 256, 7, 1024


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


def proposals(g, B, Rn):
    """[B*Rn, 5]: per image Rn // 6 clusters, every RoI a cluster's box jittered by up to 8 % of its size"""
    rois = np.zeros((B * Rn, 5), np.float32)
    for b in range(B):
        m = max(1, Rn // 6)
        cx, cy, w, h = g.uniform(0, IMAGE[1], m), g.uniform(0, IMAGE[0], m), g.uniform(32, 400, m), g.uniform(32, 400, m)
        c = g.integers(0, m, Rn)
        size = np.stack([w[c], h[c], w[c], h[c]], axis=1)
        box = np.stack([cx[c] - w[c] / 2, cy[c] - h[c] / 2, cx[c] + w[c] / 2, cy[c] + h[c] / 2], axis=1)
        box = np.clip(box + g.uniform(-1, 1, (Rn, 4)) * 0.08 * size, 0, [IMAGE[1], IMAGE[0], IMAGE[1], IMAGE[0]])
        rois[b * Rn:(b + 1) * Rn, 0], rois[b * Rn:(b + 1) * Rn, 1:] = b, box
        hot = c if b == 0 else np.concatenate([hot, c])
    return rois, hot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 4])
    ap.add_argument("--rois", type=int, default=1000)
    ap.add_argument("--classes", type=int, default=91)
    ap.add_argument("--detections", type=int, default=100)
    a = ap.parse_args()
    lib, ctx = L.lib(), R.get_ctx()
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    lib.rn_event_create(ctx.handle, ctypes.byref(e0)), lib.rn_event_create(ctx.handle, ctypes.byref(e1))
    Rn, C, Dn, Fi = a.rois, a.classes, a.detections, A * RES * RES
    P = D.head_pitch(C)
    g = np.random.default_rng(0)
    state = D.generate_box_head_state(Fi, REP, C, seed=0)
    bh = D.BoxHead(A, RES, REP, C, state, detections_per_img=Dn)
    layers = (("fc6", Fi, REP, 1), ("fc7", REP, REP, 1), ("predictor", REP, P, 0))
    packed = {}
    for name, cin, cout, _ in layers:
        raw = ops._up_raw(g.standard_normal((cout, cin)).astype(np.float32) / np.sqrt(cin))
        n = int(lib.rn_conv2d_packed_weight_numel_dt(L.RN_DTYPE_F32, cin, cout, 1))
        pk = _DeviceBuffer(ctx, n * 4)
        L.check(lib.rn_conv2d_pack_weight_dt(ctx.handle, L.RN_DTYPE_F32, raw.ptr, pk.ptr, cin, cout, 1), "pack", ctx.handle)
        packed[name] = (pk, ops._up_raw(np.zeros(cout, np.float32)))
    ctx.sync()
    saved_layout = lib.rn_ctx_get_layout(ctx.handle)
    ctx.set_layout(L.RN_LAYOUT_NHWC)
    for B in a.batches:
        K = B * Rn
        rois, hot = proposals(g, B, Rn)
        logits = (g.standard_normal((K, C)) * 1.5).astype(np.float32)
        logits[np.arange(K), hot % (C - 1) + 1] += 5.0
        head = ops._up_raw(D.pack_head(logits, (g.standard_normal((K, 4 * C)) * 0.5).astype(np.float32)))
        drois = ops._up_raw(rois)
        pooled = ops._up_raw(np.maximum(g.standard_normal((K, Fi), dtype=np.float32), 0))
        acts = {Fi: pooled, REP: _DeviceBuffer(ctx, K * REP * 4), P: _DeviceBuffer(ctx, K * P * 4)}
        rec = {"B": B, "R": Rn, "C": C, "D": Dn, "in_features": Fi, "representation": REP}
        for name, cin, cout, relu in layers:
            pk, bias = packed[name]
            src, dst = acts[cin], (_DeviceBuffer(ctx, K * cout * 4) if cin == cout else acts[cout])
            ep = L.Epilogue(None, bias.ptr, None, relu)

            def run(src=src, dst=dst, pk=pk, cin=cin, cout=cout, ep=ep):
                L.check(lib.rn_conv2d_nhwc_forward_dt(ctx.handle, L.RN_DTYPE_F32, L.RN_DTYPE_F32, src.ptr, dst.ptr, pk.ptr, 1, 1, 0,
                                                      1, 1, K, cin, cout, 1, 1, ctypes.byref(ep)), name, ctx.handle)

            t, s = timed(lib, ctx, (e0, e1), run, a.rounds, a.reps)
            flops = 2.0 * K * cin * cout
            rec.update({f"{name}_ms": round(t, 4), f"{name}_spread_ms": round(s, 4), f"{name}_gflop": round(flops / 1e9, 2),
                        f"{name}_tflop_per_s": round(flops / t / 1e9, 1)})
        spec, bufs = bh.buffers(B, Rn)
        req = bh.request(bufs)

        def post():
            L.check(lib.rn_detect_postprocess_forward(ctx.handle, head.ptr, drois.ptr, B, Rn, C, IMAGE[0], IMAGE[1], ctypes.byref(req)),
                    "postprocess", ctx.handle)

        def whole():
            L.check(lib.rn_box_head_forward(bh.handle, pooled.ptr, drois.ptr, B, Rn, IMAGE[0], IMAGE[1], ctypes.byref(req), None),
                    "rn_box_head_forward", ctx.handle)

        t_post, s_post = timed(lib, ctx, (e0, e1), post, a.rounds, a.reps)
        ctx.sync()
        count = ops._down_raw(bufs["count"], np.int32, B)
        # what the stage moves once: the head rows in, the class boxes out and in again, 12 bytes of order words and keys
        moved = K * P * 4 + K * 20 + 2 * K * C * 16 + K * (C - 1) * 12
        rec.update({"postprocess_3_launches_ms": round(t_post, 4), "postprocess_spread_ms": round(s_post, 4),
                    "postprocess_mb_moved_once": round(moved / 1e6, 2), "postprocess_gb_per_s": round(moved / t_post / 1e6, 1),
                    "detections": count.tolist()})
        t_all, s_all = timed(lib, ctx, (e0, e1), whole, a.rounds, a.reps)
        rec.update({"box_head_forward_ms": round(t_all, 4), "box_head_forward_spread_ms": round(s_all, 4)})
        print(json.dumps(rec), flush=True)
        del head, drois, pooled, acts
    ctx.set_layout(saved_layout)
    bh.close()


if __name__ == "__main__":
    main()
