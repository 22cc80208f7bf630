#!/usr/bin/env python3
"""What the keypoint head costs: the launches behind the box head at torchvision's keypointrcnn_resnet50_fpn shapes.

    python tools/keypoint_rate.py [--rounds 5] [--reps 5] [--batches 1 4] [--detections 100]

An 800 x 1344 image, a = 256 channels pooled to 14 x 14, eight 3x3 layers of 512, Kp = 17 keypoints, D = 100 detections
per image.  Per batch size, ms as the best of `rounds` windows of `reps` calls between two events and the spread of the
windows, for
  - one 3x3 layer of 512 -> 512 (rn_conv2d_nhwc_forward_dt with the bias and ReLU the object gives it) beside its FLOPs,
    the TFLOP/s that makes and the share of the fp32 MFMA roof (157.3 TFLOP/s);
  - the transposed convolution as its 1x1 panel of 16 * Kp = 272 channels, likewise;
  - rn_keypoint_predict_forward (keypoints and scores only: no heat map reaches memory) on boxes of 32 .. 400 pixels,
    beside the resized pixels it searches (the sum over detections of Kp * ceil(w) * ceil(h)) and the pixels per ns that
    makes, and beside rn_paste_masks_forward (fp32 masks of 28 x 28 probabilities) on the same boxes: the tree's other
    per-box-pixel kernel.  The paste writes K planes of the image; the search writes 4 * Kp floats per detection;
  - the same launch with the heat maps [K, 17, 56, 56] written as well;
  - rn_keypoint_head_forward through the object (the stage without its pooler) and the predict launch's share of it;
  - the RoI former and the NHWC pooler on a seeded pyramid of the image's four levels."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import keypoint as KP
from resnet_c_amd import ops
from resnet_c_amd.tensor import _DeviceBuffer

IMAGE, A, M, KPN, LAYERS = (800, 1344), 256, 14, 17, (512,) * 8
MFMA_F32_FLOP_PER_MS = 157.3e9


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


def detections(g, K):
    """[K, 4]: boxes of 32 .. 400 pixels inside the image (tools/mask_rate.py's draw)"""
    cx, cy, w, h = g.uniform(0, IMAGE[1], K), g.uniform(0, IMAGE[0], K), g.uniform(32, 400, K), g.uniform(32, 400, K)
    box = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=1)
    return np.clip(box, 0, [IMAGE[1], IMAGE[0], IMAGE[1], IMAGE[0]]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 4])
    ap.add_argument("--detections", type=int, default=100)
    a = ap.parse_args()
    lib, ctx = L.lib(), R.get_ctx()
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    lib.rn_event_create(ctx.handle, ctypes.byref(e0)), lib.rn_event_create(ctx.handle, ctypes.byref(e1))
    ev = (e0, e1)
    Dn, H, W, C = a.detections, IMAGE[0], IMAGE[1], LAYERS[-1]
    g = np.random.default_rng(0)
    state = KP.generate_keypoint_head_state(A, LAYERS, KPN, seed=0)
    kh = KP.KeypointHead(A, LAYERS, KPN, state, resolution=M)
    packed = {}
    for name, cin, cout, k in (("conv3x3", C, C, 3), ("deconv_panel", C, 16 * KPN, 1)):
        raw = ops._up_raw((g.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32))
        n = int(lib.rn_conv2d_packed_weight_numel_dt(L.RN_DTYPE_F32, cin, cout, k))
        pk = _DeviceBuffer(ctx, n * 4)
        L.check(lib.rn_conv2d_pack_weight_dt(ctx.handle, L.RN_DTYPE_F32, raw.ptr, pk.ptr, cin, cout, k), "pack", ctx.handle)
        packed[name] = (pk, ops._up_raw(np.zeros(cout, np.float32)), cin, cout, k)
    bias = ops._up_raw(state[KP.PREDICTOR_KEYS[1]])
    ctx.sync()
    saved_layout = lib.rn_ctx_get_layout(ctx.handle)
    ctx.set_layout(L.RN_LAYOUT_NHWC)
    sizes = [(200, 336), (100, 168), (50, 84), (25, 42)]
    for B in a.batches:
        K = B * Dn
        rec = {"B": B, "D": Dn, "Kp": KPN, "M": M, "a": A, "layers": len(LAYERS), "layer_channels": C}
        boxes = detections(g, K)
        labels = np.ones(K, np.int32)
        dboxes, dlabels = ops._up_raw(boxes), ops._up_raw(labels)
        pooled = ops._up_raw(np.maximum(g.standard_normal((K, M, M, A), dtype=np.float32), 0))
        x512 = ops._up_raw(np.maximum(g.standard_normal((K, M, M, C), dtype=np.float32), 0))
        mid = _DeviceBuffer(ctx, K * M * M * C * 4)
        t_dev = _DeviceBuffer(ctx, K * M * M * 16 * KPN * 4)
        for name, (pk, shift, cin, cout, k) in packed.items():
            dst = mid if k == 3 else t_dev
            ep = L.Epilogue(None, shift.ptr if k == 3 else None, None, 1 if k == 3 else 0)

            def run(dst=dst, pk=pk, cin=cin, cout=cout, k=k, ep=ep):
                L.check(lib.rn_conv2d_nhwc_forward_dt(ctx.handle, L.RN_DTYPE_F32, L.RN_DTYPE_F32, x512.ptr, dst.ptr, pk.ptr, k, 1,
                                                      k // 2, M, M, K, cin, cout, M, M, ctypes.byref(ep)), name, ctx.handle)

            t, s = timed(lib, ctx, ev, run, a.rounds, a.reps)
            flops = 2.0 * K * M * M * cin * k * k * cout
            rec.update({f"{name}_ms": round(t, 4), f"{name}_spread_ms": round(s, 4), f"{name}_gflop": round(flops / 1e9, 2),
                        f"{name}_tflop_per_s": round(flops / t / 1e9, 1),
                        f"{name}_share_of_f32_mfma_roof": round(flops / t / MFMA_F32_FLOP_PER_MS, 3)})
        kps, scores = _DeviceBuffer(ctx, K * KPN * 12), _DeviceBuffer(ctx, K * KPN * 4)
        heat = _DeviceBuffer(ctx, K * KPN * 16 * M * M * 4)

        def predict(h=None):
            L.check(lib.rn_keypoint_predict_forward(ctx.handle, t_dev.ptr, bias.ptr, dboxes.ptr, dlabels.ptr, K, M, KPN, H, W, h, kps.ptr,
                                                    scores.ptr), "predict", ctx.handle)

        w_, h_, Wr, Hr, _ = KP.box_sizes_ref(boxes, IMAGE)
        pixels = float(KPN * (Wr * Hr).sum())
        t, s = timed(lib, ctx, ev, predict, a.rounds, a.reps)
        predict_ms = t
        rec.update({"predict_ms": round(t, 4), "predict_spread_ms": round(s, 4), "predict_resized_mpixels": round(pixels / 1e6, 2),
                    "predict_pixels_per_ns": round(pixels / t / 1e6, 2)})
        t, s = timed(lib, ctx, ev, lambda: predict(heat.ptr), a.rounds, a.reps)
        rec.update({"predict_with_heat_ms": round(t, 4), "predict_with_heat_spread_ms": round(s, 4),
                    "heat_mb_written": round(K * KPN * 16 * M * M * 4 / 1e6, 2)})
        probs = ops._up_raw(g.uniform(0, 1, (K, 2 * M, 2 * M)).astype(np.float32))
        masks = _DeviceBuffer(ctx, K * H * W * 4)

        def paste():
            L.check(lib.rn_paste_masks_forward(ctx.handle, probs.ptr, dboxes.ptr, dlabels.ptr, K, 2 * M, H, W, 0.5, masks.ptr, None),
                    "paste", ctx.handle)

        t, s = timed(lib, ctx, ev, paste, a.rounds, a.reps)
        rec.update({"paste_masks_same_boxes_ms": round(t, 4), "paste_masks_same_boxes_spread_ms": round(s, 4),
                    "paste_box_mpixels": round(float((Wr * Hr).sum()) / 1e6, 2)})
        del masks, probs
        spec, bufs = kh.buffers(1, K, ("keypoints",))
        req = kh.request(bufs)

        def whole():
            L.check(lib.rn_keypoint_head_forward(kh.handle, pooled.ptr, dlabels.ptr, dboxes.ptr, K, H, W, ctypes.byref(req)),
                    "rn_keypoint_head_forward", ctx.handle)

        t, s = timed(lib, ctx, ev, whole, a.rounds, a.reps)
        rec.update({"head_ms": round(t, 4), "head_spread_ms": round(s, 4), "predict_share_of_head": round(predict_ms / t, 3)})
        del bufs
        # the front of the stage: the RoI former and the NHWC pooler on a seeded pyramid
        maps = [ops._up_raw(g.standard_normal((B, h, w, A), dtype=np.float32)) for h, w in sizes]
        scales = np.array([0.25, 0.125, 0.0625, 0.03125], np.float32)
        thr = np.concatenate([ops.roi_level_thresholds(scales), np.zeros(1, np.float32)])
        rois = _DeviceBuffer(ctx, K * 20)
        fp = ctypes.POINTER(ctypes.c_float)
        lab2 = ops._up_raw(labels.reshape(B, Dn))
        out = _DeviceBuffer(ctx, K * M * M * A * 4)

        def former():
            L.check(lib.rn_detection_rois_forward(ctx.handle, dboxes.ptr, lab2.ptr, B, Dn, rois.ptr), "rois", ctx.handle)

        def pool():
            L.check(lib.rn_roi_align_nhwc_forward_dt(
                ctx.handle, L.RN_DTYPE_F32, 4, (ctypes.c_void_p * 4)(*[d.ptr for d in maps]), (ctypes.c_uint64 * 4)(*[h for h, _ in sizes]),
                (ctypes.c_uint64 * 4)(*[w for _, w in sizes]), scales.ctypes.data_as(fp), thr.ctypes.data_as(fp), B, A, rois.ptr, K, M, M,
                2, 0, out.ptr, None), "pool", ctx.handle)

        t, s = timed(lib, ctx, ev, former, a.rounds, a.reps)
        rec.update({"detection_rois_ms": round(t, 4)})
        t, s = timed(lib, ctx, ev, pool, a.rounds, a.reps)
        rec.update({"roi_align_nhwc_ms": round(t, 4), "roi_align_nhwc_spread_ms": round(s, 4)})
        rec["stage_ms"] = round(rec["head_ms"] + rec["detection_rois_ms"] + rec["roi_align_nhwc_ms"], 4)
        rec["predict_share_of_stage"] = round(predict_ms / rec["stage_ms"], 3)
        print(json.dumps(rec), flush=True)
        del maps, pooled, x512, mid, t_dev, heat, out
    ctx.set_layout(saved_layout)
    kh.close()


if __name__ == "__main__":
    main()
