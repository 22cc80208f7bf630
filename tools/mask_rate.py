#!/usr/bin/env python3
"""What the mask head costs: the launches behind the box head at the box head profile's workload.

    python tools/mask_rate.py [--rounds 5] [--reps 5] [--batches 1 4] [--detections 100] [--classes 91]

An 800 x 1344 image, a = 256 channels pooled to 14 x 14, four 3x3 layers of 256, dim_reduced 256, C = 91 classes,
D = 100 detections per image.  Per batch size, ms as the best of `rounds` windows of `reps` calls between two events
and the spread of the windows, for
  - each contraction alone (rn_conv2d_nhwc_forward_dt: a 3x3 layer, and the transposed convolution as its 1x1 panel of
    1024 channels, with the bias and ReLU the object gives them), beside its FLOPs and the TFLOP/s that makes;
  - rn_mask_predict_forward beside the bytes it must read once (the [K, 14, 14, 1024] tensor) and the GB/s that makes;
  - rn_paste_masks_forward for `masks` alone, for `bits` alone and for both, beside rn_memset of the same output bytes:
    boxes of 32 .. 400 pixels, so most of a plane is zero fill;
  - rn_mask_head_forward through the object, probabilities only and with the pasted bits;
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
from resnet_c_amd import mask as MK
from resnet_c_amd import ops
from resnet_c_amd.tensor import _DeviceBuffer

IMAGE, A, M, CR, LAYERS = (800, 1344), 256, 14, 256, (256,) * 4


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
    """[K, 4]: boxes of 32 .. 400 pixels inside the image"""
    cx, cy, w, h = g.uniform(0, IMAGE[1], K), g.uniform(0, IMAGE[0], K), g.uniform(32, 400, K), g.uniform(32, 400, K)
    box = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=1)
    return np.clip(box, 0, [IMAGE[1], IMAGE[0], IMAGE[1], IMAGE[0]]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 4])
    ap.add_argument("--detections", type=int, default=100)
    ap.add_argument("--classes", type=int, default=91)
    a = ap.parse_args()
    lib, ctx = L.lib(), R.get_ctx()
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    lib.rn_event_create(ctx.handle, ctypes.byref(e0)), lib.rn_event_create(ctx.handle, ctypes.byref(e1))
    ev = (e0, e1)
    C, Dn, H, W = a.classes, a.detections, IMAGE[0], IMAGE[1]
    g = np.random.default_rng(0)
    state = MK.generate_mask_head_state(A, LAYERS, CR, C, seed=0)
    mh = MK.MaskHead(A, LAYERS, CR, C, state, resolution=M)
    packed = {}
    for name, cin, cout, k in (("conv3x3", A, A, 3), ("deconv_panel", A, 4 * CR, 1)):
        raw = ops._up_raw((g.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32))
        n = int(lib.rn_conv2d_packed_weight_numel_dt(L.RN_DTYPE_F32, cin, cout, k))
        pk = _DeviceBuffer(ctx, n * 4)
        L.check(lib.rn_conv2d_pack_weight_dt(ctx.handle, L.RN_DTYPE_F32, raw.ptr, pk.ptr, cin, cout, k), "pack", ctx.handle)
        packed[name] = (pk, ops._up_raw(np.zeros(cout, np.float32)), cin, cout, k)
    wl = ops._up_raw(state[MK.PREDICTOR_KEYS[2]].reshape(C, CR))
    bl = ops._up_raw(state[MK.PREDICTOR_KEYS[3]])
    ctx.sync()
    saved_layout = lib.rn_ctx_get_layout(ctx.handle)
    ctx.set_layout(L.RN_LAYOUT_NHWC)
    sizes = [(200, 336), (100, 168), (50, 84), (25, 42)]
    for B in a.batches:
        K = B * Dn
        rec = {"B": B, "D": Dn, "C": C, "M": M, "a": A, "dim_reduced": CR, "layers": len(LAYERS)}
        boxes = detections(g, K)
        labels = g.integers(1, C, K).astype(np.int32)
        dboxes, dlabels = ops._up_raw(boxes), ops._up_raw(labels)
        pooled = ops._up_raw(np.maximum(g.standard_normal((K, M, M, A), dtype=np.float32), 0))
        mid = _DeviceBuffer(ctx, K * M * M * A * 4)
        t_dev = _DeviceBuffer(ctx, K * M * M * 4 * CR * 4)
        for name, (pk, bias, cin, cout, k) in packed.items():
            dst = mid if cout == A else t_dev
            ep = L.Epilogue(None, bias.ptr, None, 1)

            def run(dst=dst, pk=pk, cin=cin, cout=cout, k=k, ep=ep):
                L.check(lib.rn_conv2d_nhwc_forward_dt(ctx.handle, L.RN_DTYPE_F32, L.RN_DTYPE_F32, pooled.ptr, dst.ptr, pk.ptr, k, 1,
                                                      k // 2, M, M, K, cin, cout, M, M, ctypes.byref(ep)), name, ctx.handle)

            t, s = timed(lib, ctx, ev, run, a.rounds, a.reps)
            flops = 2.0 * K * M * M * cin * k * k * cout
            rec.update({f"{name}_ms": round(t, 4), f"{name}_spread_ms": round(s, 4), f"{name}_gflop": round(flops / 1e9, 2),
                        f"{name}_tflop_per_s": round(flops / t / 1e9, 1)})
        probs = _DeviceBuffer(ctx, K * 4 * M * M * 4)

        def predict():
            L.check(lib.rn_mask_predict_forward(ctx.handle, t_dev.ptr, dlabels.ptr, wl.ptr, bl.ptr, K, M, CR, C, probs.ptr), "predict",
                    ctx.handle)

        t, s = timed(lib, ctx, ev, predict, a.rounds, a.reps)
        read = K * M * M * 4 * CR * 4
        rec.update({"predict_ms": round(t, 4), "predict_spread_ms": round(s, 4), "predict_mb_read_once": round(read / 1e6, 2),
                    "predict_gb_per_s": round(read / t / 1e6, 1)})
        masks, bits = _DeviceBuffer(ctx, K * H * W * 4), _DeviceBuffer(ctx, K * H * W)
        for name, m, b, nbytes in (("paste_masks", masks, None, K * H * W * 4), ("paste_bits", None, bits, K * H * W),
                                   ("paste_both", masks, bits, K * H * W * 5)):
            def paste(m=m, b=b):
                L.check(lib.rn_paste_masks_forward(ctx.handle, probs.ptr, dboxes.ptr, dlabels.ptr, K, 2 * M, H, W, 0.5, m.ptr if m else None,
                                                   b.ptr if b else None), name, ctx.handle)

            def fill(m=m, b=b):
                if m:
                    L.check(lib.rn_memset(ctx.handle, m.ptr, 0, K * H * W * 4), "memset", ctx.handle)
                if b:
                    L.check(lib.rn_memset(ctx.handle, b.ptr, 0, K * H * W), "memset", ctx.handle)

            t, s = timed(lib, ctx, ev, paste, a.rounds, a.reps)
            tm, _ = timed(lib, ctx, ev, fill, a.rounds, a.reps)
            rec.update({f"{name}_ms": round(t, 4), f"{name}_spread_ms": round(s, 4), f"{name}_mb_written": round(nbytes / 1e6, 1),
                        f"{name}_gb_per_s": round(nbytes / t / 1e6, 1), f"{name}_memset_ms": round(tm, 4),
                        f"{name}_memset_gb_per_s": round(nbytes / tm / 1e6, 1)})
        del masks
        for name, want in (("head_probs", ("probs",)), ("head_probs_bits", ("probs", "bits"))):
            spec, bufs = mh.buffers(1, K, IMAGE, want)
            req = mh.request(bufs)

            def whole(req=req):
                L.check(lib.rn_mask_head_forward(mh.handle, pooled.ptr, dlabels.ptr, dboxes.ptr, K, H, W, ctypes.byref(req)),
                        "rn_mask_head_forward", ctx.handle)

            t, s = timed(lib, ctx, ev, whole, a.rounds, a.reps)
            rec.update({f"{name}_ms": round(t, 4), f"{name}_spread_ms": round(s, 4)})
            del bufs
        # the front of the stage: the RoI former and the NHWC pooler on a seeded pyramid
        maps = [ops._up_raw(g.standard_normal((B, h, w, A), dtype=np.float32)) for h, w in sizes]
        scales = np.array([0.25, 0.125, 0.0625, 0.03125], np.float32)
        thr = np.concatenate([ops.roi_level_thresholds(scales), np.zeros(1, np.float32)])
        rois = _DeviceBuffer(ctx, K * 20)
        fp = ctypes.POINTER(ctypes.c_float)
        lab2 = ops._up_raw(labels.reshape(B, Dn))

        def former():
            L.check(lib.rn_detection_rois_forward(ctx.handle, dboxes.ptr, lab2.ptr, B, Dn, rois.ptr), "rois", ctx.handle)

        def pool():
            L.check(lib.rn_roi_align_nhwc_forward_dt(
                ctx.handle, L.RN_DTYPE_F32, 4, (ctypes.c_void_p * 4)(*[d.ptr for d in maps]), (ctypes.c_uint64 * 4)(*[h for h, _ in sizes]),
                (ctypes.c_uint64 * 4)(*[w for _, w in sizes]), scales.ctypes.data_as(fp), thr.ctypes.data_as(fp), B, A, rois.ptr, K, M, M,
                2, 0, mid.ptr, None), "pool", ctx.handle)

        t, s = timed(lib, ctx, ev, former, a.rounds, a.reps)
        rec.update({"detection_rois_ms": round(t, 4)})
        t, s = timed(lib, ctx, ev, pool, a.rounds, a.reps)
        out_b = K * M * M * A * 4
        rec.update({"roi_align_nhwc_ms": round(t, 4), "roi_align_nhwc_spread_ms": round(s, 4), "roi_align_nhwc_output_gb_per_s": round(out_b / t / 1e6, 1)})
        print(json.dumps(rec), flush=True)
        del maps, pooled, mid, t_dev, bits, probs
    ctx.set_layout(saved_layout)
    mh.close()


if __name__ == "__main__":
    main()
