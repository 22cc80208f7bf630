#!/usr/bin/env python3
"""What the pooler costs: rn_roi_align_forward_dt alone on a detection-sized pyramid, beside the library's own
HBM-bound NCHW writer.

    python tools/roi_rate.py [--rounds 5] [--reps 5] [--rois 1000] [--dtype f32 bf16] [--sizes 7 14]

The pyramid of an 800 x 1344 input at strides 4, 8, 16, 32 (200 x 336 .. 25 x 42), C = 256, B = 2; `--rois` RoIs per
image whose sides are log-uniform in 16 .. 800 pixels with aspect ratios in 1/2 .. 2, clipped to the image (the
spread of a detector's proposals: most of them small, every level used); output 7 x 7 and 14 x 14, sampling ratio 2.
Per launch: ms (the best of `rounds` windows of `reps` launches between two events) and GB/s of the OUTPUT bytes, the
traffic that has to reach HBM, beside the bytes of the distinct pixels each RoI reads (counted on the host, once
per RoI: the RoIs of a batch share little and the maps do not fit the L2) and GB/s of both together.  In the same
run, rn_nhwc_to_nchw_dt on [K,PH,PW,C] fp32 -> [K,C,PH,PW]: the same number of output bytes in the same layout,
written by the library's streaming exporter from one streamed read.  Every launch of a window writes the next of
`sets` output buffers (rotated until a round touches 600 MB, at most 8)."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd import ops
from resnet_c_amd.tensor import _DeviceBuffer

IMAGE, STRIDES, C, B = (800, 1344), (4, 8, 16, 32), 256, 2
FP = ctypes.POINTER(ctypes.c_float)


def elapsed(lib, ctx, events, body):
    e0, e1 = events
    lib.rn_event_record(ctx.handle, e0)
    body()
    lib.rn_event_record(ctx.handle, e1)
    ms = ctypes.c_float()
    L.check(lib.rn_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "elapsed", ctx.handle)
    return ms.value


def proposals(per_image, seed=0):
    rng = np.random.default_rng(seed)
    n = per_image * B
    side, ratio = np.exp(rng.uniform(np.log(16), np.log(800), n)), np.exp(rng.uniform(np.log(0.5), np.log(2), n))
    bw, bh = side * np.sqrt(ratio), side / np.sqrt(ratio)
    cx, cy = rng.uniform(0, IMAGE[1], n), rng.uniform(0, IMAGE[0], n)
    x1, x2 = np.clip(cx - bw / 2, 0, IMAGE[1]), np.clip(cx + bw / 2, 0, IMAGE[1])
    y1, y2 = np.clip(cy - bh / 2, 0, IMAGE[0]), np.clip(cy + bh / 2, 0, IMAGE[0])
    return np.stack([np.arange(n) % B, x1, y1, x2, y2], axis=1).astype(np.float32)


def distinct_pixels(rois, levels, scales, hs, ws, side, S=2):
    """the pixels every RoI reads, counted once per RoI (rows x columns of its sample grid's corners), summed: what
    the launch has to fetch when the RoIs of a batch share nothing"""
    total = 0
    for r, lv in zip(rois.astype(np.float64), levels):
        sc, h, w = float(scales[lv]), hs[lv], ws[lv]
        x1, y1, x2, y2 = (v * sc for v in r[1:])
        rw, rh = max(x2 - x1, 1.0), max(y2 - y1, 1.0)
        n = side * S

        def touched(c0, extent, size):
            c = np.clip(c0 + (np.arange(n) + 0.5) * extent / n, 0, None)
            lo = np.minimum(c.astype(np.int64), size - 1)
            return len(np.unique(np.concatenate([lo, np.minimum(lo + 1, size - 1)])))
        total += touched(y1, rh, h) * touched(x1, rw, w)
    return total


def timed(lib, ctx, events, run, sets, rounds, reps):
    for _ in range(sets):
        run()
    ctx.sync()
    t = [elapsed(lib, ctx, events, lambda: [run() for _ in range(reps)]) / reps for _ in range(rounds)]
    return min(t), max(t) - min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rois", type=int, default=1000)
    ap.add_argument("--dtype", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--sizes", nargs="+", type=int, default=[7, 14])
    a = ap.parse_args()
    lib, ctx = L.lib(), R.get_ctx()
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    lib.rn_event_create(ctx.handle, ctypes.byref(e0)), lib.rn_event_create(ctx.handle, ctypes.byref(e1))
    hs, ws = [IMAGE[0] // s for s in STRIDES], [IMAGE[1] // s for s in STRIDES]
    scales = np.array([1.0 / s for s in STRIDES], np.float32)
    thr = np.concatenate([ops.roi_level_thresholds(scales), np.zeros(1, np.float32)])
    rois = proposals(a.rois)
    K = len(rois)
    levels = ops.roi_levels_ref(rois, thr[:3])
    drois = ops._up_raw(rois)
    rng = np.random.default_rng(1)
    for dtype in a.dtype:
        dt, np_dt = (L.RN_DTYPE_BF16, np.uint16) if dtype == "bf16" else (L.RN_DTYPE_F32, np.float32)
        maps = []
        for h, w in zip(hs, ws):
            v = rng.random((B, h, w, C), dtype=np.float32)
            maps.append(ops._up_raw(v if dtype == "f32" else ops.to_bf16_bits(v)))
        mp = (ctypes.c_void_p * 4)(*[m.ptr for m in maps])
        hp, wp = (ctypes.c_uint64 * 4)(*hs), (ctypes.c_uint64 * 4)(*ws)
        for side in a.sizes:
            out_bytes = K * C * side * side * 4
            src_bytes = distinct_pixels(rois, levels, scales, hs, ws, side) * C * (2 if dtype == "bf16" else 4)
            sets = min(8, max(2, -(-600_000_000 // out_bytes)))
            outs = [_DeviceBuffer(ctx, out_bytes) for _ in range(sets)]
            src = _DeviceBuffer(ctx, out_bytes)          # the exporter's source: as many bytes, streamed once
            L.check(lib.rn_memset(ctx.handle, src.ptr, 0, out_bytes), "memset", ctx.handle)
            at = [0]

            def run_roi():
                i = at[0] = (at[0] + 1) % sets
                L.check(lib.rn_roi_align_forward_dt(ctx.handle, dt, 4, mp, hp, wp, scales.ctypes.data_as(FP), thr.ctypes.data_as(FP),
                                                    B, C, drois.ptr, K, side, side, 2, 0, outs[i].ptr, None),
                        "rn_roi_align_forward_dt", ctx.handle)

            def run_export():
                i = at[0] = (at[0] + 1) % sets
                L.check(lib.rn_nhwc_to_nchw_dt(ctx.handle, L.RN_DTYPE_F32, src.ptr, outs[i].ptr, K, C, side, side),
                        "rn_nhwc_to_nchw_dt", ctx.handle)

            t_roi, s_roi = timed(lib, ctx, (e0, e1), run_roi, sets, a.rounds, a.reps)
            t_exp, s_exp = timed(lib, ctx, (e0, e1), run_export, sets, a.rounds, a.reps)
            t_roi2, _ = timed(lib, ctx, (e0, e1), run_roi, sets, a.rounds, a.reps)        # and the pooler once more, behind it
            t_roi = min(t_roi, t_roi2)
            print(json.dumps({"launch": "rn_roi_align_forward_dt", "maps": dtype, "B": B, "C": C, "levels": list(zip(hs, ws)),
                              "rois": K, "rois_per_level": np.bincount(levels, minlength=4).tolist(), "output": [side, side],
                              "sampling_ratio": 2, "output_mb": round(out_bytes / 1e6, 1), "buffer_sets_rotated": sets,
                              "ms": round(t_roi, 4), "spread_ms": round(s_roi, 4),
                              "output_gb_per_s": round(out_bytes / t_roi / 1e6, 1),
                              "distinct_source_mb": round(src_bytes / 1e6, 1),
                              "source_plus_output_gb_per_s": round((src_bytes + out_bytes) / t_roi / 1e6, 1),
                              "exporter_ms": round(t_exp, 4), "exporter_spread_ms": round(s_exp, 4),
                              "exporter_output_gb_per_s": round(out_bytes / t_exp / 1e6, 1),
                              "share_of_exporter_rate": round(t_exp / t_roi, 3)}), flush=True)
            del outs, src
        del maps


if __name__ == "__main__":
    main()
