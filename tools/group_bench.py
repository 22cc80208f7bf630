#!/usr/bin/env python3
"""The grouped 3x3 kernel (rn_conv_group.hip) against the dense contraction on the zero-filled dense weight,
for every conv2 shape of a ResNeXt: the comparison that justifies the kernel.

    python tools/group_bench.py [--arch resnext50_32x4d] [--batch 256] [--dtype f32] [--rounds 5] [--reps 50]

Both versions are warmed up and timed alternately (device events, `reps` launches per window, the best of
`rounds` windows).  Per shape: ms, algorithmic TFLOP/s (dense / groups), padded TFLOP/s (x 32/Cg, the products
the super-group kernel issues), GB/s of the algorithmic bytes, and the dense fallback's ms.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd.tensor import _DeviceBuffer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="resnext50_32x4d")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    lib, ctx = L.lib(), R.get_ctx()
    groups = R.weights.family_of(a.arch)[1]
    dt = L.RN_DTYPE_BF16 if a.dtype == "bf16" else L.RN_DTYPE_F32
    es = 2 if a.dtype == "bf16" else 4
    shapes, hw = [], 56
    for pre, _cin, mid, _cout, stride, _ds in R.weights.iter_blocks(a.arch):
        if (hw, mid, stride) not in [s[1:] for s in shapes]:
            shapes.append((pre, hw, mid, stride))
        hw //= stride
    rng = np.random.default_rng(0)
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    lib.rn_event_create(ctx.handle, ctypes.byref(e0)); lib.rn_event_create(ctx.handle, ctypes.byref(e1))
    for pre, H, C, s in shapes:
        B, cg = a.batch, C // groups
        ho = int(lib.rn_conv_output_size(H, 3, s, 1))
        xh = rng.standard_normal(B * H * H * C, dtype=np.float32)
        x = _DeviceBuffer(ctx, xh.size * es)
        xs = R.ops.to_bf16_bits(xh) if es == 2 else xh
        L.check(lib.rn_memcpy_h2d(ctx.handle, x.ptr, xs.ctypes.data, xs.nbytes), "h2d", ctx.handle)
        w = (rng.standard_normal((C, cg, 3, 3), dtype=np.float32) / np.float32(np.sqrt(9 * cg)))
        dense = np.zeros((C, C, 3, 3), np.float32)
        for o in range(C):
            dense[o, o // cg * cg:(o // cg + 1) * cg] = w[o]
        dw, dd = R.FloatTensor.from_numpy(w, R.Device.GPU), R.FloatTensor.from_numpy(dense, R.Device.GPU)
        pg = _DeviceBuffer(ctx, int(lib.rn_conv2d_grouped_packed_weight_numel_dt(dt, C, C, 3, groups)) * es)
        pd = _DeviceBuffer(ctx, int(lib.rn_conv2d_packed_weight_numel_dt(dt, C, C, 3)) * es)
        L.check(lib.rn_conv2d_grouped_pack_weight_dt(ctx.handle, dt, dw.data(), pg.ptr, C, C, 3, groups), "pack", ctx.handle)
        L.check(lib.rn_conv2d_pack_weight_dt(ctx.handle, dt, dd.data(), pd.ptr, C, C, 3), "pack", ctx.handle)
        out = _DeviceBuffer(ctx, B * ho * ho * C * es)
        sc = R.FloatTensor.from_numpy(np.ones(C, np.float32), R.Device.GPU)
        sh = R.FloatTensor.from_numpy(np.zeros(C, np.float32), R.Device.GPU)
        ep = L.Epilogue(sc.data(), sh.data(), None, 1)

        def grouped():
            L.check(lib.rn_conv2d_grouped_nhwc_forward_dt(ctx.handle, dt, dt, x.ptr, out.ptr, pg.ptr, 3, s, 1, ho, ho, B, C,
                                                          C, H, H, groups, ctypes.byref(ep)), "grouped", ctx.handle)

        def fallback():
            L.check(lib.rn_conv2d_nhwc_forward_dt(ctx.handle, dt, dt, x.ptr, out.ptr, pd.ptr, 3, s, 1, ho, ho, B, C, C, H, H,
                                                  ctypes.byref(ep)), "dense", ctx.handle)

        def window(fn):
            lib.rn_event_record(ctx.handle, e0)
            for _ in range(a.reps):
                fn()
            lib.rn_event_record(ctx.handle, e1)
            ms = ctypes.c_float()
            lib.rn_event_elapsed_ms(e0, e1, ctypes.byref(ms))
            return ms.value / a.reps

        for _ in range(10):
            grouped(); fallback()
        ctx.sync()
        tg, td = [], []
        for _ in range(a.rounds):
            tg.append(window(grouped)); td.append(window(fallback))
        g, d = min(tg), min(td)
        flops = 2.0 * B * ho * ho * C * cg * 9
        nbytes = es * (B * H * H * C + C * cg * 9 + B * ho * ho * C)
        print(json.dumps({"layer": pre + ".conv2", "dtype": a.dtype, "B": B, "H": H, "C": C, "Cg": cg, "stride": s,
                          "grouped_ms": round(g, 4), "dense_fallback_ms": round(d, 4), "speedup": round(d / g, 2),
                          "alg_tflops": round(flops / g / 1e9, 2),
                          "padded_tflops": round(flops * max(1, 32 // cg) / g / 1e9, 2) if es == 4 else None,
                          "alg_gbs": round(nbytes / g / 1e6, 1),
                          "spread_ms": [round(max(tg) - g, 4), round(max(td) - d, 4)]}), flush=True)


if __name__ == "__main__":
    main()
