#!/usr/bin/env python3
"""What dilation costs: the model's dilated 3x3 layers next to the undilated convolution of the same tensor
shapes, and ResNet-50 under replace_stride_with_dilation next to the undilated network.

    python tools/dilation_rate.py [--batch 64] [--model-batch 64] [--seconds 0.5] [--rounds 5] [--reps 20]

Per layer (rn_conv2d_dilated_nhwc_forward_dt with an epilogue, as the driver launches it): 28 x 28 maps with
C = 256 and 512, d = 2 and 4, at B = --batch, in fp32, bf16 and the ResNeXt grouped form (32 groups, fp32: the
super-group kernel; bf16: the dense panel).  Each next to d = 1, p = 1 on the same tensors: FLOPs, panels and
tiles are identical, so the ratio is the price of the wider tap footprint.  Both are warmed up and timed
alternately (device events, `reps` launches per window, the best of `rounds` windows).  Roofs as
tools/layer_report.py: 157.3 TFLOP/s fp32, 2500 TFLOP/s bf16, 6.3 TB/s.

Per model: images/s and TFLOP/s of ResNet-50 with (0,0,0), (0,0,1) and (0,1,1) in fp32 and bf16 at
--model-batch (forward_flops of the dilated network), with max_sub_batch and the arenas per image."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd.tensor import _DeviceBuffer

MFMA_FLOP_PER_MS = {"f32": 157.3e9, "bf16": 2500e9}
HBM_BYTES_PER_MS = 6.3e9


def layer(lib, ctx, dtype, B, C, G, d, rounds, reps, events):
    H = 28
    dt = L.RN_DTYPE_BF16 if dtype == "bf16" else L.RN_DTYPE_F32
    es = 2 if dtype == "bf16" else 4
    rng = np.random.default_rng(C + d)
    xh = rng.standard_normal(B * H * H * C, dtype=np.float32)
    xs = R.ops.to_bf16_bits(xh) if es == 2 else xh
    x = _DeviceBuffer(ctx, xs.nbytes)
    L.check(lib.rn_memcpy_h2d(ctx.handle, x.ptr, xs.ctypes.data, xs.nbytes), "h2d", ctx.handle)
    w = rng.standard_normal((C, C // G, 3, 3), dtype=np.float32) / np.float32(np.sqrt(9 * C // G))
    dw = R.FloatTensor.from_numpy(w, R.Device.GPU)
    if G == 1:
        packed = _DeviceBuffer(ctx, int(lib.rn_conv2d_packed_weight_numel_dt(dt, C, C, 3)) * es)
        L.check(lib.rn_conv2d_pack_weight_dt(ctx.handle, dt, dw.data(), packed.ptr, C, C, 3), "pack", ctx.handle)
    else:
        packed = _DeviceBuffer(ctx, int(lib.rn_conv2d_grouped_packed_weight_numel_dt(dt, C, C, 3, G)) * es)
        L.check(lib.rn_conv2d_grouped_pack_weight_dt(ctx.handle, dt, dw.data(), packed.ptr, C, C, 3, G), "pack", ctx.handle)
    out = _DeviceBuffer(ctx, B * H * H * C * es)
    sc = R.FloatTensor.from_numpy(np.ones(C, np.float32), R.Device.GPU)
    sh = R.FloatTensor.from_numpy(np.zeros(C, np.float32), R.Device.GPU)
    ep = L.Epilogue(sc.data(), sh.data(), None, 1)

    def conv(dil):
        L.check(lib.rn_conv2d_dilated_nhwc_forward_dt(ctx.handle, dt, dt, x.ptr, out.ptr, packed.ptr, 3, 1, dil, dil, H, H, B,
                                                      C, C, H, H, G, ctypes.byref(ep)), "conv", ctx.handle)

    def window(dil):
        e0, e1 = events
        lib.rn_event_record(ctx.handle, e0)
        for _ in range(reps):
            conv(dil)
        lib.rn_event_record(ctx.handle, e1)
        ms = ctypes.c_float()
        L.check(lib.rn_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "elapsed", ctx.handle)
        return ms.value / reps

    for _ in range(5):
        conv(d), conv(1)
    ctx.sync()
    td, t1 = [], []
    for _ in range(rounds):
        td.append(window(d)), t1.append(window(1))
    a, b = min(td), min(t1)
    flops = 2.0 * B * H * H * C * (C // G) * 9
    nbytes = es * (2 * B * H * H * C + C * (C // G) * 9)
    ideal = max(flops / MFMA_FLOP_PER_MS[dtype], nbytes / HBM_BYTES_PER_MS)
    print(json.dumps({"layer": f"{H}x{H}x{C}" + (f" G={G}" if G > 1 else ""), "dtype": dtype, "B": B, "d": d,
                      "dilated_ms": round(a, 4), "undilated_ms": round(b, 4), "ratio": round(a / b, 3),
                      "dilated_tflops": round(flops / a / 1e9, 1), "undilated_tflops": round(flops / b / 1e9, 1),
                      "roofline_ideal_ms": round(ideal, 4), "dilated_share_of_roof": round(ideal / a, 3),
                      "spread_ms": [round(max(td) - a, 4), round(max(t1) - b, 4)]}), flush=True)


def model(arch, dtype, B, seconds):
    m = R.NativeModel(arch, state=R.weights.generate_state(arch, 0), dtype=dtype)
    lib = L.lib()
    try:
        for flags in ((0, 0, 0), (0, 0, 1), (0, 1, 1)):
            m.set_dilation(*flags)
            n = min(B, m.max_sub_batch())
            x = R.FloatTensor.from_numpy(R.weights.generate_input(n, 0), R.Device.GPU)
            out = R.FloatTensor((n, 1000), R.Device.GPU)
            run = lambda: m.forward_ptr(x.data(), n, out.data(), True)
            for _ in range(3):
                run()
            m.ctx.sync()
            t0 = time.perf_counter()
            run()
            m.ctx.sync()
            steps = max(5, int(seconds / max(time.perf_counter() - t0, 1e-5)) + 1)
            e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
            lib.rn_event_create(m.ctx.handle, ctypes.byref(e0)), lib.rn_event_create(m.ctx.handle, ctypes.byref(e1))
            lib.rn_event_record(m.ctx.handle, e0)
            for _ in range(steps):
                run()
            lib.rn_event_record(m.ctx.handle, e1)
            m.ctx.sync()
            ms = ctypes.c_float()
            L.check(lib.rn_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "elapsed", m.ctx.handle)
            lib.rn_event_destroy(e0), lib.rn_event_destroy(e1)
            ms = ms.value / steps
            gflop = R.weights.forward_flops(arch, 224, replace_stride_with_dilation=flags) / 1e9
            ips = n / ms * 1e3
            print(json.dumps({"arch": arch, "dtype": dtype, "replace_stride_with_dilation": list(flags),
                              "output_stride": m.output_stride, "batch": n, "max_sub_batch": m.max_sub_batch(),
                              "steps": steps, "ms_per_batch": round(ms, 3), "images_per_s": round(ips, 1),
                              "gflop_per_image": round(gflop, 3), "tflops": round(ips * gflop / 1e3, 1),
                              "activation_mb_per_image": round(m.activation_bytes() / n / 1e6, 2)}), flush=True)
    finally:
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--model-batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    lib, ctx = L.lib(), R.get_ctx()
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    lib.rn_event_create(ctx.handle, ctypes.byref(e0)), lib.rn_event_create(ctx.handle, ctypes.byref(e1))
    for dtype in ("f32", "bf16"):
        for G in (1, 32):
            for C, d in ((256, 2), (512, 2), (512, 4)):
                layer(lib, ctx, dtype, a.batch, C, G, d, a.rounds, a.reps, (e0, e1))
    if not a.skip_model:
        for dtype in ("f32", "bf16"):
            model("resnet50", dtype, a.model_batch, a.seconds)


if __name__ == "__main__":
    main()
