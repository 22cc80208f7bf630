#!/usr/bin/env python3
"""Images/s of NativeModel at several input sizes (rn_model_set_input_size), the stem route each size takes,
and the global average pool alone on a 16 x 16 x 2048 map against the generic pooling kernel.

    python tools/size_rate.py [--arch resnet50] [--dtype f32 bf16] [--batch 256] [--seconds 1.0]

Per size and dtype: one model, resized; back-to-back fused forwards of one batch timed with HIP events on the
model's stream over a window of at least --seconds (untuned tiles: the per-launch choice).  The stem route is
read off a profiled forward: "fused" = one conv + bn + relu + max-pool launch, "unfused" = stem and max-pool as
separate launches (conv output width off a multiple of 8 or above 128).
The pool: B = 256 maps of 16 x 16 x 2048 (what a 512 x 512 image ends in), rn_global_avgpool_nhwc_forward_dt
against rn_avgpool2d_nhwc_forward_dt(k = 16) -- the launch the head took for such a map before -- and against
the byte floor: the input read once at the HBM rate tools/layer_report.py uses."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd.tensor import _DeviceBuffer

SIZES = [(128, 128), (160, 160), (224, 224), (288, 288), (320, 320), (224, 320)]
HBM_BYTES_PER_S = 6.3e12  # the achievable rate tools/layer_report.py uses (6.3e9 bytes per ms)


def events(ctx):
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    for e in (e0, e1):
        L.check(L.lib().rn_event_create(ctx.handle, ctypes.byref(e)), "event", ctx.handle)
    return e0, e1


def timed(ctx, launch, seconds):
    """ms per call of launch() over a window of at least `seconds`, after five warm-up calls"""
    lib = L.lib()
    for _ in range(5):
        launch()
    ctx.sync()
    t0 = time.perf_counter()
    launch()
    ctx.sync()
    steps = max(10, int(seconds / max(time.perf_counter() - t0, 1e-5)) + 1)
    e0, e1 = events(ctx)
    L.check(lib.rn_event_record(ctx.handle, e0), "record", ctx.handle)
    for _ in range(steps):
        launch()
    L.check(lib.rn_event_record(ctx.handle, e1), "record", ctx.handle)
    ctx.sync()
    ms = ctypes.c_float()
    L.check(lib.rn_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "elapsed", ctx.handle)
    lib.rn_event_destroy(e0)
    lib.rn_event_destroy(e1)
    return ms.value / steps, steps


def stem_route(m, x, B):
    out = R.FloatTensor((B, 1000), R.Device.GPU)
    m.set_profiling(True)
    try:
        m.forward_ptr(x.data(), B, out.data(), True)
        ops = [r["op"] for r in m.profile()]
    finally:
        m.set_profiling(False)
    return "fused" if "conv2d+epilogue+maxpool" in ops else "unfused"


def model_rates(arch, dtype, B, seconds):
    m = R.NativeModel(arch, state=R.weights.generate_state(arch, 0), dtype=dtype)
    try:
        for size in SIZES:
            m.set_input_size(*size)
            n = min(B, 4 * m.max_sub_batch())
            x = R.FloatTensor.from_numpy(R.weights.generate_input(n, 0, hw=size), R.Device.GPU)
            out = R.FloatTensor((n, 1000), R.Device.GPU)
            route = stem_route(m, x, n)
            ms, steps = timed(m.ctx, lambda: m.forward_ptr(x.data(), n, out.data(), True), seconds)
            gflop = R.weights.forward_flops(arch, hw=size) / 1e9
            ips = n / ms * 1e3
            print(json.dumps({"arch": arch, "dtype": dtype, "size": list(size), "batch": n, "stem_route": route,
                              "max_sub_batch": m.max_sub_batch(), "steps": steps, "ms_per_batch": round(ms, 3),
                              "images_per_s": round(ips, 1), "gflop_per_image": round(gflop, 3),
                              "tflops": round(ips * gflop / 1e3, 1),
                              "activation_mb_per_image": round(m.activation_bytes() / n / 1e6, 2)}), flush=True)
    finally:
        m.close()


def pool_alone(dtype, seconds, B=256, C=2048, H=16, W=16):
    ctx, lib = R.get_ctx(), L.lib()
    es = 2 if dtype == "bf16" else 4
    dt = L.RN_DTYPE_BF16 if dtype == "bf16" else L.RN_DTYPE_F32
    inp = _DeviceBuffer(ctx, B * H * W * C * es)
    L.check(lib.rn_memset(ctx.handle, inp.ptr, 0, B * H * W * C * es), "memset", ctx.handle)
    out = _DeviceBuffer(ctx, B * C * es)

    def new():
        L.check(lib.rn_global_avgpool_nhwc_forward_dt(ctx.handle, dt, inp.ptr, out.ptr, B, C, H, W), "global", ctx.handle)

    def generic():
        L.check(lib.rn_avgpool2d_nhwc_forward_dt(ctx.handle, dt, inp.ptr, out.ptr, H, 1, 0, 1, 1, B, C, H, W), "generic",
                ctx.handle)
    ms_new, _ = timed(ctx, new, seconds)
    ms_old, _ = timed(ctx, generic, seconds)
    floor_ms = B * H * W * C * es / HBM_BYTES_PER_S * 1e3
    print(json.dumps({"op": "global_avgpool", "dtype": dtype, "map": [B, H, W, C], "input_mb": round(B * H * W * C * es / 1e6, 1),
                      "global_avgpool_ms": round(ms_new, 4), "generic_avgpool2d_ms": round(ms_old, 4),
                      "byte_floor_ms": round(floor_ms, 4), "speedup": round(ms_old / ms_new, 2),
                      "share_of_floor": round(floor_ms / ms_new, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--dtype", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=1.0)
    a = ap.parse_args()
    for dt in a.dtype:
        pool_alone(dt, min(a.seconds, 0.5))
    for dt in a.dtype:
        model_rates(a.arch, dt, a.batch, a.seconds)


if __name__ == "__main__":
    main()
