#!/usr/bin/env python3
"""Images/s and achieved TFLOP/s of NativeModel for any architecture the driver takes (bench.py times
ResNet-50/101/152 only): tuned tiles, warm-up, then back-to-back forwards of one batch timed with HIP events
on the model's stream over a window of at least --seconds.

    python tools/arch_rate.py [--arch resnet18 resnet34 ...] [--dtype f32 bf16] [--batch 256] [--seconds 1.5]

FLOPs per image: weights.forward_flops (2 x MACs of the convolutions and fc, as bench.py counts ResNet-50's
8.178368512 GFLOP): ResNet-18 3.628146688, ResNet-34 7.327522816."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import resnet_c_amd as R
from resnet_c_amd import _lib as L


def rate(arch, dtype, B, seconds, warmup):
    lib = L.lib()
    m = R.NativeModel(arch, state=R.weights.generate_state(arch, 0), dtype=dtype)
    try:
        x = R.FloatTensor.from_numpy(R.weights.generate_input(B, 0), R.Device.GPU)
        out = R.FloatTensor((B, 1000), R.Device.GPU)
        m.tune(x.data(), B, out.data(), True)
        for _ in range(warmup):
            m.forward_ptr(x.data(), B, out.data(), True)
        m.ctx.sync()
        e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
        L.check(lib.rn_event_create(m.ctx.handle, ctypes.byref(e0)), "event", m.ctx.handle)
        L.check(lib.rn_event_create(m.ctx.handle, ctypes.byref(e1)), "event", m.ctx.handle)
        # size the window: one timed forward, then enough of them for `seconds`
        t0 = time.perf_counter()
        m.forward_ptr(x.data(), B, out.data(), True)
        m.ctx.sync()
        steps = max(10, int(seconds / max(time.perf_counter() - t0, 1e-4)) + 1)
        L.check(lib.rn_event_record(m.ctx.handle, e0), "record", m.ctx.handle)
        for _ in range(steps):
            m.forward_ptr(x.data(), B, out.data(), True)
        L.check(lib.rn_event_record(m.ctx.handle, e1), "record", m.ctx.handle)
        m.ctx.sync()
        ms = ctypes.c_float()
        L.check(lib.rn_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "elapsed", m.ctx.handle)
        lib.rn_event_destroy(e0)
        lib.rn_event_destroy(e1)
        sec = ms.value / 1e3
        gflop = R.weights.forward_flops(arch) / 1e9
        ips = B * steps / sec
        return {"arch": arch, "dtype": dtype, "batch": B, "steps": steps, "window_s": round(sec, 3),
                "images_per_s": round(ips, 1), "ms_per_batch": round(ms.value / steps, 3),
                "gflop_per_image": gflop, "tflops": round(ips * gflop / 1e3, 1), "streams": m.parts(B)}
    finally:
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", nargs="+", default=["resnet18", "resnet34"])
    ap.add_argument("--dtype", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for arch in a.arch:
        for dt in a.dtype:
            print(json.dumps(rate(arch, dt, a.batch, a.seconds, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
