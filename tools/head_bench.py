#!/usr/bin/env python3
"""rn_softmax_topk_forward alone: milliseconds per launch by HIP events and the fraction of its byte floor.

The floor is the logits read once plus the outputs written (probabilities when asked for, k probabilities
and k 64-bit indices per row) at the HBM rate tools/layer_report.py uses (6.3e9 bytes per ms).

    python tools/head_bench.py [--batch 256] [--classes 1000,21841] [--k 5] [--reps 50]"""
import argparse, ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd.tensor import _DeviceBuffer

HBM_BYTES_PER_MS = 6.3e9  # tools/layer_report.py

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--classes", default="1000,21841")
ap.add_argument("--k", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()
B, k = a.batch, a.k
lib, ctx = L.lib(), R.get_ctx()
e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
lib.rn_event_create(ctx.handle, ctypes.byref(e0)); lib.rn_event_create(ctx.handle, ctypes.byref(e1))
print(f"rn_softmax_topk_forward, B = {B}, k = {k}, best and median of {a.reps} launches (HIP events around one launch)")
print(f"{'classes':>8s} {'probs':>6s} {'best_ms':>9s} {'median_ms':>9s} {'floor_ms':>9s} {'floor/best':>10s} {'GB/s':>8s}")
for C in [int(c) for c in a.classes.split(",")]:
    x = (3 * np.random.default_rng(C).standard_normal((B, C))).astype(np.float32)
    dx = R.FloatTensor.from_numpy(x, R.Device.GPU)
    probs = R.FloatTensor((B, C), R.Device.GPU)
    tv, ti = R.FloatTensor((B, k), R.Device.GPU), _DeviceBuffer(ctx, B * k * 8)
    for want_probs in (False, True):
        def run():
            L.check(lib.rn_softmax_topk_forward(ctx.handle, dx.data(), probs.data() if want_probs else None, tv.data(),
                                                ti.ptr, B, C, k), "rn_softmax_topk_forward", ctx.handle)
        for _ in range(5):
            run()
        ctx.sync()
        ms = []
        for _ in range(a.reps):
            t = ctypes.c_float()
            lib.rn_event_record(ctx.handle, e0); run(); lib.rn_event_record(ctx.handle, e1)
            L.check(lib.rn_event_elapsed_ms(e0, e1, ctypes.byref(t)), "elapsed", ctx.handle)
            ms.append(t.value)
        nbytes = 4.0 * B * C * (2 if want_probs else 1) + 12.0 * B * k
        floor = nbytes / HBM_BYTES_PER_MS
        best, med = min(ms), float(np.median(ms))
        print(f"{C:8d} {str(want_probs):>6s} {best:9.4f} {med:9.4f} {floor:9.4f} {floor / best:10.3f} {nbytes / best / 1e6:8.0f}")
lib.rn_event_destroy(e0); lib.rn_event_destroy(e1)
