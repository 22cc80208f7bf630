#!/usr/bin/env python3
"""What the stage maps cost: rn_nhwc_to_nchw_dt alone, and ResNet-50 with and without rn_model_forward_maps.

    python tools/maps_rate.py [--batch 256] [--rounds 7] [--reps 10] [--seconds 0.5] [--skip-model] [--skip-kernel]

(a) The kernel alone: the four ResNet-50 stage shapes at 224 x 224 and the two (0,1,1) shapes (layer3 / layer4 at
28 x 28) at B = --batch, fp32 and bf16 sources.  Algorithmic bytes = elements x (source element + 4); GB/s and the
share of 6.3 TB/s.  Every launch of a window works on the next of `sets` source / destination pairs, enough of them
that one round touches more than 600 MB (the Infinity Cache holds 256 MB): the buffers are ROTATED, not enlarged.
On the fp32 buffers the existing rn_nhwc_to_nchw is timed alternately (window by window) with the new kernel;
the best window of each, and the spread (worst - best) of the existing one's windows.

(b) The model: images/s at B = --batch of rn_model_forward_outputs (logits only), rn_model_forward_maps with layer4
only and with all four stages, fp32 and bf16, timed alternately round by round; the loss next to the floor the
traffic alone sets at 6.3 TB/s."""
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

HBM_BYTES_PER_MS = 6.3e9
SHAPES = [("layer1", 256, 56, 56), ("layer2", 512, 28, 28), ("layer3", 1024, 14, 14), ("layer4", 2048, 7, 7),
          ("layer3 (0,1,1)", 1024, 28, 28), ("layer4 (0,1,1)", 2048, 28, 28)]


def elapsed(lib, ctx, events, body):
    e0, e1 = events
    lib.rn_event_record(ctx.handle, e0)
    body()
    lib.rn_event_record(ctx.handle, e1)
    ms = ctypes.c_float()
    L.check(lib.rn_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "elapsed", ctx.handle)
    return ms.value


def kernel(lib, ctx, events, name, dtype, B, C, H, W, rounds, reps):
    es = 2 if dtype == "bf16" else 4
    dt = L.RN_DTYPE_BF16 if es == 2 else L.RN_DTYPE_F32
    n = B * C * H * W
    sets = max(2, -(-600_000_000 // (n * (es + 4))))
    src = [_DeviceBuffer(ctx, n * es) for _ in range(sets)]
    dst = [_DeviceBuffer(ctx, n * 4) for _ in range(sets)]
    for b in src:
        L.check(lib.rn_memset(ctx.handle, b.ptr, 0x3C, n * es), "memset", ctx.handle)
    at = [0]

    def new():
        i = at[0] = (at[0] + 1) % sets
        L.check(lib.rn_nhwc_to_nchw_dt(ctx.handle, dt, src[i].ptr, dst[i].ptr, B, C, H, W), "rn_nhwc_to_nchw_dt", ctx.handle)

    def old():
        i = at[0] = (at[0] + 1) % sets
        L.check(lib.rn_nhwc_to_nchw(ctx.handle, src[i].ptr, dst[i].ptr, B, C, H, W), "rn_nhwc_to_nchw", ctx.handle)

    window = lambda fn: elapsed(lib, ctx, events, lambda: [fn() for _ in range(reps)]) / reps
    for _ in range(sets):
        new()
        if es == 4:
            old()
    ctx.sync()
    tn, to = [], []
    for _ in range(rounds):
        tn.append(window(new))
        if es == 4:
            to.append(window(old))
    nbytes = n * (es + 4)
    rec = {"shape": name, "dtype": dtype, "B": B, "C": C, "H": H, "W": W, "buffer_sets_rotated": sets,
           "algorithmic_mb": round(nbytes / 1e6, 1), "ms": round(min(tn), 4), "gb_per_s": round(nbytes / min(tn) / 1e6, 1),
           "share_of_6.3_tb_per_s": round(nbytes / HBM_BYTES_PER_MS / min(tn), 3), "spread_ms": round(max(tn) - min(tn), 4)}
    if to:
        rec.update({"existing_ms": round(min(to), 4), "existing_gb_per_s": round(nbytes / min(to) / 1e6, 1),
                    "existing_spread_ms": round(max(to) - min(to), 4), "new_over_existing": round(min(tn) / min(to), 3)})
    print(json.dumps(rec), flush=True)


def model(dtype, B, seconds, rounds):
    arch = "resnet50"
    m = R.NativeModel(arch, state=R.weights.generate_state(arch, 0), dtype=dtype)
    lib, ctx = L.lib(), m.ctx
    es = 2 if dtype == "bf16" else 4
    try:
        x = R.FloatTensor.from_numpy(R.weights.generate_input(B, 0), R.Device.GPU)
        logits = R.FloatTensor((B, 1000), R.Device.GPU)
        shapes = m.stage_shapes
        bufs = {s: _DeviceBuffer(ctx, B * int(np.prod(chw)) * 4) for s, chw in shapes.items()}
        outs = L.ModelOutputs(logits.data(), None, None, None, None, 0)
        four, last = L.ModelMaps(), L.ModelMaps()
        for i, s in enumerate(m.STAGES):
            four.layer[i] = bufs[s].ptr
        last.layer[3] = bufs["layer4"].ptr
        runs = {
            "forward_outputs": lambda: L.check(lib.rn_model_forward_outputs(m.handle, x.data(), B, ctypes.byref(outs), L.RN_FWD_FUSED), "outputs", ctx.handle),
            "forward_maps layer4": lambda: L.check(lib.rn_model_forward_maps(m.handle, x.data(), B, ctypes.byref(outs), ctypes.byref(last), L.RN_FWD_FUSED), "maps", ctx.handle),
            "forward_maps all four": lambda: L.check(lib.rn_model_forward_maps(m.handle, x.data(), B, ctypes.byref(outs), ctypes.byref(four), L.RN_FWD_FUSED), "maps", ctx.handle),
        }
        for run in runs.values():
            for _ in range(3):
                run()
        ctx.sync()
        t0 = time.perf_counter()
        runs["forward_outputs"]()
        ctx.sync()
        steps = max(5, int(seconds / max(time.perf_counter() - t0, 1e-5)) + 1)
        e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
        lib.rn_event_create(ctx.handle, ctypes.byref(e0)), lib.rn_event_create(ctx.handle, ctypes.byref(e1))
        ms = {k: [] for k in runs}
        for _ in range(rounds):
            for k, run in runs.items():
                ms[k].append(elapsed(lib, ctx, (e0, e1), lambda: [run() for _ in range(steps)]) / steps)
        lib.rn_event_destroy(e0), lib.rn_event_destroy(e1)
        base = min(ms["forward_outputs"])
        elems = {"forward_outputs": 0, "forward_maps layer4": int(np.prod(shapes["layer4"])),
                 "forward_maps all four": sum(int(np.prod(c)) for c in shapes.values())}
        for k in runs:
            best = min(ms[k])
            floor_ms = B * elems[k] * (es + 4) / HBM_BYTES_PER_MS
            print(json.dumps({"arch": arch, "dtype": dtype, "batch": B, "run": k, "steps": steps, "rounds": rounds,
                              "ms_per_batch": round(best, 3), "spread_ms": round(max(ms[k]) - best, 3),
                              "images_per_s": round(B / best * 1e3, 1), "slowdown": round(best / base - 1, 4),
                              "export_mb": round(B * elems[k] * (es + 4) / 1e6, 1),
                              "floor_ms_at_6.3_tb_per_s": round(floor_ms, 3), "floor_slowdown": round(floor_ms / base, 4)}),
                  flush=True)
    finally:
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    a = ap.parse_args()
    lib, ctx = L.lib(), R.get_ctx()
    if not a.skip_kernel:
        e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
        lib.rn_event_create(ctx.handle, ctypes.byref(e0)), lib.rn_event_create(ctx.handle, ctypes.byref(e1))
        for dtype in ("f32", "bf16"):
            for name, C, H, W in SHAPES:
                kernel(lib, ctx, (e0, e1), name, dtype, a.batch, C, H, W, a.rounds, a.reps)
    if not a.skip_model:
        for dtype in ("f32", "bf16"):
            model(dtype, a.batch, a.seconds, a.rounds)


if __name__ == "__main__":
    main()
