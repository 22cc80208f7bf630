#!/usr/bin/env python3
"""What the pyramid costs: rn_upsample_nearest_add_forward_dt alone, and ResNet-50 with torchvision's FPN neck.

    python tools/fpn_rate.py [--rounds 5] [--reps 10] [--seconds 0.3] [--skip-model] [--skip-kernel]
                             [--arch resnet50] [--sizes "32,224;8,512"] [--channels 256]

(a) The top-down launch alone at the three steps of a ResNet-50 pyramid on 224 x 224 images (7 -> 14, 14 -> 28,
28 -> 56, 256 channels, B = 64), fp32 and bf16, in place on the lateral as the neck runs it.  Bytes moved = the finer
tensor read and written + the coarser tensor once (its repeats come from cache); GB/s and the share of 6.3 TB/s.
Every launch of a window works on the next of `sets` buffer pairs (rotated until a round touches 600 MB, at most 32).
(b) The model: images/s of rn_model_forward_fpn (all five outputs, left on the device) against
rn_model_forward_outputs (the logits) at the same batch, fp32 and bf16, timed alternately round by round (wall clock
around a synchronised call), then one line per launch of the neck from the model's profile records."""
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
from resnet_c_amd import fpn as P
from resnet_c_amd.tensor import _DeviceBuffer

HBM_BYTES_PER_MS = 6.3e9
KERNEL_SHAPES = [(64, 7, 14, 256), (64, 14, 28, 256), (64, 28, 56, 256)]
MODEL_SHAPES = [(32, 224), (8, 512)]


def elapsed(lib, ctx, events, body):
    e0, e1 = events
    lib.rn_event_record(ctx.handle, e0)
    body()
    lib.rn_event_record(ctx.handle, e1)
    ms = ctypes.c_float()
    L.check(lib.rn_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "elapsed", ctx.handle)
    return ms.value


def kernel(lib, ctx, events, B, n_in, n_out, C, dtype, rounds, reps):
    es = 2 if dtype == "bf16" else 4
    top_bytes, lat_bytes = B * n_in * n_in * C * es, B * n_out * n_out * C * es
    moved = top_bytes + 2 * lat_bytes
    sets = min(32, max(2, -(-600_000_000 // moved)))
    zeros = np.zeros(lat_bytes, np.uint8)
    top = [_DeviceBuffer(ctx, top_bytes) for _ in range(sets)]
    lat = [_DeviceBuffer(ctx, lat_bytes) for _ in range(sets)]
    for bufs, nbytes in ((top, top_bytes), (lat, lat_bytes)):      # zeros: sums stay finite however often a set is reused
        for b in bufs:
            L.check(lib.rn_memcpy_h2d(ctx.handle, b.ptr, zeros.ctypes.data, nbytes), "h2d", ctx.handle)
    at = [0]
    dt = L.RN_DTYPE_BF16 if dtype == "bf16" else L.RN_DTYPE_F32

    def run():
        i = at[0] = (at[0] + 1) % sets
        L.check(lib.rn_upsample_nearest_add_forward_dt(ctx.handle, dt, top[i].ptr, B, n_in, n_in, C, lat[i].ptr, lat[i].ptr,
                                                       n_out, n_out), "rn_upsample_nearest_add_forward_dt", ctx.handle)

    for _ in range(sets):
        run()
    ctx.sync()
    t = [elapsed(lib, ctx, events, lambda: [run() for _ in range(reps)]) / reps for _ in range(rounds)]
    print(json.dumps({"launch": "rn_upsample_nearest_add_forward_dt", "dtype": dtype, "B": B, "top": [n_in, n_in],
                      "dst": [n_out, n_out], "C": C, "in_place": True, "buffer_sets_rotated": sets,
                      "cache_resident": moved * sets < 256e6, "moved_mb": round(moved / 1e6, 2), "ms": round(min(t), 4),
                      "spread_ms": round(max(t) - min(t), 4), "gb_per_s": round(moved / min(t) / 1e6, 1),
                      "share_of_6.3_tb_per_s": round(moved / HBM_BYTES_PER_MS / min(t), 3)}), flush=True)


def model(arch, dtype, B, side, channels, seconds, rounds):
    m = R.NativeModel(arch, state=R.weights.generate_state(arch, 0), dtype=dtype, input_size=(side, side))
    shapes = m.stage_shapes
    cin = [shapes[s][0] for s in m.STAGES]
    neck = P.FeaturePyramidNetwork(cin, channels, P.generate_fpn_state(cin, channels, 0), dtype=dtype)
    lib, ctx = L.lib(), m.ctx
    try:
        x = R.FloatTensor.from_numpy(R.weights.generate_input(B, 0, hw=side), R.Device.GPU)
        logits = _DeviceBuffer(ctx, B * m.classes * 4)
        outs = L.ModelOutputs(logits.ptr, None, None, None, None, 0)
        fo, keep = L.FpnOutputs(), []
        for i, name in enumerate(neck.names):
            _, h, w = shapes[m.STAGES[min(i, 3)]]
            c, hh, ww = neck.level_shape(name, h, w)
            keep.append(_DeviceBuffer(ctx, B * c * hh * ww * 4))
            fo.level[i] = keep[-1].ptr
        stages = (ctypes.c_int * 4)(1, 2, 3, 4)

        def run_outputs():
            L.check(lib.rn_model_forward_outputs(m.handle, x.data(), B, ctypes.byref(outs), L.RN_FWD_FUSED), "outputs", ctx.handle)

        def run_fpn():
            L.check(lib.rn_model_forward_fpn(m.handle, neck.handle, x.data(), B, ctypes.byref(outs), stages, ctypes.byref(fo),
                                             L.RN_FWD_FUSED), "fpn", ctx.handle)

        runs = {"forward_outputs (logits)": run_outputs, "forward_fpn (logits + five levels)": run_fpn}

        def wall(run, steps):
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                run()
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3 / steps

        for run in runs.values():
            wall(run, 2)
        steps = max(3, int(seconds * 1e3 / wall(run_fpn, 1)) + 1)
        ms = {k: [] for k in runs}
        for _ in range(rounds):
            for k, run in runs.items():
                ms[k].append(wall(run, steps))
        base = min(ms["forward_outputs (logits)"])
        for k in runs:
            best = min(ms[k])
            print(json.dumps({"arch": arch, "dtype": dtype, "batch": B, "size": side, "out_channels": channels, "run": k,
                              "steps": steps, "rounds": rounds, "ms_per_batch": round(best, 3),
                              "spread_ms": round(max(ms[k]) - best, 3), "images_per_s": round(B / best * 1e3, 1),
                              "against_outputs": round(best / base, 4)}), flush=True)
        xh = R.weights.generate_input(B, 0, hw=side)
        m.set_profiling(True)
        try:
            m.forward_fpn(xh, neck)
            recs = m.profile()
        finally:
            m.set_profiling(False)
        tag = {"arch": arch, "dtype": dtype, "batch": B, "size": side}
        for r in (r for r in recs if r["layer"] == "fpn"):
            print(json.dumps(dict(tag, op=r["op"], ms=round(r["ms"], 4), gflop=round(r["flops"] / 1e9, 3),
                                  tflops=round(r["flops"] / r["ms"] / 1e9, 1) if r["ms"] > 0 and r["flops"] else None,
                                  gb_per_s=round(r["bytes"] / r["ms"] / 1e6, 1) if r["ms"] > 0 else None)), flush=True)
        print(json.dumps(dict(tag, op="neck total", ms=round(sum(r["ms"] for r in recs if r["layer"] == "fpn"), 4),
                              forward_total_ms=round(sum(r["ms"] for r in recs), 4))), flush=True)
    finally:
        neck.close()
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--sizes", default="", help="B,side[;B,side...] in place of 32,224;8,512")
    a = ap.parse_args()
    lib, ctx = L.lib(), R.get_ctx()
    if not a.skip_kernel:
        e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
        lib.rn_event_create(ctx.handle, ctypes.byref(e0)), lib.rn_event_create(ctx.handle, ctypes.byref(e1))
        for dtype in ("f32", "bf16"):
            for shape in KERNEL_SHAPES:
                kernel(lib, ctx, (e0, e1), *shape, dtype, a.rounds, a.reps)
    if not a.skip_model:
        shapes = [tuple(int(v) for v in t.split(",")) for t in a.sizes.split(";")] if a.sizes else MODEL_SHAPES
        for dtype in ("f32", "bf16"):
            for B, side in shapes:
                model(a.arch, dtype, B, side, a.channels, a.seconds, a.rounds)


if __name__ == "__main__":
    main()
