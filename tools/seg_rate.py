#!/usr/bin/env python3
"""What the label map costs: rn_upsample_bilinear_forward alone, and ResNet-50 (0,1,1) with a 21-class FCN head.

    python tools/seg_rate.py [--rounds 5] [--reps 10] [--seconds 0.3] [--skip-model] [--skip-kernel]
                             [--head fcn|deeplabv3] [--dilate a,b,c] [--steps-profile]

--head deeplabv3 runs (c) with torchvision's DeepLabHead (ASPP 256, rates 12, 24, 36) instead of the FCN head;
--dilate sets the backbone's replace_stride_with_dilation (default 0,1,1); --steps-profile adds one line per launch
of the head from the model's profile records (a DeepLab head: once with the centre-tap plan, once without).  With
none of the three the output is what it always was.

(a) The upsample launch alone, coarse scores [B,h,w,24] (21 classes) at output stride 8 to 224 x 224 (B = 64) and
512 x 512 (B = 16), in its three forms: labels only, scores only, both.  Bytes actually moved = the source once +
one byte per pixel (labels) + 4 x 21 bytes per pixel (scores); GB/s and the share of 6.3 TB/s.  Every launch of a
window works on the next of `sets` buffer pairs (rotated, at most 32 sets, until a round touches 600 MB): the
labels-only form moves so little that its buffers stay cache-resident whatever is rotated, which its line says.
(b) Labels only against what it replaces on the device: the scores-only launch followed by torch.argmax(dim=1) on
the same buffer, each timed with its own events on its own stream and added.
(c) The model: images/s of rn_model_forward_segment (labels only, downloaded: one byte per pixel) against
rn_model_forward_maps(layer4) plus the download of the [B,2048,H/8,W/8] fp32 map the host-side head would need,
fp32 and bf16, at 224 x 224 (B = 32) and 512 x 512 (B = 8), timed alternately round by round (wall clock around a
synchronised call: both include their download)."""
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
from resnet_c_amd import segmentation as S
from resnet_c_amd.tensor import _DeviceBuffer

HBM_BYTES_PER_MS = 6.3e9
CLASSES, CS = 21, 24
KERNEL_SHAPES = [(64, 28, 28, 224, 224), (16, 64, 64, 512, 512)]
MODEL_SHAPES = [(32, 224), (8, 512)]


def elapsed(lib, ctx, events, body):
    e0, e1 = events
    lib.rn_event_record(ctx.handle, e0)
    body()
    lib.rn_event_record(ctx.handle, e1)
    ms = ctypes.c_float()
    L.check(lib.rn_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "elapsed", ctx.handle)
    return ms.value


def kernel(lib, ctx, events, B, h, w, H, W, rounds, reps):
    import torch
    src_bytes, pix = B * h * w * CS * 4, B * H * W
    x = np.random.default_rng(0).standard_normal((B, h, w, CS), dtype=np.float32)
    times = {}
    for form, want_s, want_l in (("labels", False, True), ("scores", True, False), ("both", True, True)):
        moved = src_bytes + (pix * CLASSES * 4 if want_s else 0) + (pix if want_l else 0)
        sets = min(32, max(2, -(-600_000_000 // moved)))
        src = [_DeviceBuffer(ctx, src_bytes) for _ in range(sets)]
        for b in src:
            L.check(lib.rn_memcpy_h2d(ctx.handle, b.ptr, x.ctypes.data, src_bytes), "h2d", ctx.handle)
        sc = [_DeviceBuffer(ctx, pix * CLASSES * 4) for _ in range(sets)] if want_s else None
        lb = [_DeviceBuffer(ctx, pix) for _ in range(sets)] if want_l else None
        at = [0]

        def run():
            i = at[0] = (at[0] + 1) % sets
            L.check(lib.rn_upsample_bilinear_forward(ctx.handle, src[i].ptr, B, h, w, CLASSES, CS, H, W,
                                                     sc[i].ptr if sc else None, lb[i].ptr if lb else None),
                    "rn_upsample_bilinear_forward", ctx.handle)

        for _ in range(sets):
            run()
        ctx.sync()
        t = [elapsed(lib, ctx, events, lambda: [run() for _ in range(reps)]) / reps for _ in range(rounds)]
        times[form] = min(t)
        print(json.dumps({"launch": "rn_upsample_bilinear_forward", "form": form, "B": B, "src": [h, w], "dst": [H, W],
                          "classes": CLASSES, "buffer_sets_rotated": sets, "cache_resident": moved * sets < 256e6,
                          "moved_mb": round(moved / 1e6, 2), "ms": round(min(t), 4), "spread_ms": round(max(t) - min(t), 4),
                          "gb_per_s": round(moved / min(t) / 1e6, 1),
                          "share_of_6.3_tb_per_s": round(moved / HBM_BYTES_PER_MS / min(t), 3)}), flush=True)
        del src, sc, lb
    # scores-only followed by torch.argmax on the device, against the fused labels-only launch
    scores = torch.empty((B, CLASSES, H, W), dtype=torch.float32, device="cuda")
    for _ in range(3):
        torch.argmax(scores, dim=1)
    torch.cuda.synchronize()
    t = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            torch.argmax(scores, dim=1)
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) / reps)
    print(json.dumps({"compare": "labels only against scores only + torch.argmax(dim=1)", "B": B, "dst": [H, W],
                      "labels_only_ms": round(times["labels"], 4), "scores_only_ms": round(times["scores"], 4),
                      "torch_argmax_ms": round(min(t), 4), "scores_then_argmax_ms": round(times["scores"] + min(t), 4),
                      "fused_over_unfused": round(times["labels"] / (times["scores"] + min(t)), 4)}), flush=True)


def steps_profile(m, head, x_host, tag):
    """one line per launch of the head: the profile records of layer "segmentation" of one labels-only forward"""
    m.forward_segment(x_host, head)
    m.set_profiling(True)
    try:
        m.forward_segment(x_host, head)
        recs = [r for r in m.profile() if r["layer"] == "segmentation"]
    finally:
        m.set_profiling(False)
    for r in recs:
        print(json.dumps(dict(tag, op=r["op"], ms=round(r["ms"], 4), gflop=round(r["flops"] / 1e9, 3),
                              tflops=round(r["flops"] / r["ms"] / 1e9, 1) if r["ms"] > 0 else None)), flush=True)
    print(json.dumps(dict(tag, op="head total", ms=round(sum(r["ms"] for r in recs), 4))), flush=True)


def model(dtype, B, side, seconds, rounds, head_kind="fcn", flags=(0, 1, 1), profile=False):
    arch = "resnet50"
    m = R.NativeModel(arch, state=R.weights.generate_state(arch, 0), dtype=dtype, input_size=(side, side),
                      replace_stride_with_dilation=tuple(flags))
    if head_kind == "fcn":
        head = S.FCNHead(m.features, CLASSES, S.generate_fcn_head_state(m.features, CLASSES, 0), dtype=dtype)
    else:
        head = S.DeepLabHead(m.features, CLASSES, S.generate_deeplab_head_state(m.features, CLASSES, seed=0), dtype=dtype)
    lib, ctx = L.lib(), m.ctx
    try:
        x = R.FloatTensor.from_numpy(R.weights.generate_input(B, 0, hw=side), R.Device.GPU)
        C4, h4, w4 = m.stage_shapes["layer4"]
        dmap, dlab = _DeviceBuffer(ctx, B * C4 * h4 * w4 * 4), _DeviceBuffer(ctx, B * side * side)
        hmap, hlab = np.empty(B * C4 * h4 * w4, np.float32), np.empty(B * side * side, np.uint8)
        maps, seg = L.ModelMaps(), L.SegOutputs(dlab.ptr, None)
        maps.layer[3] = dmap.ptr

        def run_maps():
            L.check(lib.rn_model_forward_maps(m.handle, x.data(), B, None, ctypes.byref(maps), L.RN_FWD_FUSED), "maps", ctx.handle)
            L.check(lib.rn_memcpy_d2h(ctx.handle, hmap.ctypes.data, dmap.ptr, hmap.nbytes), "d2h", ctx.handle)

        def run_seg():
            L.check(lib.rn_model_forward_segment(m.handle, head.handle, x.data(), B, None, ctypes.byref(seg), L.RN_FWD_FUSED),
                    "segment", ctx.handle)
            L.check(lib.rn_memcpy_d2h(ctx.handle, hlab.ctypes.data, dlab.ptr, hlab.nbytes), "d2h", ctx.handle)

        runs = {"forward_maps(layer4) + download of the map": run_maps, "forward_segment, labels only + download": run_seg}

        def wall(run, steps):
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                run()
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3 / steps

        for run in runs.values():
            wall(run, 2)
        steps = max(3, int(seconds * 1e3 / wall(run_seg, 1)) + 1)
        ms = {k: [] for k in runs}
        for _ in range(rounds):
            for k, run in runs.items():
                ms[k].append(wall(run, steps))
        base = min(ms["forward_maps(layer4) + download of the map"])
        for k in runs:
            best = min(ms[k])
            extra = {} if head_kind == "fcn" else {"head": head_kind}
            print(json.dumps({"arch": arch, **extra, "dilation": list(flags), "dtype": dtype, "batch": B, "size": side, "run": k,
                              "steps": steps, "rounds": rounds, "ms_per_batch": round(best, 3),
                              "spread_ms": round(max(ms[k]) - best, 3), "images_per_s": round(B / best * 1e3, 1),
                              "downloaded_mb": round((hmap.nbytes if run_maps is runs[k] else hlab.nbytes) / 1e6, 2),
                              "against_maps": round(best / base, 4)}), flush=True)
        if profile:
            tag = {"head": head_kind, "dilation": list(flags), "dtype": dtype, "batch": B, "size": side,
                   "map": list(m.stage_shapes["layer4"][1:])}
            xh = R.weights.generate_input(B, 0, hw=side)
            if head_kind == "fcn":
                steps_profile(m, head, xh, tag)
            else:
                for on in (True, False):
                    head.center_tap(on)
                    steps_profile(m, head, xh, dict(tag, center_tap=on))
                head.center_tap(True)
    finally:
        head.close()
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--head", choices=("fcn", "deeplabv3"), default="fcn")
    ap.add_argument("--dilate", default="0,1,1")
    ap.add_argument("--steps-profile", action="store_true")
    ap.add_argument("--sizes", default="", help="B,side[;B,side...] in place of 32,224;8,512")
    a = ap.parse_args()
    lib, ctx = L.lib(), R.get_ctx()
    if not a.skip_kernel:
        e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
        lib.rn_event_create(ctx.handle, ctypes.byref(e0)), lib.rn_event_create(ctx.handle, ctypes.byref(e1))
        for shape in KERNEL_SHAPES:
            kernel(lib, ctx, (e0, e1), *shape, a.rounds, a.reps)
    if not a.skip_model:
        for dtype in ("f32", "bf16"):
            shapes = [tuple(int(v) for v in t.split(",")) for t in a.sizes.split(";")] if a.sizes else MODEL_SHAPES
            for B, side in shapes:
                model(dtype, B, side, a.seconds, a.rounds, a.head, tuple(int(v) for v in a.dilate.split(",")), a.steps_profile)


if __name__ == "__main__":
    main()
