"""Device resize (rn_image_u8_resize_crop): the launch against its byte floor, and the image pipeline
against the host route it replaces.

  1. time of the resize launch at B = 256 for 375x500 and 1080x1920 sources (events around `--reps`
     launches after `--warmup`, tables uploaded once), beside its byte floor: the source bytes the
     crop reads (the rows and columns its taps touch) + 150,528 written per image, at 6.29 TB/s (the
     measured HBM copy rate of an MI355X);
  2. end to end, bf16 resnet50, B = 256, 375x500 sources in pageable memory: images/s of
     Pipeline(input="images") against PIL's resize + crop on `--workers` processes (they never open
     the GPU) feeding Pipeline(input="u8"), `--repeats` times each, alternating.

    python tools/resize_bench.py > profiles/resize/resize_bench.txt
"""
import argparse
import ctypes
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 6.29e12
_IMGS = None


def make_images(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(n)]


def _worker_init(n, h, w, seed):
    global _IMGS
    _IMGS = make_images(n, h, w, seed)


def _worker_crop(i):
    """The host route: preprocess_image_u8's resize and crop from a decoded array (PIL, one core)."""
    from PIL import Image
    im = Image.fromarray(_IMGS[i % len(_IMGS)])
    w, h = im.size
    nw, nh = (256, int(256 * h / w)) if w <= h else (int(256 * w / h), 256)
    im = im.resize((nw, nh), Image.BILINEAR)
    left, top = int(round((nw - 224) / 2.0)), int(round((nh - 224) / 2.0))
    return np.asarray(im.crop((left, top, left + 224, top + 224)), dtype=np.uint8)


def kernel_time(R, L, ops, P, h, w, B, warmup, reps):
    ctx, lib = R.get_ctx(), L.lib()
    imgs = make_images(8, h, w, 1)
    imgs = [imgs[i % 8] for i in range(B)]
    packed, offsets, heights, widths = ops.pack_images(imgs)
    u = ops._u64p
    n = ctypes.c_uint64()
    L.check(lib.rn_image_u8_resize_crop_table(u(offsets), u(heights), u(widths), B, 256, 224, None, 0, ctypes.byref(n)), "table")
    tab = np.zeros(n.value, dtype=np.uint8)
    L.check(lib.rn_image_u8_resize_crop_table(u(offsets), u(heights), u(widths), B, 256, 224, tab.ctypes.data, tab.nbytes,
                                              ctypes.byref(n)), "table")
    src, dtab = ops._up_raw(packed), ops._up_raw(tab)
    from resnet_c_amd.tensor import _DeviceBuffer
    dst = _DeviceBuffer(ctx, B * 150528)
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    lib.rn_event_create(ctx.handle, ctypes.byref(e0))
    lib.rn_event_create(ctx.handle, ctypes.byref(e1))

    def launch(k):
        for _ in range(k):
            L.check(lib.rn_image_u8_resize_crop_launch(ctx.handle, src.ptr, dtab.ptr, B, dst.ptr, 224), "launch", ctx.handle)

    launch(warmup)
    ctx.sync()
    times = []
    for _ in range(5):
        lib.rn_event_record(ctx.handle, e0)
        launch(reps)
        lib.rn_event_record(ctx.handle, e1)
        ms = ctypes.c_float()
        L.check(lib.rn_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "elapsed")
        times.append(ms.value / reps)
    got = ops._down_raw(dst, np.uint8, 150528).reshape(224, 224, 3)
    assert np.array_equal(got, P.resize_crop_u8(imgs[0]))
    nh, nw, top, left = P.resize_crop_geometry(h, w)
    hb, _, _ = P.resize_coefficients(w, nw, left, 224)
    vb, _, _ = P.resize_coefficients(h, nh, top, 224)
    rows = int(vb[-1, 0] + vb[-1, 1] - vb[0, 0])
    cols = int(hb[-1, 0] + hb[-1, 1] - hb[0, 0])
    floor_ms = B * (rows * cols * 3 + 150528) / HBM * 1e3
    t = sorted(times)[len(times) // 2]
    lib.rn_event_destroy(e0)
    lib.rn_event_destroy(e1)
    return {"what": "resize launch", "source": f"{h}x{w}", "B": B, "ms_median": round(t, 4), "ms_min": round(min(times), 4),
            "ms_max": round(max(times), 4), "rows_read": rows, "cols_read": cols, "byte_floor_ms": round(floor_ms, 4),
            "fraction_of_floor_rate": round(floor_ms / t, 4), "images_per_s": round(B / t * 1e3)}


def run_images(pipe, imgs, batches):
    t = time.perf_counter()
    for _ in range(batches):
        if pipe.in_flight() == 2:
            pipe.collect_top1()
        pipe.submit_images(imgs)
    while pipe.in_flight():
        pipe.collect_top1()
    return len(imgs) * batches / (time.perf_counter() - t)


def run_host(pipe, pool, B, batches):
    t = time.perf_counter()
    buf, k = np.empty((B, 224, 224, 3), dtype=np.uint8), 0
    for crop in pool.imap(_worker_crop, range(B * batches), chunksize=8):
        buf[k] = crop
        k += 1
        if k == B:
            if pipe.in_flight() == 2:
                pipe.collect_top1()
            pipe.submit_u8(buf)      # copied into pinned staging before the call returns
            k = 0
    while pipe.in_flight():
        pipe.collect_top1()
    return B * batches / (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-end-to-end", action="store_true")
    a = ap.parse_args()
    B = a.batch
    pool = None
    if not a.no_end_to_end:     # the workers start before this process opens the GPU, and never open it
        pool = mp.get_context("spawn").Pool(a.workers, initializer=_worker_init, initargs=(B, 375, 500, 7))
        pool.map(_worker_crop, range(a.workers * 4))
    import resnet_c_amd as R
    from resnet_c_amd import _lib as L
    from resnet_c_amd import ops
    from resnet_c_amd import preprocess as P
    for h, w in ((375, 500), (1080, 1920)):
        print(json.dumps(kernel_time(R, L, ops, P, h, w, B, a.warmup, a.reps)), flush=True)
    if a.no_end_to_end:
        return
    imgs = make_images(B, 375, 500, 7)
    m = R.NativeModel("resnet50", state=R.weights.generate_state("resnet50", seed=0), dtype="bf16")
    pi = R.Pipeline(m, B, input="images", max_batch_bytes=B * 375 * 500 * 3)
    pu = R.Pipeline(m, B, input="u8")
    run_images(pi, imgs, 2)
    run_host(pu, pool, B, 2)
    new, old = [], []
    for _ in range(a.repeats):
        old.append(run_host(pu, pool, B, a.batches))
        new.append(run_images(pi, imgs, a.batches))
    pool.close()
    pool.join()
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({"what": "end to end, bf16 resnet50, 375x500 pageable sources", "B": B, "batches": a.batches,
                      "host_route_workers": a.workers, "host_route_images_per_s": [round(v) for v in old],
                      "image_pipeline_images_per_s": [round(v) for v in new], "host_route_median": round(med(old)),
                      "host_route_spread": round((max(old) - min(old)) / med(old), 4),
                      "image_pipeline_median": round(med(new)), "ratio": round(med(new) / med(old), 3)}), flush=True)
    pi.close()
    pu.close()
    m.close()


if __name__ == "__main__":
    main()
