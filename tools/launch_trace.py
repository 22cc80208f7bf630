#!/usr/bin/env python3
"""Every launch the contraction's host side can issue for ResNet-50, one after the other, for a kernel trace; and the
comparison of two such traces.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/launch_trace.py        (once per library:
                                                                                               RN_HIP_LIB selects it)
    python tools/launch_trace.py --compare PARENT_DIR THIS_DIR > launch_trace_parent_against_this.txt
    python tools/launch_trace.py --compare-counts PARENT_DIR THIS_DIR       (the same lines as often, in any order)

The run: every convolution shape of ResNet-50 at 224 x 224 (the stem in its small-Cin and exact-K forms, the 1x1
and 3x3 layers, the downsample layers alone and fused into conv3 as a pair) at B = 256 and B = 1, fp32 and bf16,
once per tile candidate 0 .. rn_conv_tile_candidates(), with split_k = 16 and with 2 XCD groups on candidate 0; the
fc layer fp32 -> fp32 and bf16 -> fp32; the dilated 28 x 28 layers of tools/dilation_rate.py (bf16 also as the dense
panel of 32 groups).  Operands are zero-filled buffers: the values play no part in what is launched.

The comparison: the two sequences of (kernel name, grid size, workgroup size) in dispatch order, line by line."""
import csv
import ctypes
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (Cin, Cout, k, stride, pad, H) of ResNet-50's convolutions (torchvision: the stride in the 3x3)
LAYERS = [(64, 64, 1, 1, 0, 56), (64, 64, 3, 1, 1, 56), (64, 256, 1, 1, 0, 56), (256, 64, 1, 1, 0, 56),
          (256, 128, 1, 1, 0, 56), (128, 128, 3, 2, 1, 56), (128, 512, 1, 1, 0, 28), (256, 512, 1, 2, 0, 56),
          (512, 128, 1, 1, 0, 28), (128, 128, 3, 1, 1, 28),
          (512, 256, 1, 1, 0, 28), (256, 256, 3, 2, 1, 28), (256, 1024, 1, 1, 0, 14), (512, 1024, 1, 2, 0, 28),
          (1024, 256, 1, 1, 0, 14), (256, 256, 3, 1, 1, 14),
          (1024, 512, 1, 1, 0, 14), (512, 512, 3, 2, 1, 14), (512, 2048, 1, 1, 0, 7), (1024, 2048, 1, 2, 0, 14),
          (2048, 512, 1, 1, 0, 7), (512, 512, 3, 1, 1, 7)]
# conv3 + downsample of each stage's first block as one launch: (mid, Cout, H_out, Cin of the block, its stride)
PAIRS = [(64, 256, 56, 64, 1), (128, 512, 28, 256, 2), (256, 1024, 14, 512, 2), (512, 2048, 7, 1024, 2)]
DILATED = [(256, 2), (512, 2), (512, 4)]     # (C, d) on 28 x 28 maps, B = 64


def run():
    import resnet_c_amd as R
    from resnet_c_amd import _lib as L
    from resnet_c_amd.tensor import _DeviceBuffer
    lib, ctx = L.lib(), R.get_ctx()
    h = ctx.handle
    F32, BF16 = L.RN_DTYPE_F32, L.RN_DTYPE_BF16
    ncand = lib.rn_conv_tile_candidates()
    big = 256 * 56 * 56 * 256 * 4           # the largest activation of the list (bytes, fp32); weights below 16 MB
    bufs = {n: _DeviceBuffer(ctx, b) for n, b in (("x", big), ("y", big), ("x2", big), ("w", 64 << 20), ("c", 1 << 16))}
    for b in bufs.values():
        L.check(lib.rn_memset(h, b.ptr, 0, b.nbytes), "memset", h)
    x, y, x2, w, c = (bufs[n].ptr for n in ("x", "y", "x2", "w", "c"))
    ep = L.Epilogue(c, c, None, 1)
    count = [0]

    def settings(launch):
        """one launch per setting: every candidate, then split-K and two XCD groups on the launch's own choice"""
        for cand, split, xcd in [(t, 0, 0) for t in range(ncand + 1)] + [(0, 16, 0), (0, 0, 2)]:
            L.check(lib.rn_ctx_set_conv_tile(h, cand), "tile", h)
            ctx.set_split_k(split), ctx.set_xcd_groups(xcd)
            L.check(launch(), "launch", h)
            count[0] += 1
        L.check(lib.rn_ctx_set_conv_tile(h, 0), "tile", h)
        ctx.set_split_k(0), ctx.set_xcd_groups(0)

    for B in (256, 1):
        for dt in (F32, BF16):
            # the stem: a 4-channel image, fp32 with the kernel's own padding, bf16 physically padded
            if dt == F32:
                settings(lambda: lib.rn_conv2d_nhwc_forward_dt(h, dt, dt, x, y, w, 7, 2, 3, 112, 112, B, 3, 64, 224, 224, ctypes.byref(ep)))
                settings(lambda: lib.rn_conv2d_nhwc_exact_forward(h, x, y, w, 7, 2, 112, 112, B, 3, 64, 230, 230, ctypes.byref(ep)))
            else:
                settings(lambda: lib.rn_conv2d_nhwc_forward_dt(h, dt, dt, x, y, w, 7, 2, 0, 112, 112, B, 3, 64, 230, 230, ctypes.byref(ep)))
            for Cin, Cout, k, s, p, H in LAYERS:
                ho = (H + 2 * p - k) // s + 1
                settings(lambda: lib.rn_conv2d_nhwc_forward_dt(h, dt, dt, x, y, w, k, s, p, ho, ho, B, Cin, Cout, H, H, ctypes.byref(ep)))
            for mid, Cout, ho, Cin2, s2 in PAIRS:
                second = L.ConvSecond(x2, Cin2, ho * s2, ho * s2, s2)
                settings(lambda: lib.rn_conv2d_nhwc_pair_forward_dt(h, dt, dt, x, y, w, 1, 1, 0, ho, ho, B, mid, Cout, ho, ho,
                                                                    ctypes.byref(second), ctypes.byref(ep)))
        settings(lambda: lib.rn_linear_forward(h, x, y, w, c, B, 2048, 1000))
        settings(lambda: lib.rn_conv2d_nhwc_forward_dt(h, BF16, F32, x, y, w, 1, 1, 0, 1, 1, B, 2048, 1000, 1, 1, ctypes.byref(ep)))
    for dt in (F32, BF16):
        for C, d in DILATED:
            for G in (1, 32) if dt == BF16 else (1,):
                settings(lambda: lib.rn_conv2d_dilated_nhwc_forward_dt(h, dt, dt, x, y, w, 3, 1, d, d, 28, 28, 64, C, C, 28, 28, G,
                                                                        ctypes.byref(ep)))
    ctx.sync()
    print(f"launch_trace: {count[0]} entry-point calls, candidates 0..{ncand}", flush=True)


def trace(d):
    f = max(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    g = lambda r, n: "x".join(r[f"{n}_{a}"] for a in "XYZ")
    return [f"{r['Kernel_Name']} grid {g(r, 'Grid_Size')} workgroup {g(r, 'Workgroup_Size')}" for r in rows]


def compare(a_dir, b_dir):
    a, b = trace(a_dir), trace(b_dir)
    differ = [i for i, (p, q) in enumerate(zip(a, b)) if p != q]
    ndiff = len(differ) + abs(len(a) - len(b))
    print(f"launches of the parent's library: {len(a)}; of this one: {len(b)}")
    print(f"kernel names that appear: {len(set(a))} distinct (name, grid, workgroup) lines, "
          f"{len(set(l.split(' grid ')[0] for l in a))} kernels")
    print(f"launches compared: {min(len(a), len(b))}; that differ: {ndiff}")
    if differ:
        print(f"first differing line ({differ[0] + 1}):\n  parent: {a[differ[0]]}\n  this:   {b[differ[0]]}")
    return 1 if ndiff else 0


def compare_counts(a_dir, b_dir):
    """the same (kernel name, grid, workgroup) lines the same number of times, whatever their order: for two builds that
    issue the same launches but queue a model's uploads and packs at another moment"""
    from collections import Counter
    a, b = Counter(trace(a_dir)), Counter(trace(b_dir))
    wrong = sorted(k for k in set(a) | set(b) if a[k] != b[k])
    print(f"launches of the parent's library: {sum(a.values())}; of this one: {sum(b.values())}")
    print(f"distinct (name, grid, workgroup) lines: {len(a)} / {len(b)}; kernels: {len(set(l.split(' grid ')[0] for l in a))} / "
          f"{len(set(l.split(' grid ')[0] for l in b))}")
    print(f"lines whose count differs: {len(wrong)}")
    for k in wrong[:10]:
        print(f"  parent {a[k]}, this {b[k]}: {k}")
    return 1 if wrong else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("--compare", "--compare-counts"):
        sys.exit((compare if sys.argv[1] == "--compare" else compare_counts)(sys.argv[2], sys.argv[3]))
    sys.exit(run())
