#!/usr/bin/env python3
"""Randomised run of the fp32 op entry points on offset views (tests/views.py): a random entry point, a
random shape from ops_fuzz.py's ranges (convolutions: small ones of their own), every operand at a random offset of 0, 4, 8 or 12 bytes from a
16-byte boundary, 256-byte guard bands around every operand.  Element-wise ops, pools, batch-norm and
layout changes bit-exact with the CPU oracle / numpy; linear and the convolutions bit-exact where the
alignment sends them to the direct kernel, within the suite's bounds otherwise.

    python tests/fuzz/view_fuzz.py [--seconds 60] [--seed 0]"""
import argparse
import os
import sys
import time

_TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(_TESTS))
sys.path.insert(0, _TESTS)
import numpy as np

import views as V
from oracle import oracle as O

OFFSETS = (0, 4, 8, 12)


def offs_for(g, *names):
    return {n: int(g.choice(OFFSETS)) for n in names}


def close(got, want, k_terms, what):   # assert_close of tests/test_ops_gpu.py
    tol = 3e-7 * np.sqrt(k_terms) * (float(np.abs(want).max()) + 1e-6) + 1e-6
    assert got.shape == want.shape and float(np.abs(got - want).max()) <= tol, what


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), what


def one_case(g, what):
    layout = str(g.choice(["nchw", "nhwc"]))
    if what in ("maxpool", "avgpool"):
        k, s = int(g.choice([1, 2, 3, 3, 7])), int(g.choice([1, 2, 3, 7]))
        p = int(g.integers(0, k // 2 + 1))
        B, C = int(g.integers(1, 9)), int(g.choice([1, 3, 4, 8, 12, 64, 100, 256]))
        H, W = int(g.integers(max(1, k - 2 * p), 20)), int(g.integers(max(1, k - 2 * p), 20))
        if C >= 256:
            H, W = min(H, 8), min(W, 8)
        elif what == "maxpool" and g.random() < 0.3:
            k, s, p, H = 3, 2, 1, int(g.integers(15, 60))
        if what == "avgpool" and g.random() < 0.4:
            H = W = k = 7
            s, p = int(g.choice([1, 7])), 0
        x = g.standard_normal((B, C, H, W), dtype=np.float32)
        offs = offs_for(g, "inp", "out")
        want = (O.maxpool2d if what == "maxpool" else O.avgpool2d)(x, k, s, p)
        same(V.run_pool(what[:3], x, k, s, p, layout, offs), want, f"{what} {layout} {x.shape} k={k} s={s} p={p} {offs}")
    elif what == "batchnorm":
        B, C = int(g.integers(1, 40)), int(g.choice([1, 2, 3, 4, 5, 8, 33, 64, 70, 256]))
        H, W = int(g.integers(1, 20)), int(g.integers(1, 20))
        x = g.standard_normal((B, C, H, W), dtype=np.float32) * 3
        w, b = g.random(C, dtype=np.float32) + 0.5, g.standard_normal(C, dtype=np.float32)
        m, v = g.standard_normal(C, dtype=np.float32), g.random(C, dtype=np.float32) + 0.5
        offs, inplace = offs_for(g, "inp", "out", "weight", "bias", "mean", "var"), bool(g.integers(0, 2))
        same(V.run_batchnorm(x, w, b, m, v, layout, offs, inplace), O.batchnorm2d(x, w, b, m, v),
             f"batchnorm {layout} {x.shape} inplace={inplace} {offs}")
    elif what == "linear":
        B, I, Oo = int(g.integers(1, 70)), int(g.choice([1, 7, 32, 64, 96, 300, 2048])), int(g.integers(1, 130))
        x, w = g.standard_normal((B, I), dtype=np.float32), g.standard_normal((Oo, I), dtype=np.float32) / np.sqrt(I)
        b = g.standard_normal(Oo, dtype=np.float32) if g.random() < 0.7 else None
        offs = offs_for(g, "inp", "out", "weight", "bias")
        got, want = V.run_linear(x, w, b, offs), O.linear(x, w, b)
        if V.linear_is_direct(I, b, offs):
            same(got, want, f"linear {B}x{I}->{Oo} {offs}")
        else:
            close(got, want, I, f"linear {B}x{I}->{Oo} {offs}")
    elif what == "conv2d":
        B, Cin, Cout = int(g.integers(1, 4)), int(g.choice([3, 5, 32, 48, 64])), int(g.choice([3, 8, 40, 64, 72]))
        k = int(g.choice([1, 1, 3])) if Cin >= 5 else int(g.choice([3, 7]))
        s, p = int(g.choice([1, 2])), int(g.integers(0, k // 2 + 1))
        H, W = int(g.integers(k, 15)), int(g.integers(k, 15))
        taps = int(g.choice([0, 1, 2]))
        x = g.standard_normal((B, Cin, H, W), dtype=np.float32)
        w = g.standard_normal((Cout, Cin, k, k), dtype=np.float32) / np.sqrt(Cin * k * k)
        offs = offs_for(g, "inp", "out", "weight")
        got, want = V.run_conv2d(x, w, s, p, layout, taps, offs), O.conv2d(x, w, s, p)
        label = f"conv2d {layout} taps={taps} {(B, Cin, Cout, H, W, k, s, p)} {offs}"
        if V.conv2d_is_direct((B, Cin, Cout, H, W, k, s, p), layout, taps, offs):
            same(got, want, label)
        else:
            close(got, want, Cin * k * k, label)
    elif what == "conv_nhwc":
        B, Cin, Cout = int(g.integers(1, 4)), int(g.choice([3, 4, 5, 32, 64])), int(g.choice([8, 40, 64, 96]))
        k = int(g.choice([1, 3]))
        s, p = int(g.choice([1, 2])), int(g.integers(0, k // 2 + 1))
        H, W = int(g.integers(k, 13)), int(g.integers(k, 13))
        x = g.standard_normal((B, Cin, H, W), dtype=np.float32)
        w = (g.standard_normal((Cout, Cin, k, k), dtype=np.float32) / np.sqrt(Cin * k * k)).astype(np.float32)
        scale = g.random(Cout, dtype=np.float32) + 0.5 if g.random() < 0.5 else None
        shift = g.standard_normal(Cout, dtype=np.float32) if g.random() < 0.7 else None
        y = O.conv2d(x, w, s, p)
        res = g.standard_normal(y.shape, dtype=np.float32) if g.random() < 0.6 else None
        relu = bool(g.integers(0, 2))
        names = ["inp", "out", "weight"] + [n for n, v in (("scale", scale), ("shift", shift), ("residual", res)) if v is not None]
        offs = offs_for(g, *names)
        got = V.run_conv_nhwc(x, w, s, p, scale, shift, res, relu, offs)
        want = y if scale is None else y * scale[None, :, None, None]
        if shift is not None:
            want = want + shift[None, :, None, None]
        if res is not None:
            want = want + res
        want = np.maximum(want, 0) if relu else want
        label = f"conv_nhwc {(B, Cin, Cout, H, W, k, s, p)} scale={scale is not None} shift={shift is not None} res={res is not None} relu={relu} {offs}"
        if scale is None and V.conv_nhwc_is_direct(Cin, k, offs):
            same(got, want.astype(np.float32), label)   # the direct kernel's epilogue without a scale: the op sequence in fp32
        else:
            close(got, want, Cin * k * k + 4, label)
    elif what == "argmax":
        B, C = int(g.integers(1, 12)), int(g.choice([1, 5, 63, 64, 65, 1000]))
        logits = g.standard_normal((B, C), dtype=np.float32)
        if g.random() < 0.5:
            logits[0, int(g.integers(0, C))] = np.nan
        offs = offs_for(g, "logits")
        assert np.array_equal(V.run_argmax(logits, offs), O.argmax(logits)), f"argmax {(B, C)} {offs}"
    elif what == "layout":
        B, C = int(g.integers(1, 6)), int(g.choice([1, 2, 3, 4, 5, 8, 31, 32, 64, 100]))
        H, W = int(g.integers(1, 30)), int(g.integers(1, 30))
        x = g.standard_normal((B, C, H, W), dtype=np.float32)
        nhwc = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
        offs, which = offs_for(g, "src", "dst"), str(g.choice(["plain", "back", "pad", "pad0"]))
        if which == "plain":
            same(V.run_transpose("rn_nchw_to_nhwc", x, nhwc.shape, x.shape, offs), nhwc, f"nchw_to_nhwc {x.shape} {offs}")
        elif which == "back":
            same(V.run_transpose("rn_nhwc_to_nchw", nhwc, x.shape, x.shape, offs), x, f"nhwc_to_nchw {x.shape} {offs}")
        elif which == "pad0":   # rn_nchw_to_nhwc_pad itself (no border, fp32)
            Cpad = int(g.choice([C, C + 1, max(C, 4), ((C + 3) // 4) * 4]))
            same(V.run_pad(x, Cpad, 0, offs, False), V.pad_reference(x, Cpad, 0), f"pad {x.shape} Cpad={Cpad} {offs}")
        else:
            Cpad, border = int(g.choice([C, C + 1, max(C, 4), ((C + 3) // 4) * 4])), int(g.integers(0, 4))
            same(V.run_pad(x, Cpad, border, offs, True), V.pad_reference(x, Cpad, border),
                 f"pad_dt {x.shape} Cpad={Cpad} border={border} {offs}")
    else:
        nel = int(g.choice([1, 3, 4, 5, 63, 64, 1000, 4097, 70001]))
        x, y = g.standard_normal(nel, dtype=np.float32), g.standard_normal(nel, dtype=np.float32)
        inplace = bool(g.integers(0, 2))
        o1, o2 = offs_for(g, "inp", "out"), offs_for(g, "inp1", "inp2", "out")
        same(V.run_relu(x, o1, inplace), O.relu(x), f"relu n={nel} inplace={inplace} {o1}")
        same(V.run_add(x, y, o2, inplace), O.add(x, y), f"add n={nel} inplace={inplace} {o2}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    g = np.random.default_rng(a.seed)
    t0, n = time.time(), {"maxpool": 0, "avgpool": 0, "batchnorm": 0, "linear": 0, "conv2d": 0, "conv_nhwc": 0, "argmax": 0, "relu/add": 0, "layout": 0}
    while time.time() - t0 < a.seconds:
        what = str(g.choice(list(n)))
        one_case(g, what)
        n[what] += 1
    print(f"view_fuzz: {n}, seed {a.seed}: every view gave the expected bits, all guards clean")


if __name__ == "__main__":
    main()
