"""Functional forms of the seven reference ops on host arrays.

Each function uploads its NCHW numpy operands, makes ONE call into the C-ABI
entry point that replaces the reference kernel (include/rn_hip.h), and
downloads the result.  They exist for tests, notebooks and small tools; the
throughput path is ``model.NativeModel``.  ``layout`` selects how the device
side holds activations: "nchw" (what the reference kernels see) or "nhwc" (the
engine layout; arrays are transposed on the host around the call).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib as L
from .tensor import Device, FloatTensor, get_ctx

_LAYOUT = {"nchw": L.RN_LAYOUT_NCHW, "nhwc": L.RN_LAYOUT_NHWC}


def _up(a: np.ndarray, layout: str) -> FloatTensor:
    a = np.asarray(a, dtype=np.float32)
    if layout == "nhwc" and a.ndim == 4:
        a = a.transpose(0, 2, 3, 1)
    return FloatTensor.from_numpy(a, Device.GPU)


def _down(t: FloatTensor, shape_nchw, layout: str) -> np.ndarray:
    flat = t.cpu()._storage
    if layout == "nhwc" and len(shape_nchw) == 4:
        B, C, H, W = shape_nchw
        return flat.reshape(B, H, W, C).transpose(0, 3, 1, 2).copy()
    return flat.reshape(shape_nchw).copy()


def _run(name: str, layout: str, *args) -> None:
    ctx = get_ctx()
    ctx.set_layout(_LAYOUT[layout])
    L.check(getattr(L.lib(), name)(ctx.handle, *args), name, ctx.handle)
    ctx.sync()


def conv_output_size(x: int, k: int, stride: int, pad: int) -> int:
    return int(L.lib().rn_conv_output_size(x, k, stride, pad))


def conv2d(x, w, stride: int = 1, pad: int = 0, layout: str = "nchw") -> np.ndarray:
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    ho, wo = conv_output_size(H, k, stride, pad), conv_output_size(W, k, stride, pad)
    dx, dw = _up(x, layout), _up(w, "nchw")
    out = FloatTensor((B, Cout, ho, wo), Device.GPU)
    _run("rn_conv2d_forward", layout, dx.data(), out.data(), dw.data(), k, stride, pad, ho, wo, B,
         Cin, Cout, H, W)
    return _down(out, (B, Cout, ho, wo), layout)


def _pool(name, x, k, stride, pad, layout):
    B, C, H, W = x.shape
    ho, wo = conv_output_size(H, k, stride, pad), conv_output_size(W, k, stride, pad)
    dx = _up(x, layout)
    out = FloatTensor((B, C, ho, wo), Device.GPU)
    _run(name, layout, dx.data(), out.data(), k, stride, pad, ho, wo, B, C, H, W)
    return _down(out, (B, C, ho, wo), layout)


def maxpool2d(x, k, stride=1, pad=0, layout="nchw"):
    return _pool("rn_maxpool2d_forward", x, k, stride, pad, layout)


def avgpool2d(x, k, stride=1, pad=0, layout="nchw"):
    return _pool("rn_avgpool2d_forward", x, k, stride, pad, layout)


def linear(x, w, b: Optional[np.ndarray]) -> np.ndarray:
    B, fin = x.shape
    fout = w.shape[0]
    dx, dw = _up(x, "nchw"), _up(w, "nchw")
    db = None if b is None else _up(b, "nchw")
    out = FloatTensor((B, fout), Device.GPU)
    _run("rn_linear_forward", "nchw", dx.data(), out.data(), dw.data(),
         None if db is None else db.data(), B, fin, fout)
    return _down(out, (B, fout), "nchw")


def relu(x, inplace: bool = True) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    dx = _up(x.reshape(-1), "nchw")
    out = dx if inplace else FloatTensor((x.size,), Device.GPU)
    _run("rn_relu_forward", "nchw", dx.data(), out.data(), x.size)
    return _down(out, x.shape, "nchw")


def add(a, b, inplace: bool = True) -> np.ndarray:
    a = np.asarray(a, dtype=np.float32)
    da, db = _up(a.reshape(-1), "nchw"), _up(np.asarray(b).reshape(-1), "nchw")
    out = da if inplace else FloatTensor((a.size,), Device.GPU)
    _run("rn_add_forward", "nchw", da.data(), db.data(), out.data(), a.size)
    return _down(out, a.shape, "nchw")


def batchnorm2d(x, w, b, mean, var, layout: str = "nchw", inplace: bool = True) -> np.ndarray:
    B, C = x.shape[0], x.shape[1]
    N = int(np.prod(x.shape[2:]))
    dx = _up(x, layout)
    out = dx if inplace else FloatTensor(x.shape, Device.GPU)
    p = [_up(v, "nchw") for v in (w, b, mean, var)]
    _run("rn_batchnorm2d_forward", layout, dx.data(), out.data(), *(t.data() for t in p), B, C, N)
    return _down(out, x.shape, layout)


def argmax(logits) -> np.ndarray:
    logits = np.asarray(logits, dtype=np.float32)
    B, C = logits.shape
    dl = _up(logits, "nchw")
    idx = FloatTensor((2 * B,), Device.GPU)  # B uint64 slots
    _run("rn_argmax_forward", "nchw", dl.data(), idx.data(), B, C)
    raw = idx.cpu()._storage
    return raw.view(np.uint64).astype(np.int64)


def topk_reference(x, k: int):
    """The contract of rn_topk_forward in numpy, for rows without NaN: the k largest, descending, equal
    values (-0.0 == +0.0 among them) in ascending index order -- a stable argsort of -x."""
    x = np.asarray(x, dtype=np.float32)
    idx = np.argsort(-x, axis=-1, kind="stable")[..., :k]
    return np.take_along_axis(x, idx, axis=-1), idx.astype(np.int64)


def softmax_reference(x) -> np.ndarray:
    """float64 softmax of the fp32 rows (what rn_softmax_forward is measured against)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def softmax(x) -> np.ndarray:
    """rn_softmax_forward on host rows [B, classes]."""
    x = np.asarray(x, dtype=np.float32)
    B, C = x.shape
    dx = _up(x, "nchw")
    out = FloatTensor((B, C), Device.GPU)
    _run("rn_softmax_forward", "nchw", dx.data(), out.data(), B, C)
    return _down(out, (B, C), "nchw")


def _topk_call(name: str, x, k: int, want_probs: bool):
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    x = np.asarray(x, dtype=np.float32)
    B, C = x.shape
    dx = _up(x, "nchw")
    val = FloatTensor((B, k), Device.GPU)
    idx = _DeviceBuffer(ctx, max(B * k * 8, 16))
    probs = FloatTensor((B, C), Device.GPU) if want_probs else None
    if name == "rn_topk_forward":
        _run(name, "nchw", dx.data(), val.data(), idx.ptr, B, C, k)
    else:
        _run(name, "nchw", dx.data(), probs.data() if probs else None, val.data(), idx.ptr, B, C, k)
    hi = _down_raw(idx, np.uint64, B * k).astype(np.int64).reshape(B, k)
    return _down(val, (B, k), "nchw"), hi, (_down(probs, (B, C), "nchw") if probs else None)


def topk(x, k: int):
    """rn_topk_forward: (values [B,k], indices [B,k] int64), descending, ties by ascending index."""
    v, i, _ = _topk_call("rn_topk_forward", x, k, False)
    return v, i


def softmax_topk(x, k: int, return_probs: bool = False):
    """rn_softmax_topk_forward: (topk_prob [B,k], topk_idx [B,k]) ordered by logit, and with ``return_probs``
    the full probabilities [B, classes] as a third element, all from one launch."""
    v, i, p = _topk_call("rn_softmax_topk_forward", x, k, return_probs)
    return (v, i, p) if return_probs else (v, i)


def conv2d_nhwc_fused(x, w, stride=1, pad=0, scale=None, shift=None, residual=None,
                      relu_: bool = False) -> np.ndarray:
    """rn_conv2d_pack_weight + rn_conv2d_nhwc_forward with an epilogue (NCHW host arrays)."""
    ctx = get_ctx()
    lib = L.lib()
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    ho, wo = conv_output_size(H, k, stride, pad), conv_output_size(W, k, stride, pad)
    cs = int(lib.rn_conv2d_input_channels(Cin))
    xp = np.zeros((B, H, W, cs), dtype=np.float32)
    xp[..., :Cin] = np.asarray(x, dtype=np.float32).transpose(0, 2, 3, 1)
    dx = FloatTensor.from_numpy(xp, Device.GPU)
    dw = _up(w, "nchw")
    packed = FloatTensor((int(lib.rn_conv2d_packed_weight_numel(Cin, Cout, k)),), Device.GPU)
    L.check(lib.rn_conv2d_pack_weight(ctx.handle, dw.data(), packed.data(), Cin, Cout, k),
            "rn_conv2d_pack_weight", ctx.handle)
    keep = [_up(v, "nchw") if v is not None else None for v in (scale, shift)]
    dres = _up(residual, "nhwc") if residual is not None else None
    ep = L.Epilogue(keep[0].data() if keep[0] else None, keep[1].data() if keep[1] else None,
                    dres.data() if dres else None, int(relu_))
    out = FloatTensor((B, Cout, ho, wo), Device.GPU)
    L.check(lib.rn_conv2d_nhwc_forward(ctx.handle, dx.data(), out.data(), packed.data(), k, stride,
                                       pad, ho, wo, B, Cin, Cout, H, W, ctypes.byref(ep)),
            "rn_conv2d_nhwc_forward", ctx.handle)
    ctx.sync()
    return _down(out, (B, Cout, ho, wo), "nhwc")


def conv2d_nhwc_exact(x, w, stride=1, pad=0, scale=None, shift=None, residual=None,
                      relu_: bool = False) -> np.ndarray:
    """Small-Cin convolution in the exact-K form: rn_nchw_to_nhwc_pad_dt (physical border) +
    rn_conv2d_pack_weight_exact + rn_conv2d_nhwc_exact_forward.  NCHW fp32 host arrays."""
    ctx, lib = get_ctx(), L.lib()
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    Hp, Wp = H + 2 * pad, W + 2 * pad
    ho, wo = conv_output_size(Hp, k, stride, 0), conv_output_size(Wp, k, stride, 0)
    dx32 = _up(np.asarray(x, dtype=np.float32), "nchw")
    dx = FloatTensor((B, Hp, Wp, Cin), Device.GPU)
    L.check(lib.rn_nchw_to_nhwc_pad_dt(ctx.handle, L.RN_DTYPE_F32, dx32.data(), dx.data(), B, Cin,
                                       H, W, Cin, pad), "rn_nchw_to_nhwc_pad_dt", ctx.handle)
    dw = _up(w, "nchw")
    packed = FloatTensor((int(lib.rn_conv2d_packed_weight_numel_exact(Cin, Cout, k)),), Device.GPU)
    L.check(lib.rn_conv2d_pack_weight_exact(ctx.handle, dw.data(), packed.data(), Cin, Cout, k),
            "rn_conv2d_pack_weight_exact", ctx.handle)
    keep = [_up(v, "nchw") if v is not None else None for v in (scale, shift)]
    dres = _up(residual, "nhwc") if residual is not None else None
    ep = L.Epilogue(keep[0].data() if keep[0] else None, keep[1].data() if keep[1] else None,
                    dres.data() if dres else None, int(relu_))
    out = FloatTensor((B, Cout, ho, wo), Device.GPU)
    L.check(lib.rn_conv2d_nhwc_exact_forward(ctx.handle, dx.data(), out.data(), packed.data(), k,
                                             stride, ho, wo, B, Cin, Cout, Hp, Wp, ctypes.byref(ep)),
            "rn_conv2d_nhwc_exact_forward", ctx.handle)
    ctx.sync()
    return _down(out, (B, Cout, ho, wo), "nhwc")


# ---------------------------------------------------------------------------
# bf16 storage (element-type tagged entry points)
# ---------------------------------------------------------------------------
def to_bf16_bits(a) -> np.ndarray:
    """fp32 -> bf16 bit patterns (uint16), round to nearest even (what v_cvt_pk_bf16_f32 does)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def from_bf16_bits(b) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_round(a) -> np.ndarray:
    """fp32 values rounded to the nearest bf16, still stored as fp32."""
    return from_bf16_bits(to_bf16_bits(a)).reshape(np.shape(a))


def _up_raw(arr: np.ndarray):
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    arr = np.ascontiguousarray(arr)
    buf = _DeviceBuffer(ctx, max(arr.nbytes, 16))
    L.check(L.lib().rn_memcpy_h2d(ctx.handle, buf.ptr, arr.ctypes.data, arr.nbytes), "h2d", ctx.handle)
    return buf


def _down_raw(buf, dtype, count: int) -> np.ndarray:
    ctx = get_ctx()
    out = np.empty(count, dtype=dtype)
    L.check(L.lib().rn_memcpy_d2h(ctx.handle, out.ctypes.data, buf.ptr, out.nbytes), "d2h", ctx.handle)
    return out


def conv2d_nhwc_bf16(x, w, stride=1, pad=0, scale=None, shift=None, residual=None,
                     relu_: bool = False, out_f32: bool = False) -> np.ndarray:
    """bf16 activations/weights through rn_conv2d_pack_weight_dt + rn_conv2d_nhwc_forward_dt.
    NCHW fp32 host arrays in (rounded to bf16 on upload), NCHW fp32 host array out.  The
    small-Cin stem form gets a physically zero-padded image, as the model driver builds it."""
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    ho, wo = conv_output_size(H, k, stride, pad), conv_output_size(W, k, stride, pad)
    c4 = Cin <= 4 and k <= 8
    dx32 = _up(np.asarray(x, dtype=np.float32), "nchw")
    if c4:
        Hp, Wp = H + 2 * pad, W + 2 * pad
        dx = _DeviceBuffer(ctx, B * Hp * Wp * 4 * 2)
        L.check(lib.rn_nchw_to_nhwc_pad_dt(ctx.handle, L.RN_DTYPE_BF16, dx32.data(), dx.ptr, B, Cin,
                                           H, W, 4, pad), "pad_dt", ctx.handle)
        Hin, Win, pad_arg = Hp, Wp, 0
    else:
        dx = _up_raw(to_bf16_bits(np.asarray(x, dtype=np.float32).transpose(0, 2, 3, 1)))
        Hin, Win, pad_arg = H, W, pad
    dw = _up(w, "nchw")
    pn = int(lib.rn_conv2d_packed_weight_numel_dt(L.RN_DTYPE_BF16, Cin, Cout, k))
    packed = _DeviceBuffer(ctx, pn * 2)
    L.check(lib.rn_conv2d_pack_weight_dt(ctx.handle, L.RN_DTYPE_BF16, dw.data(), packed.ptr, Cin,
                                         Cout, k), "pack_dt", ctx.handle)
    keep = [_up(v, "nchw") if v is not None else None for v in (scale, shift)]
    dres = None
    if residual is not None:
        r = np.asarray(residual, dtype=np.float32).transpose(0, 2, 3, 1)
        dres = _up_raw(r if out_f32 else to_bf16_bits(r))
    ep = L.Epilogue(keep[0].data() if keep[0] else None, keep[1].data() if keep[1] else None,
                    dres.ptr if dres else None, int(relu_))
    n_out = B * Cout * ho * wo
    out = _DeviceBuffer(ctx, n_out * (4 if out_f32 else 2))
    L.check(lib.rn_conv2d_nhwc_forward_dt(ctx.handle, L.RN_DTYPE_BF16,
                                          L.RN_DTYPE_F32 if out_f32 else L.RN_DTYPE_BF16, dx.ptr,
                                          out.ptr, packed.ptr, k, stride, pad_arg, ho, wo, B, Cin,
                                          Cout, Hin, Win, ctypes.byref(ep)),
            "rn_conv2d_nhwc_forward_dt", ctx.handle)
    ctx.sync()
    if out_f32:
        y = _down_raw(out, np.float32, n_out)
    else:
        y = from_bf16_bits(_down_raw(out, np.uint16, n_out))
    return y.reshape(B, ho, wo, Cout).transpose(0, 3, 1, 2).copy()


def conv_chain_bf16(t2, x, w3, scale3, shift3, w1, scale1, shift1):
    """rn_conv_chain_forward_dt: relu(bn3(conv1x1(t2, w3)) + x) -> y and relu(bn1(conv1x1(y, w1)))
    -> t1 as one launch (bf16 storage).  NCHW fp32 host arrays in (rounded to bf16 on upload);
    returns (y, t1) as NCHW fp32 host arrays."""
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    B, Cm, H, W = t2.shape
    C, N1 = w3.shape[0], w1.shape[0]
    rows = B * H * W

    def up_act(a):
        return _up_raw(to_bf16_bits(np.asarray(a, dtype=np.float32).transpose(0, 2, 3, 1)))

    def pack(w, cin, cout):
        dw = _up(w, "nchw")
        pk = _DeviceBuffer(ctx, int(lib.rn_conv2d_packed_weight_numel_dt(L.RN_DTYPE_BF16, cin, cout, 1)) * 2)
        L.check(lib.rn_conv2d_pack_weight_dt(ctx.handle, L.RN_DTYPE_BF16, dw.data(), pk.ptr, cin, cout, 1),
                "pack_dt", ctx.handle)
        return pk

    dt2, dx = up_act(t2), up_act(x)
    p3, p1 = pack(w3, Cm, C), pack(w1, C, N1)
    keep = [_up(np.asarray(v, dtype=np.float32), "nchw") if v is not None else None
            for v in (scale3, shift3, scale1, shift1)]
    ptr = [k.data() if k else None for k in keep]
    y, t1 = _DeviceBuffer(ctx, rows * C * 2), _DeviceBuffer(ctx, rows * N1 * 2)
    L.check(lib.rn_conv_chain_forward_dt(ctx.handle, L.RN_DTYPE_BF16, dt2.ptr, dx.ptr, y.ptr, p3.ptr, ptr[0],
                                         ptr[1], t1.ptr, p1.ptr, ptr[2], ptr[3], rows, Cm, C, N1),
            "rn_conv_chain_forward_dt", ctx.handle)
    ctx.sync()
    yh = from_bf16_bits(_down_raw(y, np.uint16, rows * C)).reshape(B, H, W, C).transpose(0, 3, 1, 2).copy()
    th = from_bf16_bits(_down_raw(t1, np.uint16, rows * N1)).reshape(B, H, W, N1).transpose(0, 3, 1, 2).copy()
    return yh, th


def conv_chain_f32(t2, x, w3, scale3, shift3, w1, scale1, shift1):
    """rn_conv_chain_forward_dt with fp32 storage (64 -> 256 -> 64 | 128 channels): (y, t1) as NCHW
    fp32 host arrays."""
    ctx, lib = get_ctx(), L.lib()
    B, Cm, H, W = t2.shape
    C, N1 = w3.shape[0], w1.shape[0]
    rows = B * H * W

    def pack(w, cin, cout):
        dw = _up(w, "nchw")
        pk = FloatTensor((int(lib.rn_conv2d_packed_weight_numel(cin, cout, 1)),), Device.GPU)
        L.check(lib.rn_conv2d_pack_weight(ctx.handle, dw.data(), pk.data(), cin, cout, 1), "pack", ctx.handle)
        return pk

    dt2, dx = _up(np.asarray(t2, dtype=np.float32), "nhwc"), _up(np.asarray(x, dtype=np.float32), "nhwc")
    p3, p1 = pack(w3, Cm, C), pack(w1, C, N1)
    keep = [_up(np.asarray(v, dtype=np.float32), "nchw") if v is not None else None
            for v in (scale3, shift3, scale1, shift1)]
    ptr = [k.data() if k else None for k in keep]
    y, t1 = FloatTensor((B, C, H, W), Device.GPU), FloatTensor((B, N1, H, W), Device.GPU)
    L.check(lib.rn_conv_chain_forward_dt(ctx.handle, L.RN_DTYPE_F32, dt2.data(), dx.data(), y.data(), p3.data(),
                                         ptr[0], ptr[1], t1.data(), p1.data(), ptr[2], ptr[3], rows, Cm, C, N1),
            "rn_conv_chain_forward_dt", ctx.handle)
    ctx.sync()
    return _down(y, (B, C, H, W), "nhwc"), _down(t1, (B, N1, H, W), "nhwc")


def conv_chain_pair(t2, x2, w3, scale3, wd, scaled, shift, w1, scale1, shift1, bf16: bool = True):
    """rn_conv_chain_pair_forward_dt: relu(conv1x1(t2, w3*scale3) + conv1x1(x2, wd*scaled) + shift) -> y
    and relu(bn1(conv1x1(y, w1))) -> t1 as one launch.  NCHW fp32 host arrays; returns (y, t1)."""
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    B, Cm, H, W = t2.shape
    C, C2, N1 = w3.shape[0], x2.shape[1], w1.shape[0]
    rows = B * H * W
    dt, es = (L.RN_DTYPE_BF16, 2) if bf16 else (L.RN_DTYPE_F32, 4)

    def up_act(a):
        a = np.asarray(a, dtype=np.float32).transpose(0, 2, 3, 1)
        return _up_raw(to_bf16_bits(a) if bf16 else a)

    dt2, dx2 = up_act(t2), up_act(x2)
    dw3, dwd, dw1 = _up(w3, "nchw"), _up(wd, "nchw"), _up(w1, "nchw")
    keep = [_up(np.asarray(v, dtype=np.float32), "nchw") if v is not None else None
            for v in (scale3, scaled, shift, scale1, shift1)]
    ptr = [k.data() if k else None for k in keep]
    pp = _DeviceBuffer(ctx, int(lib.rn_conv2d_packed_pair_weight_numel(Cm, C, 1, C2)) * es)
    L.check(lib.rn_conv2d_pack_weight_pair_dt(ctx.handle, dt, dw3.data(), ptr[0], dwd.data(), ptr[1],
                                              pp.ptr, Cm, C, 1, C2), "pack_pair", ctx.handle)
    p1 = _DeviceBuffer(ctx, int(lib.rn_conv2d_packed_weight_numel_dt(dt, C, N1, 1)) * es)
    L.check(lib.rn_conv2d_pack_weight_dt(ctx.handle, dt, dw1.data(), p1.ptr, C, N1, 1), "pack_dt", ctx.handle)
    y, t1 = _DeviceBuffer(ctx, rows * C * es), _DeviceBuffer(ctx, rows * N1 * es)
    L.check(lib.rn_conv_chain_pair_forward_dt(ctx.handle, dt, dt2.ptr, dx2.ptr, y.ptr, pp.ptr, ptr[2],
                                              t1.ptr, p1.ptr, ptr[3], ptr[4], rows, Cm, C2, C, N1),
            "rn_conv_chain_pair_forward_dt", ctx.handle)
    ctx.sync()

    def down(b, n, c):
        h = from_bf16_bits(_down_raw(b, np.uint16, n)) if bf16 else _down_raw(b, np.float32, n)
        return h.reshape(B, H, W, c).transpose(0, 3, 1, 2).copy()

    return down(y, rows * C, C), down(t1, rows * N1, N1)


def conv_chain_pair_bf16(*a):
    return conv_chain_pair(*a, bf16=True)


def conv2d_nhwc_pair(x, w, x2, w2, stride=1, pad=0, stride2=1, scale=None, scale2=None, shift=None,
                     residual=None, relu_: bool = False, bf16: bool = False) -> np.ndarray:
    """epilogue(conv(x, w * scale) + conv1x1(x2, w2 * scale2)) as ONE contraction:
    rn_conv2d_pack_weight_pair_dt + rn_conv2d_nhwc_pair_forward_dt.  NCHW fp32 host arrays."""
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    _, Cin2, H2, W2 = x2.shape
    ho, wo = conv_output_size(H, k, stride, pad), conv_output_size(W, k, stride, pad)
    dt, es = (L.RN_DTYPE_BF16, 2) if bf16 else (L.RN_DTYPE_F32, 4)

    def up_act(a):
        a = np.asarray(a, dtype=np.float32).transpose(0, 2, 3, 1)
        return _up_raw(to_bf16_bits(a) if bf16 else a)

    dx, dx2 = up_act(x), up_act(x2)
    dw, dw2 = _up(w, "nchw"), _up(w2, "nchw")
    keep = [_up(v, "nchw") if v is not None else None for v in (scale, scale2, shift)]
    pn = int(lib.rn_conv2d_packed_pair_weight_numel(Cin, Cout, k, Cin2))
    packed = _DeviceBuffer(ctx, pn * es)
    L.check(lib.rn_conv2d_pack_weight_pair_dt(ctx.handle, dt, dw.data(),
                                              keep[0].data() if keep[0] else None, dw2.data(),
                                              keep[1].data() if keep[1] else None, packed.ptr, Cin,
                                              Cout, k, Cin2), "pack_pair", ctx.handle)
    dres = up_act(residual) if residual is not None else None
    ep = L.Epilogue(None, keep[2].data() if keep[2] else None, dres.ptr if dres else None,
                    int(relu_))
    second = L.ConvSecond(dx2.ptr, Cin2, H2, W2, stride2)
    n_out = B * Cout * ho * wo
    out = _DeviceBuffer(ctx, n_out * es)
    L.check(lib.rn_conv2d_nhwc_pair_forward_dt(ctx.handle, dt, dt, dx.ptr, out.ptr, packed.ptr, k,
                                               stride, pad, ho, wo, B, Cin, Cout, H, W,
                                               ctypes.byref(second), ctypes.byref(ep)),
            "rn_conv2d_nhwc_pair_forward_dt", ctx.handle)
    ctx.sync()
    y = from_bf16_bits(_down_raw(out, np.uint16, n_out)) if bf16 else _down_raw(out, np.float32, n_out)
    return y.reshape(B, ho, wo, Cout).transpose(0, 3, 1, 2).copy()


def pool_nhwc_bf16(x, k, stride=1, pad=0, is_max=True) -> np.ndarray:
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    B, C, H, W = x.shape
    ho, wo = conv_output_size(H, k, stride, pad), conv_output_size(W, k, stride, pad)
    dx = _up_raw(to_bf16_bits(np.asarray(x, dtype=np.float32).transpose(0, 2, 3, 1)))
    out = _DeviceBuffer(ctx, B * C * ho * wo * 2)
    fn = lib.rn_maxpool2d_nhwc_forward_dt if is_max else lib.rn_avgpool2d_nhwc_forward_dt
    L.check(fn(ctx.handle, L.RN_DTYPE_BF16, dx.ptr, out.ptr, k, stride, pad, ho, wo, B, C, H, W),
            "pool_dt", ctx.handle)
    ctx.sync()
    y = from_bf16_bits(_down_raw(out, np.uint16, B * C * ho * wo))
    return y.reshape(B, ho, wo, C).transpose(0, 3, 1, 2).copy()


def global_avgpool(x, bf16: bool = False) -> np.ndarray:
    """Mean over the whole H x W map (rn_global_avgpool_nhwc_forward_dt): NCHW fp32 host array [B,C,H,W] in
    (uploaded as NHWC, rounded to bf16 first when ``bf16``), [B,C] fp32 out (bf16 results widened, exact).
    C % 4 == 0 (bf16: % 8).  The summation order depends on (H, W) only; 7 x 7 gives the bits of
    avgpool2d(k=7) on NHWC."""
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    x = np.asarray(x, dtype=np.float32)
    B, C, H, W = x.shape
    nhwc = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    dx = _up_raw(to_bf16_bits(nhwc) if bf16 else nhwc)
    out = _DeviceBuffer(ctx, max(B * C * (2 if bf16 else 4), 16))
    L.check(L.lib().rn_global_avgpool_nhwc_forward_dt(ctx.handle, L.RN_DTYPE_BF16 if bf16 else L.RN_DTYPE_F32,
                                                      dx.ptr, out.ptr, B, C, H, W),
            "rn_global_avgpool_nhwc_forward_dt", ctx.handle)
    ctx.sync()
    y = from_bf16_bits(_down_raw(out, np.uint16, B * C)) if bf16 else _down_raw(out, np.float32, B * C)
    return y.reshape(B, C)


def nhwc_to_nchw_dt(x, bf16: bool = False) -> np.ndarray:
    """rn_nhwc_to_nchw_dt: NHWC host array [B,H,W,C] in -- fp32, or uint16 bf16 bit patterns (``bf16``; an fp32
    array is rounded to bf16 first) -- NCHW fp32 [B,C,H,W] out, bf16 widened exactly.  Any C, H, W; the fast
    form where C % 4 == 0 (bf16: % 8)."""
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    x = np.asarray(x)
    if bf16:
        x = x if x.dtype == np.uint16 else to_bf16_bits(x).reshape(x.shape)
    else:
        x = x.astype(np.float32, copy=False)
    B, H, W, C = x.shape
    dx = _up_raw(x)
    out = _DeviceBuffer(ctx, max(x.size * 4, 16))
    L.check(L.lib().rn_nhwc_to_nchw_dt(ctx.handle, L.RN_DTYPE_BF16 if bf16 else L.RN_DTYPE_F32, dx.ptr, out.ptr,
                                       B, C, H, W), "rn_nhwc_to_nchw_dt", ctx.handle)
    ctx.sync()
    return _down_raw(out, np.float32, x.size).reshape(B, C, H, W)


def image_u8_to_nhwc_pad(px, cpad: int = 4, border: int = 0, bf16: bool = False, mean=None, std=None,
                         prefill: Optional[int] = None) -> np.ndarray:
    """rn_image_u8_to_nhwc_pad_dt: uint8 RGB [B,H,W,3] -> the normalised, padded first tensor
    [B,H+2b,W+2b,cpad] as the device wrote it: fp32, or for ``bf16`` the raw bf16 bits (uint16).
    ``mean`` / ``std`` default to the ImageNet values of preprocess.py; ``prefill`` fills the
    destination with that byte first, so that an element the launch did not write shows."""
    from . import preprocess
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    px = np.ascontiguousarray(px, dtype=np.uint8)
    B, H, W, C = px.shape
    assert C == 3
    dt, es, ht = (L.RN_DTYPE_BF16, 2, np.uint16) if bf16 else (L.RN_DTYPE_F32, 4, np.float32)
    n = B * (H + 2 * border) * (W + 2 * border) * cpad
    src = _up_raw(px)
    dst = _DeviceBuffer(ctx, max(n * es, 16))
    if prefill is not None:
        L.check(lib.rn_memset(ctx.handle, dst.ptr, prefill, max(n * es, 16)), "memset", ctx.handle)
    m3 = (ctypes.c_float * 3)(*(preprocess.MEAN if mean is None else mean))
    s3 = (ctypes.c_float * 3)(*(preprocess.STD if std is None else std))
    L.check(lib.rn_image_u8_to_nhwc_pad_dt(ctx.handle, dt, src.ptr, dst.ptr, B, H, W, cpad, border, m3, s3),
            "rn_image_u8_to_nhwc_pad_dt", ctx.handle)
    return _down_raw(dst, ht, n).reshape(B, H + 2 * border, W + 2 * border, cpad)


def pack_images(images):
    """A list of [H,W,3] uint8 arrays -> (packed bytes back to back, offsets, heights, widths as uint64)."""
    imgs = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
    for a in imgs:
        assert a.ndim == 3 and a.shape[2] == 3, a.shape
    sizes = np.array([a.size for a in imgs], dtype=np.uint64)
    offsets = np.concatenate([np.zeros(1, np.uint64), np.cumsum(sizes)[:-1]]).astype(np.uint64) if imgs \
        else np.zeros(0, np.uint64)
    packed = np.concatenate([a.reshape(-1) for a in imgs]) if imgs else np.zeros(0, np.uint8)
    heights = np.array([a.shape[0] for a in imgs], dtype=np.uint64)
    widths = np.array([a.shape[1] for a in imgs], dtype=np.uint64)
    return packed, offsets, heights, widths


def _u64p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def image_u8_resize_crop(images, resize: int = 256, crop: int = 224) -> np.ndarray:
    """rn_image_u8_resize_crop: a list of [H,W,3] uint8 RGB arrays of any sizes -> [B,crop,crop,3] uint8,
    PIL's antialiased bilinear resize (short side ``resize``) and centre crop, on the device."""
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    packed, offsets, heights, widths = pack_images(images)
    B = len(heights)
    n = B * crop * crop * 3
    src = _up_raw(packed)
    dst = _DeviceBuffer(ctx, max(n, 16))
    L.check(lib.rn_image_u8_resize_crop(ctx.handle, src.ptr, _u64p(offsets), _u64p(heights), _u64p(widths), B,
                                        dst.ptr, resize, crop), "rn_image_u8_resize_crop", ctx.handle)
    ctx.sync()
    return _down_raw(dst, np.uint8, n).reshape(B, crop, crop, 3)


def stem_pool(x, w, scale=None, shift=None, relu_: bool = True, bf16: bool = False,
              from_nchw: bool = False) -> np.ndarray:
    """conv 7x7/2 pad 3 + per-channel affine + ReLU + max-pool 3x3/2/1 through the fused launch
    (rn_stem_pool_pack_weight_dt + rn_nchw_to_nhwc_pad_dt + rn_stem_pool_forward_dt, or with
    ``from_nchw`` rn_stem_pool_nchw_forward_dt on the NCHW image itself).  NCHW fp32 host arrays
    in, NCHW fp32 host array [B,64,PH,PW] out."""
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    B, Cin, H, W = x.shape
    assert w.shape == (64, Cin, 7, 7)
    dt, es, cpad = (L.RN_DTYPE_BF16, 2, 4) if bf16 else (L.RN_DTYPE_F32, 4, 3)
    Hp, Wp = H + 6, W + 6
    ho, wo = conv_output_size(Hp, 7, 2, 0), conv_output_size(Wp, 7, 2, 0)
    ph, pw = conv_output_size(ho, 3, 2, 1), conv_output_size(wo, 3, 2, 1)
    xin = FloatTensor.from_numpy(np.ascontiguousarray(x, dtype=np.float32), Device.GPU)
    if not from_nchw:
        xp = _DeviceBuffer(ctx, B * Hp * Wp * cpad * es)
        L.check(lib.rn_nchw_to_nhwc_pad_dt(ctx.handle, dt, xin.data(), xp.ptr, B, Cin, H, W, cpad, 3), "pad", ctx.handle)
    wd = FloatTensor.from_numpy(np.ascontiguousarray(w, dtype=np.float32), Device.GPU)
    wp = _DeviceBuffer(ctx, int(lib.rn_stem_pool_packed_weight_numel(dt)) * es)
    L.check(lib.rn_stem_pool_pack_weight_dt(ctx.handle, dt, wd.data(), wp.ptr, Cin), "pack", ctx.handle)
    sc = FloatTensor.from_numpy(np.asarray(scale, dtype=np.float32), Device.GPU) if scale is not None else None
    sh = FloatTensor.from_numpy(np.asarray(shift, dtype=np.float32), Device.GPU) if shift is not None else None
    out = _DeviceBuffer(ctx, B * ph * pw * 64 * es)
    if from_nchw:
        L.check(lib.rn_stem_pool_nchw_forward_dt(ctx.handle, dt, xin.data(), out.ptr, wp.ptr,
                                                 sc.data() if sc else None, sh.data() if sh else None,
                                                 int(relu_), B, Cin, H, W), "stem_pool_nchw", ctx.handle)
    else:
        L.check(lib.rn_stem_pool_forward_dt(ctx.handle, dt, xp.ptr, out.ptr, wp.ptr, sc.data() if sc else None,
                                            sh.data() if sh else None, int(relu_), B, Hp, Wp), "stem_pool", ctx.handle)
    host = np.empty(B * ph * pw * 64, dtype=np.uint16 if bf16 else np.float32)
    L.check(lib.rn_memcpy_d2h(ctx.handle, host.ctypes.data, out.ptr, host.nbytes), "d2h", ctx.handle)
    if bf16:
        host = (host.astype(np.uint32) << 16).view(np.float32)
    return np.ascontiguousarray(host.reshape(B, ph, pw, 64).transpose(0, 3, 1, 2))


def stem_conv_pool(x, w, scale=None, shift=None):
    """rn_stem_conv_pool_nchw_forward: the fused stem launch that also writes the stem tensor.  NCHW fp32 host
    arrays in; (stem [B,64,Ho,Wo], pooled [B,64,PH,PW]) NCHW fp32 host arrays out."""
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    B, Cin, H, W = x.shape
    assert w.shape == (64, Cin, 7, 7)
    ho, wo = conv_output_size(H + 6, 7, 2, 0), conv_output_size(W + 6, 7, 2, 0)
    ph, pw = conv_output_size(ho, 3, 2, 1), conv_output_size(wo, 3, 2, 1)
    xin = FloatTensor.from_numpy(np.ascontiguousarray(x, dtype=np.float32), Device.GPU)
    wd = FloatTensor.from_numpy(np.ascontiguousarray(w, dtype=np.float32), Device.GPU)
    wp = _DeviceBuffer(ctx, int(lib.rn_stem_pool_packed_weight_numel(L.RN_DTYPE_F32)) * 4)
    L.check(lib.rn_stem_pool_pack_weight_dt(ctx.handle, L.RN_DTYPE_F32, wd.data(), wp.ptr, Cin), "pack", ctx.handle)
    sc = FloatTensor.from_numpy(np.asarray(scale, dtype=np.float32), Device.GPU) if scale is not None else None
    sh = FloatTensor.from_numpy(np.asarray(shift, dtype=np.float32), Device.GPU) if shift is not None else None
    y, out = _DeviceBuffer(ctx, B * ho * wo * 64 * 4), _DeviceBuffer(ctx, B * ph * pw * 64 * 4)
    L.check(lib.rn_memset(ctx.handle, y.ptr, 0xFF, B * ho * wo * 64 * 4), "memset", ctx.handle)   # NaNs: every element must be written
    L.check(lib.rn_stem_conv_pool_nchw_forward(ctx.handle, xin.data(), y.ptr, out.ptr, wp.ptr, sc.data() if sc else None,
                                               sh.data() if sh else None, B, Cin, H, W), "stem_conv_pool", ctx.handle)
    hy, hp = np.empty(B * ho * wo * 64, dtype=np.float32), np.empty(B * ph * pw * 64, dtype=np.float32)
    L.check(lib.rn_memcpy_d2h(ctx.handle, hy.ctypes.data, y.ptr, hy.nbytes), "d2h", ctx.handle)
    L.check(lib.rn_memcpy_d2h(ctx.handle, hp.ctypes.data, out.ptr, hp.nbytes), "d2h", ctx.handle)
    return (np.ascontiguousarray(hy.reshape(B, ho, wo, 64).transpose(0, 3, 1, 2)),
            np.ascontiguousarray(hp.reshape(B, ph, pw, 64).transpose(0, 3, 1, 2)))


# ---------------------------------------------------------------------------
# grouped convolution (torch's ``groups``)
# ---------------------------------------------------------------------------
def conv2d_grouped(x, w, stride: int = 1, pad: int = 0, groups: int = 1, layout: str = "nchw") -> np.ndarray:
    """rn_conv2d_grouped_forward: w is [Cout, Cin / groups, k, k] (torch's layout)."""
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    ho, wo = conv_output_size(H, k, stride, pad), conv_output_size(W, k, stride, pad)
    dx, dw = _up(x, layout), _up(w, "nchw")
    out = FloatTensor((B, Cout, ho, wo), Device.GPU)
    _run("rn_conv2d_grouped_forward", layout, dx.data(), out.data(), dw.data(), k, stride, pad, ho, wo, B,
         Cin, Cout, H, W, groups)
    return _down(out, (B, Cout, ho, wo), layout)


def conv2d_grouped_nhwc(x, w, stride=1, pad=0, groups=1, scale=None, shift=None, residual=None,
                        relu_: bool = False) -> np.ndarray:
    """rn_conv2d_grouped_pack_weight_dt + rn_conv2d_grouped_nhwc_forward_dt in fp32, with an epilogue
    (NCHW host arrays)."""
    ctx, lib = get_ctx(), L.lib()
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    ho, wo = conv_output_size(H, k, stride, pad), conv_output_size(W, k, stride, pad)
    dx, dw = _up(x, "nhwc"), _up(w, "nchw")
    pn = int(lib.rn_conv2d_grouped_packed_weight_numel_dt(L.RN_DTYPE_F32, Cin, Cout, k, groups))
    packed = FloatTensor((max(pn, 1),), Device.GPU)
    L.check(lib.rn_conv2d_grouped_pack_weight_dt(ctx.handle, L.RN_DTYPE_F32, dw.data(), packed.data(), Cin, Cout,
                                                 k, groups), "rn_conv2d_grouped_pack_weight_dt", ctx.handle)
    keep = [_up(v, "nchw") if v is not None else None for v in (scale, shift)]
    dres = _up(residual, "nhwc") if residual is not None else None
    ep = L.Epilogue(keep[0].data() if keep[0] else None, keep[1].data() if keep[1] else None,
                    dres.data() if dres else None, int(relu_))
    out = FloatTensor((B, Cout, ho, wo), Device.GPU)
    L.check(lib.rn_conv2d_grouped_nhwc_forward_dt(ctx.handle, L.RN_DTYPE_F32, L.RN_DTYPE_F32, dx.data(), out.data(),
                                                  packed.data(), k, stride, pad, ho, wo, B, Cin, Cout, H, W, groups,
                                                  ctypes.byref(ep)),
            "rn_conv2d_grouped_nhwc_forward_dt", ctx.handle)
    ctx.sync()
    return _down(out, (B, Cout, ho, wo), "nhwc")


def conv2d_grouped_nhwc_bf16(x, w, stride=1, pad=0, groups=1, scale=None, shift=None, residual=None,
                             relu_: bool = False, out_f32: bool = False) -> np.ndarray:
    """The bf16 route of the grouped convolution (dense panel with zeros outside the groups).  NCHW fp32
    host arrays in (rounded to bf16 on upload), NCHW fp32 host array out."""
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    ho, wo = conv_output_size(H, k, stride, pad), conv_output_size(W, k, stride, pad)
    dx = _up_raw(to_bf16_bits(np.asarray(x, dtype=np.float32).transpose(0, 2, 3, 1)))
    dw = _up(w, "nchw")
    pn = int(lib.rn_conv2d_grouped_packed_weight_numel_dt(L.RN_DTYPE_BF16, Cin, Cout, k, groups))
    packed = _DeviceBuffer(ctx, max(pn, 8) * 2)
    L.check(lib.rn_conv2d_grouped_pack_weight_dt(ctx.handle, L.RN_DTYPE_BF16, dw.data(), packed.ptr, Cin, Cout, k,
                                                 groups), "rn_conv2d_grouped_pack_weight_dt", ctx.handle)
    keep = [_up(v, "nchw") if v is not None else None for v in (scale, shift)]
    dres = None
    if residual is not None:
        r = np.asarray(residual, dtype=np.float32).transpose(0, 2, 3, 1)
        dres = _up_raw(r if out_f32 else to_bf16_bits(r))
    ep = L.Epilogue(keep[0].data() if keep[0] else None, keep[1].data() if keep[1] else None,
                    dres.ptr if dres else None, int(relu_))
    n_out = B * Cout * ho * wo
    out = _DeviceBuffer(ctx, n_out * (4 if out_f32 else 2))
    L.check(lib.rn_conv2d_grouped_nhwc_forward_dt(ctx.handle, L.RN_DTYPE_BF16,
                                                  L.RN_DTYPE_F32 if out_f32 else L.RN_DTYPE_BF16, dx.ptr, out.ptr,
                                                  packed.ptr, k, stride, pad, ho, wo, B, Cin, Cout, H, W, groups,
                                                  ctypes.byref(ep)),
            "rn_conv2d_grouped_nhwc_forward_dt", ctx.handle)
    ctx.sync()
    y = _down_raw(out, np.float32, n_out) if out_f32 else from_bf16_bits(_down_raw(out, np.uint16, n_out))
    return y.reshape(B, ho, wo, Cout).transpose(0, 3, 1, 2).copy()


# ---------------------------------------------------------------------------
# dilated convolution (torch's ``dilation``, one factor for rows and columns)
# ---------------------------------------------------------------------------
def conv_output_size_dilated(x: int, k: int, stride: int, pad: int, dilation: int) -> int:
    return int(L.lib().rn_conv_output_size_dilated(x, k, stride, pad, dilation))


def conv2d_dilated(x, w, stride: int = 1, pad: int = 0, dilation: int = 1, groups: int = 1,
                   layout: str = "nchw") -> np.ndarray:
    """rn_conv2d_dilated_forward: w is [Cout, Cin / groups, k, k] (torch's layout)."""
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    ho, wo = (conv_output_size_dilated(n, k, stride, pad, dilation) for n in (H, W))
    dx, dw = _up(x, layout), _up(w, "nchw")
    out = FloatTensor((B, Cout, ho, wo), Device.GPU)
    _run("rn_conv2d_dilated_forward", layout, dx.data(), out.data(), dw.data(), k, stride, pad, dilation, ho, wo, B,
         Cin, Cout, H, W, groups)
    return _down(out, (B, Cout, ho, wo), layout)


def _pack_dt(dtype, dw, Cin, Cout, k, groups):
    """The panel the dilated NHWC entry point reads: the dense one for groups == 1, the grouped one above."""
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    es = 2 if dtype == L.RN_DTYPE_BF16 else 4
    if groups == 1:
        pn = int(lib.rn_conv2d_packed_weight_numel_dt(dtype, Cin, Cout, k))
        packed = _DeviceBuffer(ctx, max(pn, 8) * es)
        L.check(lib.rn_conv2d_pack_weight_dt(ctx.handle, dtype, dw.data(), packed.ptr, Cin, Cout, k),
                "rn_conv2d_pack_weight_dt", ctx.handle)
    else:
        pn = int(lib.rn_conv2d_grouped_packed_weight_numel_dt(dtype, Cin, Cout, k, groups))
        packed = _DeviceBuffer(ctx, max(pn, 8) * es)
        L.check(lib.rn_conv2d_grouped_pack_weight_dt(ctx.handle, dtype, dw.data(), packed.ptr, Cin, Cout, k, groups),
                "rn_conv2d_grouped_pack_weight_dt", ctx.handle)
    return packed


def conv2d_dilated_nhwc(x, w, stride=1, pad=0, dilation=1, groups=1, scale=None, shift=None, residual=None,
                        relu_: bool = False) -> np.ndarray:
    """rn_conv2d_pack_weight_dt / rn_conv2d_grouped_pack_weight_dt + rn_conv2d_dilated_nhwc_forward_dt in
    fp32, with an epilogue (NCHW host arrays; a small-Cin image is padded to its 4 channels)."""
    ctx, lib = get_ctx(), L.lib()
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    ho, wo = (conv_output_size_dilated(n, k, stride, pad, dilation) for n in (H, W))
    cs = int(lib.rn_conv2d_input_channels(Cin)) if groups == 1 else Cin
    xp = np.zeros((B, H, W, cs), dtype=np.float32)
    xp[..., :Cin] = np.asarray(x, dtype=np.float32).transpose(0, 2, 3, 1)
    dx, dw = FloatTensor.from_numpy(xp, Device.GPU), _up(w, "nchw")
    packed = _pack_dt(L.RN_DTYPE_F32, dw, Cin, Cout, k, groups)
    keep = [_up(v, "nchw") if v is not None else None for v in (scale, shift)]
    dres = _up(residual, "nhwc") if residual is not None else None
    ep = L.Epilogue(keep[0].data() if keep[0] else None, keep[1].data() if keep[1] else None,
                    dres.data() if dres else None, int(relu_))
    out = FloatTensor((B, Cout, ho, wo), Device.GPU)
    L.check(lib.rn_conv2d_dilated_nhwc_forward_dt(ctx.handle, L.RN_DTYPE_F32, L.RN_DTYPE_F32, dx.data(), out.data(),
                                                  packed.ptr, k, stride, pad, dilation, ho, wo, B, Cin, Cout, H, W,
                                                  groups, ctypes.byref(ep)),
            "rn_conv2d_dilated_nhwc_forward_dt", ctx.handle)
    ctx.sync()
    return _down(out, (B, Cout, ho, wo), "nhwc")


def conv2d_dilated_nhwc_bf16(x, w, stride=1, pad=0, dilation=1, groups=1, scale=None, shift=None, residual=None,
                             relu_: bool = False, out_f32: bool = False) -> np.ndarray:
    """The bf16 form of conv2d_dilated_nhwc (in_channels % 64 == 0).  NCHW fp32 host arrays in (rounded
    to bf16 on upload), NCHW fp32 host array out."""
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    ho, wo = (conv_output_size_dilated(n, k, stride, pad, dilation) for n in (H, W))
    dx = _up_raw(to_bf16_bits(np.asarray(x, dtype=np.float32).transpose(0, 2, 3, 1)))
    dw = _up(w, "nchw")
    packed = _pack_dt(L.RN_DTYPE_BF16, dw, Cin, Cout, k, groups)
    keep = [_up(v, "nchw") if v is not None else None for v in (scale, shift)]
    dres = None
    if residual is not None:
        r = np.asarray(residual, dtype=np.float32).transpose(0, 2, 3, 1)
        dres = _up_raw(r if out_f32 else to_bf16_bits(r))
    ep = L.Epilogue(keep[0].data() if keep[0] else None, keep[1].data() if keep[1] else None,
                    dres.ptr if dres else None, int(relu_))
    n_out = B * Cout * ho * wo
    out = _DeviceBuffer(ctx, max(n_out, 8) * (4 if out_f32 else 2))
    L.check(lib.rn_conv2d_dilated_nhwc_forward_dt(ctx.handle, L.RN_DTYPE_BF16,
                                                  L.RN_DTYPE_F32 if out_f32 else L.RN_DTYPE_BF16, dx.ptr, out.ptr,
                                                  packed.ptr, k, stride, pad, dilation, ho, wo, B, Cin, Cout, H, W,
                                                  groups, ctypes.byref(ep)),
            "rn_conv2d_dilated_nhwc_forward_dt", ctx.handle)
    ctx.sync()
    y = _down_raw(out, np.float32, n_out) if out_f32 else from_bf16_bits(_down_raw(out, np.uint16, n_out))
    return y.reshape(B, ho, wo, Cout).transpose(0, 3, 1, 2).copy()


def upsample_bilinear(x_nhwc, size, classes: Optional[int] = None, scores: bool = True, labels: bool = False):
    """rn_upsample_bilinear_forward: NHWC scores [B,h,w,C] fp32 (C % 4 == 0, C <= 256) -> (scores [B,classes,H,W]
    fp32 or None, labels [B,H,W] uint8 or None) at size = (H, W), one launch; only channels 0 .. classes-1 are read
    (classes = None: all).  Bit for bit segmentation.upsample_bilinear_ref; with scores=False the launch writes
    the label bytes only."""
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    x = np.ascontiguousarray(x_nhwc, dtype=np.float32)
    B, h, w, C = x.shape
    classes = C if classes is None else int(classes)
    H, W = int(size[0]), int(size[1])
    dx = _up_raw(x)
    ds = _DeviceBuffer(ctx, max(B * classes * H * W * 4, 16)) if scores else None
    dl = _DeviceBuffer(ctx, max(B * H * W, 16)) if labels else None
    L.check(L.lib().rn_upsample_bilinear_forward(ctx.handle, dx.ptr, B, h, w, classes, C, H, W, ds.ptr if ds else None,
                                                 dl.ptr if dl else None), "rn_upsample_bilinear_forward", ctx.handle)
    ctx.sync()
    s = _down_raw(ds, np.float32, B * classes * H * W).reshape(B, classes, H, W) if scores else None
    lb = _down_raw(dl, np.uint8, B * H * W).reshape(B, H, W) if labels else None
    return s, lb


def concat_channels_ref(srcs, per_image=None) -> np.ndarray:
    """The contract of rn_concat_channels_forward_dt in numpy: sources [B, pixels, C_i] (any one dtype) joined along
    the channels, then per_image [B, C_p] repeated at every pixel of its image.  A copy: no value is touched."""
    parts = [np.asarray(s) for s in srcs]
    if per_image is not None:
        p = np.asarray(per_image)
        B, pixels = parts[0].shape[:2]
        parts.append(np.broadcast_to(p[:, None, :], (B, pixels, p.shape[1])))
    return np.ascontiguousarray(np.concatenate(parts, axis=2))


def _concat_channels(dtype, np_dtype, srcs, per_image):
    from .tensor import _DeviceBuffer
    ctx, lib = get_ctx(), L.lib()
    srcs = [np.ascontiguousarray(s, dtype=np_dtype) for s in srcs]
    B, pixels = srcs[0].shape[:2]
    assert all(s.ndim == 3 and s.shape[:2] == (B, pixels) for s in srcs), [s.shape for s in srcs]
    ch = [int(s.shape[2]) for s in srcs]
    cp = 0
    dp = None
    if per_image is not None:
        per_image = np.ascontiguousarray(per_image, dtype=np_dtype)
        assert per_image.shape[0] == B and per_image.ndim == 2, per_image.shape
        cp, dp = int(per_image.shape[1]), _up_raw(per_image)
    bufs = [_up_raw(s) for s in srcs]
    total = sum(ch) + cp
    es = np.dtype(np_dtype).itemsize
    out = _DeviceBuffer(ctx, max(B * pixels * total * es, 16))
    ptrs = (ctypes.c_void_p * len(bufs))(*[b.ptr for b in bufs])
    chans = (ctypes.c_uint64 * len(ch))(*ch)
    L.check(lib.rn_concat_channels_forward_dt(ctx.handle, dtype, len(bufs), ptrs, chans, dp.ptr if dp else None, cp,
                                              out.ptr, B, pixels), "rn_concat_channels_forward_dt", ctx.handle)
    ctx.sync()
    return _down_raw(out, np_dtype, B * pixels * total).reshape(B, pixels, total)


def concat_channels(srcs, per_image=None) -> np.ndarray:
    """rn_concat_channels_forward_dt in fp32: host arrays [B, pixels, C_i] (C_i % 4 == 0) and per_image [B, C_p] or
    None -> [B, pixels, sum C_i + C_p], one launch; bit for bit concat_channels_ref."""
    return _concat_channels(L.RN_DTYPE_F32, np.float32, srcs, per_image)


def concat_channels_bf16(srcs, per_image=None) -> np.ndarray:
    """The bf16 form of concat_channels: uint16 bit patterns in (to_bf16_bits of fp32 data) and out, C_i % 8 == 0."""
    return _concat_channels(L.RN_DTYPE_BF16, np.uint16, srcs, per_image)


def nearest_index(n_in: int, n_out: int) -> np.ndarray:
    """The source index of every output index along one axis, as rn_upsample_nearest_add_forward_dt computes it
    (torch's size= form): scale = fp32(n_in) / fp32(n_out), i(o) = min(int(floor(fp32(fp32(o) * scale))), n_in - 1),
    the product rounded to fp32 on its own."""
    scale = np.float32(n_in) / np.float32(n_out)
    o = np.arange(n_out, dtype=np.float32)
    prod = (o * scale).astype(np.float32)
    return np.minimum(np.floor(prod).astype(np.int64), n_in - 1)


def upsample_nearest_add_ref(top, lat=None, size=None) -> np.ndarray:
    """The contract of rn_upsample_nearest_add_forward_dt in numpy: top [B,h,w,C] and lat [B,H,W,C] or None, NHWC;
    size = (H, W) (default: lat's).  fp32 arrays: lat + top[:, iy][:, :, ix], one fp32 add.  uint16 arrays (bf16 bit
    patterns): widened, added in fp32, rounded once to the nearest even bf16.  lat = None: the gathered copy of top,
    every bit kept."""
    top = np.asarray(top)
    if size is None:
        size = np.asarray(lat).shape[1:3]
    H, W = int(size[0]), int(size[1])
    iy, ix = nearest_index(top.shape[1], H), nearest_index(top.shape[2], W)
    up = top[:, iy][:, :, ix]
    if lat is None:
        return np.ascontiguousarray(up)
    lat = np.asarray(lat)
    assert lat.dtype == top.dtype and lat.shape == up.shape, (lat.shape, up.shape, lat.dtype, top.dtype)
    if top.dtype == np.uint16:
        with np.errstate(invalid="ignore"):
            return to_bf16_bits(from_bf16_bits(lat) + from_bf16_bits(up)).reshape(up.shape)
    assert top.dtype == np.float32, top.dtype
    with np.errstate(invalid="ignore"):
        return lat + up


def _upsample_nearest_add(dtype, np_dtype, top, lat, size):
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    top = np.ascontiguousarray(top, dtype=np_dtype)
    B, h, w, C = top.shape
    if lat is not None:
        lat = np.ascontiguousarray(lat, dtype=np_dtype)
        size = lat.shape[1:3] if size is None else size
        assert lat.shape == (B, int(size[0]), int(size[1]), C), (lat.shape, top.shape, size)
    H, W = int(size[0]), int(size[1])
    dt, dl = _up_raw(top), (_up_raw(lat) if lat is not None else None)
    n = B * H * W * C
    out = _DeviceBuffer(ctx, max(n * np.dtype(np_dtype).itemsize, 16))
    L.check(L.lib().rn_upsample_nearest_add_forward_dt(ctx.handle, dtype, dt.ptr, B, h, w, C, dl.ptr if dl else None,
                                                       out.ptr, H, W), "rn_upsample_nearest_add_forward_dt", ctx.handle)
    ctx.sync()
    return _down_raw(out, np_dtype, n).reshape(B, H, W, C)


def upsample_nearest_add(top, lat=None, size=None) -> np.ndarray:
    """rn_upsample_nearest_add_forward_dt in fp32: host arrays top [B,h,w,C] and lat [B,H,W,C] or None (then size =
    (H, W)), C % 4 == 0 -> lat + nearest_upsample(top) [B,H,W,C], one launch; bit for bit upsample_nearest_add_ref."""
    return _upsample_nearest_add(L.RN_DTYPE_F32, np.float32, top, lat, size)


def upsample_nearest_add_bf16(top, lat=None, size=None) -> np.ndarray:
    """The bf16 form of upsample_nearest_add: uint16 bit patterns in (to_bf16_bits of fp32 data) and out, C % 8 == 0."""
    return _upsample_nearest_add(L.RN_DTYPE_BF16, np.uint16, top, lat, size)


# ---------------------------------------------------------------------------
# RoIAlign over a pyramid (rn_roi_align_forward_dt)
# ---------------------------------------------------------------------------
def roi_level_thresholds(scales, canonical_scale: float = 224.0, canonical_level: int = 4) -> np.ndarray:
    """rn_roi_level_thresholds (host only): the len(scales) - 1 fp32 area thresholds between the levels of
    torchvision's LevelMapper, thr[j] = (s0 * 2^(k_min + 1 + j - k0 - 1e-6))^2 in double, rounded up to fp32."""
    sc = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
    thr = np.zeros(max(sc.size - 1, 1), dtype=np.float32)
    st = L.lib().rn_roi_level_thresholds(sc.size, sc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), float(canonical_scale),
                                         int(canonical_level), thr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    if st != L.RN_OK:
        raise ValueError(f"rn_roi_level_thresholds: 1..4 positive finite scales and a positive canonical scale, not {sc}")
    return thr[:sc.size - 1]


def roi_levels_ref(rois, thresholds, images: Optional[int] = None) -> np.ndarray:
    """The level of every RoI as the kernel chooses it: area = (x2 - x1) * (y2 - y1) in fp32, level = the number of j
    with area >= thresholds[j]; int32 [K].  images: a RoI whose image index is no integer in [0, images) gets -1."""
    r = np.ascontiguousarray(rois, dtype=np.float32).reshape(-1, 5)
    thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        area = (r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])
        lv = (area[:, None] >= thr[None, :]).sum(axis=1).astype(np.int32)
    if images is not None:
        lv[~roi_image_valid(r, images)] = -1
    return lv


def roi_image_valid(rois, images: int) -> np.ndarray:
    """Which RoIs name an image: the index is an integer in [0, images)."""
    b = np.ascontiguousarray(rois, dtype=np.float32).reshape(-1, 5)[:, 0]
    with np.errstate(invalid="ignore"):
        return (b >= 0) & (b < np.float32(2147483648.0)) & (b == np.trunc(b)) & (b.astype(np.float64) < images)


def _roi_axis(c, ok, n, ft):
    """the contract's "One sample" along one axis on an array of coordinates: (low index, high index, l, h)"""
    c = np.where(ok, c, ft(0))
    c = np.where(c > 0, c, ft(0))
    lo = c.astype(np.int64)
    top = lo >= n - 1
    lo = np.where(top, n - 1, lo)
    hi = np.where(top, n - 1, lo + 1)
    c = np.where(top, lo.astype(ft), c)
    lw = (c - lo.astype(ft)).astype(ft)
    return lo, hi, lw, (ft(1) - lw).astype(ft)


def _roi_align_host(maps_nhwc, rois, scales, output_size, sampling_ratio, aligned, levels, ft):
    """The contract of rn_roi_align_forward_dt in numpy, every operation in the float type ft and rounded on its own,
    vectorised over the channels and the sample grid of a RoI.  maps_nhwc: [B,h,w,C] arrays of ft; levels: the level
    of every RoI (-1: a row of zeros) -> [K,C,PH,PW] of ft."""
    PH, PW = (int(output_size), int(output_size)) if np.ndim(output_size) == 0 else (int(output_size[0]), int(output_size[1]))
    S = int(sampling_ratio)
    rois = np.asarray(rois).reshape(-1, 5)
    K, C = rois.shape[0], maps_nhwc[0].shape[3]
    out = np.zeros((K, C, PH, PW), dtype=ft)
    off = ft(0.5) if aligned else ft(0)
    grid = lambda n: ((np.arange(n, dtype=ft)[:, None], (np.arange(S, dtype=ft) + ft(0.5))[None, :]))  # noqa: E731
    (ph, sy), (pw, sx) = grid(PH), grid(PW)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(K):
            lv = int(levels[r])
            if lv < 0:
                continue
            m = maps_nhwc[lv]
            h, w = m.shape[1], m.shape[2]
            scale = ft(scales[lv])
            b, x1, y1, x2, y2 = (ft(v) for v in rois[r])
            x1s, y1s, x2s, y2s = x1 * scale - off, y1 * scale - off, x2 * scale - off, y2 * scale - off
            rw, rh = ft(x2s - x1s), ft(y2s - y1s)
            if not aligned:
                rw, rh = (ft(1) if rw < 1 else rw), (ft(1) if rh < 1 else rh)
            bin_h, bin_w = ft(rh / ft(PH)), ft(rw / ft(PW))
            y = ((y1s + ph * bin_h) + (sy * bin_h) / ft(S)).astype(ft).reshape(-1)      # [PH*S]
            x = ((x1s + pw * bin_w) + (sx * bin_w) / ft(S)).astype(ft).reshape(-1)      # [PW*S]
            oky, okx = (y >= -1) & (y <= h), (x >= -1) & (x <= w)
            ok = oky[:, None] & okx[None, :]
            yl, yh, ly, hy = _roi_axis(y, oky, h, ft)
            xl, xh, lx, hx = _roi_axis(x, okx, w, ft)
            img = m[int(b)]
            v1, v2 = img[yl][:, xl], img[yl][:, xh]
            v3, v4 = img[yh][:, xl], img[yh][:, xh]
            w1, w2 = (hy[:, None] * hx[None, :])[..., None], (hy[:, None] * lx[None, :])[..., None]
            w3, w4 = (ly[:, None] * hx[None, :])[..., None], (ly[:, None] * lx[None, :])[..., None]
            val = (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4).reshape(PH, S, PW, S, C)
            okg = ok.reshape(PH, S, PW, S)
            acc = np.zeros((PH, PW, C), dtype=ft)
            for iy in range(S):
                for ix in range(S):
                    acc = np.where(okg[:, iy, :, ix, None], acc + val[:, iy, :, ix], acc)
            out[r] = (acc / ft(S * S)).transpose(2, 0, 1)
    return out


def roi_align_ref(maps_nhwc, rois, scales, output_size, sampling_ratio: int = 2, aligned: bool = False,
                  thresholds=None, return_levels: bool = False):
    """The contract of rn_roi_align_forward_dt in numpy fp32 (include/rn_hip.h states it): maps_nhwc one [B,h,w,C]
    array per level, finest first, fp32 or uint16 bf16 bit patterns (widened exactly); rois [K,5] fp32 (image index,
    x1, y1, x2, y2) -> [K,C,PH,PW] fp32, and with return_levels the int32 level of every RoI.  A RoI whose image index
    is no integer in [0, B): zeros, level -1."""
    maps = [np.asarray(m) for m in maps_nhwc]
    maps = [from_bf16_bits(m).reshape(m.shape) if m.dtype == np.uint16 else np.ascontiguousarray(m, dtype=np.float32) for m in maps]
    rois = np.ascontiguousarray(rois, dtype=np.float32).reshape(-1, 5)
    if thresholds is None:
        thresholds = roi_level_thresholds(scales)
    levels = roi_levels_ref(rois, thresholds, images=maps[0].shape[0])
    out = _roi_align_host(maps, rois, np.asarray(scales, dtype=np.float32), output_size, sampling_ratio, aligned, levels,
                          np.float32)
    return (out, levels) if return_levels else out


def _roi_align(dtype, np_dtype, maps_nhwc, rois, scales, output_size, sampling_ratio, aligned, thresholds, return_levels,
               nhwc: bool = False, validate: bool = True):
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    maps = [np.ascontiguousarray(m, dtype=np_dtype) for m in maps_nhwc]
    n, (B, C) = len(maps), (maps[0].shape[0], maps[0].shape[3])
    assert all(m.ndim == 4 and m.shape[0] == B and m.shape[3] == C for m in maps), [m.shape for m in maps]
    rois = np.ascontiguousarray(rois, dtype=np.float32).reshape(-1, 5)
    K = rois.shape[0]
    if validate and not roi_image_valid(rois, B).all():
        raise ValueError(f"a RoI's image index is no integer in [0, {B})")
    PH, PW = (int(output_size), int(output_size)) if np.ndim(output_size) == 0 else (int(output_size[0]), int(output_size[1]))
    sc = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
    assert sc.size == n, (sc.size, n)
    thr = roi_level_thresholds(sc) if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
    assert thr.size == n - 1, (thr.size, n)
    thr = np.concatenate([thr, np.zeros(1, np.float32)])       # never an empty array behind the pointer
    dm, dr = [_up_raw(m) for m in maps], _up_raw(rois)
    out = _DeviceBuffer(ctx, max(K * C * PH * PW * 4, 16))
    lv = _DeviceBuffer(ctx, max(K * 4, 16)) if return_levels else None
    fp = ctypes.POINTER(ctypes.c_float)
    name = "rn_roi_align_nhwc_forward_dt" if nhwc else "rn_roi_align_forward_dt"
    L.check(getattr(L.lib(), name)(
        ctx.handle, dtype, n, (ctypes.c_void_p * n)(*[d.ptr for d in dm]), (ctypes.c_uint64 * n)(*[m.shape[1] for m in maps]),
        (ctypes.c_uint64 * n)(*[m.shape[2] for m in maps]), sc.ctypes.data_as(fp), thr.ctypes.data_as(fp), B, C, dr.ptr, K,
        PH, PW, int(sampling_ratio), int(bool(aligned)), out.ptr, lv.ptr if lv else None), name, ctx.handle)
    ctx.sync()
    pooled = _down_raw(out, np.float32, K * C * PH * PW).reshape((K, PH, PW, C) if nhwc else (K, C, PH, PW))
    return (pooled, _down_raw(lv, np.int32, K)) if return_levels else pooled


def roi_align(maps_nhwc, rois, scales, output_size, sampling_ratio: int = 2, aligned: bool = False, thresholds=None,
              return_levels: bool = False):
    """rn_roi_align_forward_dt in fp32, one launch: host arrays maps_nhwc (one [B,h,w,C] per level, finest first,
    C % 4 == 0), rois [K,5] (image index, x1, y1, x2, y2), scales per level -> [K,C,PH,PW] fp32, bit for bit
    roi_align_ref; thresholds default to roi_level_thresholds(scales); return_levels: (pooled, int32 [K]).  A RoI
    whose image index is no integer in [0, B) raises ValueError."""
    return _roi_align(L.RN_DTYPE_F32, np.float32, maps_nhwc, rois, scales, output_size, sampling_ratio, aligned, thresholds,
                      return_levels)


def roi_align_bf16(maps_nhwc, rois, scales, output_size, sampling_ratio: int = 2, aligned: bool = False, thresholds=None,
                   return_levels: bool = False):
    """The bf16 form of roi_align: the maps are uint16 bit patterns (to_bf16_bits of fp32 data), C % 8 == 0; the
    output is fp32."""
    return _roi_align(L.RN_DTYPE_BF16, np.uint16, maps_nhwc, rois, scales, output_size, sampling_ratio, aligned, thresholds,
                      return_levels)


def roi_align_nhwc(maps_nhwc, rois, scales, output_size, sampling_ratio: int = 2, aligned: bool = False, thresholds=None,
                   return_levels: bool = False, bf16: bool = False, validate: bool = True):
    """rn_roi_align_nhwc_forward_dt, one launch: roi_align's arguments (bf16: roi_align_bf16's) -> [K,PH,PW,C] fp32, bit
    for bit the transpose of what roi_align returns.  validate=False hands a RoI whose image index is no integer in
    [0, B) -- the rows detection_rois forms of padding detections -- to the device, which answers zeros and level -1."""
    return _roi_align(L.RN_DTYPE_BF16 if bf16 else L.RN_DTYPE_F32, np.uint16 if bf16 else np.float32, maps_nhwc, rois, scales,
                      output_size, sampling_ratio, aligned, thresholds, return_levels, nhwc=True, validate=validate)


# ---------------------------------------------------------------------------
# RPN proposals behind the head (rn_rpn.hip); the contract in numpy is rpn.py's
# ---------------------------------------------------------------------------
def box_decode_ref(anchors, deltas, weights=(1.0, 1.0, 1.0, 1.0), image_size=(np.inf, np.inf)) -> np.ndarray:
    from . import rpn
    return rpn.decode_ref(anchors, deltas, weights, image_size)


def nms_ref(boxes, iou_threshold: float, valid=None) -> np.ndarray:
    from . import rpn
    return rpn.nms_ref(boxes, iou_threshold, valid)


def nms_segments_ref(boxes, iou_threshold: float, valid=None) -> np.ndarray:
    boxes = np.asarray(boxes, dtype=np.float32)
    return np.stack([nms_ref(boxes[s], iou_threshold, None if valid is None else valid[s]) for s in range(boxes.shape[0])])


def box_decode(anchors, deltas, weights=(1.0, 1.0, 1.0, 1.0), image_size=(np.inf, np.inf)) -> np.ndarray:
    """rn_box_decode_forward, one launch: anchors [N,4] + deltas [N,4] -> boxes [N,4] fp32, BoxCoder.decode_single
    with `weights` then the clip to image_size (H, W); box_decode_ref up to the device's expf."""
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    a = np.ascontiguousarray(anchors, dtype=np.float32).reshape(-1, 4)
    d = np.ascontiguousarray(deltas, dtype=np.float32).reshape(-1, 4)
    assert a.shape == d.shape, (a.shape, d.shape)
    N = a.shape[0]
    da, dd, out = _up_raw(a), _up_raw(d), _DeviceBuffer(ctx, max(N * 16, 16))
    L.check(L.lib().rn_box_decode_forward(ctx.handle, da.ptr, dd.ptr, N, *[float(v) for v in weights], float(image_size[0]),
                                          float(image_size[1]), out.ptr), "rn_box_decode_forward", ctx.handle)
    ctx.sync()
    return _down_raw(out, np.float32, N * 4).reshape(N, 4)


def nms_segments(boxes, iou_threshold: float, valid=None, return_count: bool = False):
    """rn_nms_forward, two launches: S segments of n <= 4096 boxes [S,n,4], each already in score order, valid [S,n]
    or None -> keep, bool [S,n], bit for bit nms_segments_ref (and the kept count of every segment)."""
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    b = np.ascontiguousarray(boxes, dtype=np.float32)
    assert b.ndim == 3 and b.shape[2] == 4, b.shape
    S, n = b.shape[:2]
    db = _up_raw(b)
    dv = _up_raw(np.ascontiguousarray(valid).astype(np.uint8).reshape(S, n)) if valid is not None else None
    keep, cnt = _DeviceBuffer(ctx, max(S * n, 16)), _DeviceBuffer(ctx, max(S * 4, 16))
    L.check(L.lib().rn_nms_forward(ctx.handle, db.ptr, dv.ptr if dv else None, S, n, float(iou_threshold), keep.ptr, cnt.ptr),
            "rn_nms_forward", ctx.handle)
    ctx.sync()
    k = _down_raw(keep, np.uint8, S * n).reshape(S, n).astype(bool)
    return (k, _down_raw(cnt, np.int32, S)) if return_count else k


def nms(boxes, scores, iou_threshold: float) -> np.ndarray:
    """torchvision.ops.nms: the indices of the boxes greedy NMS keeps, in descending score (ties: the lower index
    first; the host sorts, the device suppresses).  n <= 4096."""
    from . import rpn
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
    order = rpn.select_ref(scores, b.shape[0])
    if order.size == 0:
        return order
    return order[nms_segments(b[order][None], iou_threshold)[0]]


def _cand_buffers(ctx, B, n_levels, pre):
    from .tensor import _DeviceBuffer
    rows = B * n_levels * pre
    spec = (("index", np.int32, rows, (B, n_levels, pre)), ("logit", np.float32, rows, (B, n_levels, pre)),
            ("box", np.float32, rows * 4, (B, n_levels, pre, 4)), ("valid", np.uint8, rows, (B, n_levels, pre)),
            ("count", np.int32, B * n_levels, (B, n_levels)))
    bufs = {k: _DeviceBuffer(ctx, max(n * np.dtype(t).itemsize, 16)) for k, t, n, _ in spec}
    return spec, bufs, L.RpnCandidates(*[bufs[k].ptr for k, *_ in spec])


def _select_decode_launch(ctx, heads, base, image_size, pre, min_size, logit_thresh):
    heads = [np.ascontiguousarray(hd, dtype=np.float32) for hd in heads]
    base = np.ascontiguousarray(base, dtype=np.float32)
    n_levels, A = base.shape[:2]
    B = heads[0].shape[0]
    P = (5 * A + 3) // 4 * 4
    assert len(heads) == n_levels and all(hd.ndim == 4 and hd.shape[0] == B and hd.shape[3] == P for hd in heads), \
        [hd.shape for hd in heads]
    dh = [_up_raw(hd) for hd in heads]
    spec, bufs, cand = _cand_buffers(ctx, B, n_levels, int(pre))
    L.check(L.lib().rn_rpn_select_decode_forward(
        ctx.handle, n_levels, (ctypes.c_void_p * n_levels)(*[d.ptr for d in dh]), B,
        (ctypes.c_uint64 * n_levels)(*[hd.shape[1] for hd in heads]), (ctypes.c_uint64 * n_levels)(*[hd.shape[2] for hd in heads]),
        A, base.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), int(image_size[0]), int(image_size[1]), int(pre),
        float(min_size), float(logit_thresh), ctypes.byref(cand)), "rn_rpn_select_decode_forward", ctx.handle)
    return dh, spec, bufs, cand


def rpn_select_decode(heads, base_anchors, image_size, pre_nms_top_n: int, min_size: float = 1e-3,
                      logit_thresh: float = -np.inf) -> dict:
    """rn_rpn_select_decode_forward, one launch: heads one host [B,h,w,P] per level, base_anchors [L,A,4] -> the
    candidates per (image, level, rank): "index" int32, "logit", "box", "valid" (bytes) and "count" [B,L]; index,
    logit and count bit for bit rpn.select_decode_ref's, box within test_rpn_host.decode_bound of rpn.decode_f64."""
    ctx = get_ctx()
    _dh, spec, bufs, _cand = _select_decode_launch(ctx, heads, base_anchors, image_size, pre_nms_top_n, min_size, logit_thresh)
    ctx.sync()
    return {k: _down_raw(bufs[k], t, n).reshape(shape) for k, t, n, shape in spec}


def rpn_proposals(heads, base_anchors, image_size, pre_nms_top_n: int, post_nms_top_n: int, nms_thresh: float,
                  min_size: float = 1e-3, logit_thresh: float = -np.inf):
    """rn_rpn_select_decode_forward and rn_rpn_nms_merge_forward, three launches, nothing leaving the device in
    between: (candidates as rpn_select_decode returns them, proposals): "boxes" [B,post,4], "logits", "levels" int32,
    "count" [B], "rois" [B*post,5], "cand_keep" [B,L,pre]; the proposals bit for bit rpn.nms_merge_ref of the
    candidates."""
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    pre, post = int(pre_nms_top_n), int(post_nms_top_n)
    _dh, spec, bufs, cand = _select_decode_launch(ctx, heads, base_anchors, image_size, pre, min_size, logit_thresh)
    B, n_levels = spec[0][3][0], spec[0][3][1]
    ospec = (("boxes", np.float32, B * post * 4, (B, post, 4)), ("logits", np.float32, B * post, (B, post)),
             ("levels", np.int32, B * post, (B, post)), ("count", np.int32, B, (B,)),
             ("rois", np.float32, B * post * 5, (B * post, 5)), ("cand_keep", np.uint8, B * n_levels * pre, (B, n_levels, pre)))
    obufs = {k: _DeviceBuffer(ctx, max(n * np.dtype(t).itemsize, 16)) for k, t, n, _ in ospec}
    out = L.RpnProposals(*[obufs[k].ptr for k, *_ in ospec])
    L.check(L.lib().rn_rpn_nms_merge_forward(ctx.handle, ctypes.byref(cand), B, n_levels, pre, post, float(nms_thresh),
                                             ctypes.byref(out)), "rn_rpn_nms_merge_forward", ctx.handle)
    ctx.sync()
    return ({k: _down_raw(bufs[k], t, n).reshape(shape) for k, t, n, shape in spec},
            {k: _down_raw(obufs[k], t, n).reshape(shape) for k, t, n, shape in ospec})


# ---------------------------------------------------------------------------
# The box head's post-processing (rn_detect.hip); the contract in numpy is detection.py's
# ---------------------------------------------------------------------------
def detect_postprocess(head, rois, B: int, C: int, image_size, score_thresh: float = 0.05, nms_thresh: float = 0.5,
                       detections_per_img: int = 100, weights=(10.0, 10.0, 5.0, 5.0), min_size: float = 1e-2,
                       intermediates: bool = False) -> dict:
    """rn_detect_postprocess_forward, three launches: head [K,P] and rois [K,5] host arrays of B images (K = B*R) ->
    "boxes" [B,D,4], "scores", "labels", "roi" int32 [B,D], "count" [B]; with intermediates also "probs" [K,C],
    "class_boxes" [K,C,4], "valid" and "keep" [K,C].  Bit for bit detection.postprocess_ref on the device's own
    probabilities and class boxes."""
    from . import detection
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    h = np.ascontiguousarray(head, dtype=np.float32)
    r = np.ascontiguousarray(rois, dtype=np.float32).reshape(-1, 5)
    K = h.shape[0]
    assert h.shape == (K, detection.head_pitch(C)) and r.shape[0] == K and B > 0 and K % B == 0, (h.shape, r.shape, B, C)
    dh, dr = _up_raw(h), _up_raw(r)
    spec = detection.output_spec(B, K // B, C, int(detections_per_img), intermediates)
    bufs = {k: _DeviceBuffer(ctx, max(int(np.prod(sh)) * np.dtype(t).itemsize, 16)) for k, (t, sh) in spec.items()}
    req = detection.make_request(bufs, score_thresh, nms_thresh, min_size, detections_per_img, weights)
    L.check(L.lib().rn_detect_postprocess_forward(ctx.handle, dh.ptr, dr.ptr, B, K // B, C, int(image_size[0]), int(image_size[1]),
                                                  ctypes.byref(req)), "rn_detect_postprocess_forward", ctx.handle)
    ctx.sync()
    return {k: _down_raw(bufs[k], t, int(np.prod(sh))).reshape(sh) for k, (t, sh) in spec.items()}


# ---------------------------------------------------------------------------
# The mask head's launches (rn_mask.hip); the contracts in numpy are mask.py's
# ---------------------------------------------------------------------------
def detection_rois(boxes, labels) -> np.ndarray:
    """rn_detection_rois_forward, one launch: boxes [B,D,4] fp32 and labels [B,D] int32 -> rois [B*D,5], bit for bit
    mask.detection_rois_ref."""
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    B, D = lab.shape
    bx = np.ascontiguousarray(boxes, dtype=np.float32).reshape(B, D, 4)
    db, dl, out = _up_raw(bx), _up_raw(lab), _DeviceBuffer(ctx, max(B * D * 20, 16))
    L.check(L.lib().rn_detection_rois_forward(ctx.handle, db.ptr, dl.ptr, B, D, out.ptr), "rn_detection_rois_forward", ctx.handle)
    ctx.sync()
    return _down_raw(out, np.float32, B * D * 5).reshape(B * D, 5)


def mask_predict(t, labels, weight, bias) -> np.ndarray:
    """rn_mask_predict_forward, one launch: t [K,M,M,4*Cr] fp32 (channel (dy*2+dx)*Cr + c), labels [K] int32, weight
    [C,Cr(,1,1)] and bias [C] -> probs [K,2M,2M] fp32: the sigmoid of the label's row of the 1x1, rows of a label outside
    [1, C) zeros; within the bound of tests/test_mask_gpu.py of mask.predict_ref."""
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    t = np.ascontiguousarray(t, dtype=np.float32)
    K, M, _, c4 = t.shape
    w = np.ascontiguousarray(weight, dtype=np.float32).reshape(np.shape(weight)[0], -1)
    b = np.ascontiguousarray(bias, dtype=np.float32).reshape(-1)
    lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    assert t.shape[2] == M and c4 == 4 * w.shape[1] and b.size == w.shape[0] and lab.size == K, (t.shape, w.shape, b.shape, lab.shape)
    dt, dl, dw, db = _up_raw(t), _up_raw(lab), _up_raw(w), _up_raw(b)
    out = _DeviceBuffer(ctx, max(K * 4 * M * M * 4, 16))
    L.check(L.lib().rn_mask_predict_forward(ctx.handle, dt.ptr, dl.ptr, dw.ptr, db.ptr, K, M, w.shape[1], w.shape[0], out.ptr),
            "rn_mask_predict_forward", ctx.handle)
    ctx.sync()
    return _down_raw(out, np.float32, K * 4 * M * M).reshape(K, 2 * M, 2 * M)


def paste_masks(probs, boxes, image_size, labels=None, threshold: float = 0.5, masks: bool = True, bits: bool = False):
    """rn_paste_masks_forward, one launch: probs [K,Mo,Mo] fp32, boxes [K,4], labels [K] int32 or None -> (masks
    [K,H,W] fp32 or None, bits [K,H,W] uint8 or None) at image_size = (H, W); masks bit for bit mask.paste_masks_ref,
    bits == masks > threshold."""
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    p = np.ascontiguousarray(probs, dtype=np.float32)
    K, Mo = p.shape[0], p.shape[1]
    H, W = int(image_size[0]), int(image_size[1])
    bx = np.ascontiguousarray(boxes, dtype=np.float32).reshape(K, 4)
    dp, db = _up_raw(p), _up_raw(bx)
    dl = _up_raw(np.ascontiguousarray(labels, dtype=np.int32).reshape(K)) if labels is not None else None
    dm = _DeviceBuffer(ctx, max(K * H * W * 4, 16)) if masks else None
    dbits = _DeviceBuffer(ctx, max(K * H * W, 16)) if bits else None
    L.check(L.lib().rn_paste_masks_forward(ctx.handle, dp.ptr, db.ptr, dl.ptr if dl else None, K, Mo, H, W, float(threshold),
                                           dm.ptr if dm else None, dbits.ptr if dbits else None), "rn_paste_masks_forward", ctx.handle)
    ctx.sync()
    return (_down_raw(dm, np.float32, K * H * W).reshape(K, H, W) if masks else None,
            _down_raw(dbits, np.uint8, K * H * W).reshape(K, H, W) if bits else None)


# ---------------------------------------------------------------------------
# The keypoint head's launch (rn_keypoint.hip); the contracts in numpy are keypoint.py's
# ---------------------------------------------------------------------------
def keypoint_predict(t, bias, boxes=None, image_size=None, labels=None, heat: bool = True, keypoints: bool = True):
    """rn_keypoint_predict_forward, one launch: the panel's output t [K,M,M,16*Kp] fp32 and bias [Kp] -> (heat
    [K,Kp,4M,4M] or None, keypoints [K,Kp,3] or None, scores [K,Kp] or None); keypoints need boxes [K,4] and image_size =
    (max_h, max_w); labels [K] int32 or None.  heat bit for bit keypoint.heatmaps_ref, keypoints and scores bit for bit
    keypoint.heatmaps_to_keypoints_ref on it."""
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    t = np.ascontiguousarray(t, dtype=np.float32)
    K, M, _, c16 = t.shape
    b = np.ascontiguousarray(bias, dtype=np.float32).reshape(-1)
    Kp = b.size
    assert t.shape[2] == M and c16 == 16 * Kp, (t.shape, b.shape)
    S = 4 * M
    dt, dbias = _up_raw(t), _up_raw(b)
    dbox = _up_raw(np.ascontiguousarray(boxes, dtype=np.float32).reshape(K, 4)) if boxes is not None else None
    dl = _up_raw(np.ascontiguousarray(labels, dtype=np.int32).reshape(K)) if labels is not None else None
    size = image_size if image_size is not None else (1, 1)
    dh = _DeviceBuffer(ctx, max(K * Kp * S * S * 4, 16)) if heat else None
    dk = _DeviceBuffer(ctx, max(K * Kp * 12, 16)) if keypoints else None
    ds = _DeviceBuffer(ctx, max(K * Kp * 4, 16)) if keypoints else None
    L.check(L.lib().rn_keypoint_predict_forward(ctx.handle, dt.ptr, dbias.ptr, dbox.ptr if dbox else None, dl.ptr if dl else None,
                                                K, M, Kp, int(size[0]), int(size[1]), dh.ptr if dh else None,
                                                dk.ptr if dk else None, ds.ptr if ds else None),
            "rn_keypoint_predict_forward", ctx.handle)
    ctx.sync()
    return (_down_raw(dh, np.float32, K * Kp * S * S).reshape(K, Kp, S, S) if heat else None,
            _down_raw(dk, np.float32, K * Kp * 3).reshape(K, Kp, 3) if keypoints else None,
            _down_raw(ds, np.float32, K * Kp).reshape(K, Kp) if keypoints else None)


def heatmaps_to_keypoints(heat, boxes, image_size, labels=None):
    """rn_heatmaps_to_keypoints_forward, one launch: heat [K,Kp,S,S] fp32, boxes [K,4], image_size = (max_h, max_w),
    labels [K] int32 or None -> (keypoints [K,Kp,3], scores [K,Kp]), bit for bit keypoint.heatmaps_to_keypoints_ref."""
    from .tensor import _DeviceBuffer
    ctx = get_ctx()
    x = np.ascontiguousarray(heat, dtype=np.float32)
    K, Kp, S, _ = x.shape
    dh, dbox = _up_raw(x), _up_raw(np.ascontiguousarray(boxes, dtype=np.float32).reshape(K, 4))
    dl = _up_raw(np.ascontiguousarray(labels, dtype=np.int32).reshape(K)) if labels is not None else None
    dk, ds = _DeviceBuffer(ctx, max(K * Kp * 12, 16)), _DeviceBuffer(ctx, max(K * Kp * 4, 16))
    L.check(L.lib().rn_heatmaps_to_keypoints_forward(ctx.handle, dh.ptr, dbox.ptr, dl.ptr if dl else None, K, Kp, S,
                                                     int(image_size[0]), int(image_size[1]), dk.ptr, ds.ptr),
            "rn_heatmaps_to_keypoints_forward", ctx.handle)
    ctx.sync()
    return _down_raw(dk, np.float32, K * Kp * 3).reshape(K, Kp, 3), _down_raw(ds, np.float32, K * Kp).reshape(K, Kp)
