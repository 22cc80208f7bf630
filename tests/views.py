"""Op entry points on offset views with guard bands (test infrastructure; used by test_views_gpu.py and
tests/fuzz/view_fuzz.py).

The C-ABI takes device pointers and sizes, and callers hand it slices of larger buffers.  `place` puts
a tensor at `guard + offset` bytes into one device allocation whose remaining bytes hold a guard pattern;
`fetch` downloads the whole allocation, checks that every guard byte still holds the pattern and returns
the tensor part.  Input guards hold NaN (bytes 0xFF: fp32 0xFFFFFFFF, bf16 0xFFFF) -- for max-pool inputs
+inf, which a maximum cannot swallow -- so a read outside the tensor poisons the result instead of
blending in; output buffers are filled entirely with 0xA5 (-2.9e-16 as fp32: no plausible result), so an
element that was never written shows as well.

The guard width is a condition of the check, not a measurement: 256 bytes on each side, sixteen 16-byte
stores, the widest access any kernel here issues.  It bounds what the check can see: an overrun that
skips the first 256 bytes behind (or before) the tensor entirely is missed.  Within the guards every byte
is compared, with no sampling.

The `run_*` functions below make ONE call of an entry point on such views, operand by operand at the byte
offsets given in `offs` (operand name -> offset from a 16-byte boundary, default 0), check the guards of
every operand and return the result as the host array the oracle returns (NCHW)."""
import ctypes

import numpy as np

import resnet_c_amd as R
from resnet_c_amd import _lib as L
from resnet_c_amd.tensor import _DeviceBuffer

GUARD = 256
OUT_BYTE = 0xA5
_LAYOUT = {"nchw": L.RN_LAYOUT_NCHW, "nhwc": L.RN_LAYOUT_NHWC}


class View:
    """A tensor of `nbytes` bytes at `ptr`, `lo` bytes into the allocation `buf`; `image` is the host copy
    of the whole allocation as it was uploaded."""

    def __init__(self, buf, lo, nbytes, image, offset):
        self.buf, self.lo, self.nbytes, self.image, self.offset = buf, lo, nbytes, image, offset
        self.ptr = buf.ptr + lo


def place(arr, offset_bytes=0, guard_bytes=GUARD, fill="nan", nbytes=None):
    """One device allocation of guard + offset + nbytes + guard bytes, uploaded whole from a host image.
    fill: "nan" (0xFF bytes), "inf" (fp32 +inf) or "out" (every byte 0xA5, the tensor part included: pass
    arr=None and nbytes)."""
    ctx = R.get_ctx()
    if arr is not None:
        arr = np.ascontiguousarray(arr)
        if arr.dtype == np.float64:   # (a float32 array divided by np.sqrt(...): uploaded as fp32, like ops._up)
            arr = arr.astype(np.float32)
        nbytes = arr.nbytes
    lo, total = guard_bytes + offset_bytes, 2 * guard_bytes + offset_bytes + nbytes
    if fill == "inf":
        assert lo % 4 == 0 and nbytes % 4 == 0
        image = np.full((total + 3) // 4, np.inf, dtype=np.float32).view(np.uint8)[:total].copy()
    else:
        image = np.full(total, OUT_BYTE if fill == "out" else 0xFF, dtype=np.uint8)
    if arr is not None:
        image[lo:lo + nbytes] = arr.reshape(-1).view(np.uint8)
    buf = _DeviceBuffer(ctx, total)
    assert buf.ptr % 16 == 0 and guard_bytes % 16 == 0, "the allocator's base is the 16-byte boundary offsets count from"
    L.check(L.lib().rn_memcpy_h2d(ctx.handle, buf.ptr, image.ctypes.data, total), "h2d", ctx.handle)
    return View(buf, lo, nbytes, image, offset_bytes)


def place_out(nbytes, offset_bytes=0, guard_bytes=GUARD):
    return place(None, offset_bytes, guard_bytes, "out", nbytes)


def _download(view):
    ctx = R.get_ctx()
    whole = np.empty(view.image.size, dtype=np.uint8)
    L.check(L.lib().rn_memcpy_d2h(ctx.handle, whole.ctypes.data, view.buf.ptr, whole.size), "d2h", ctx.handle)
    return whole


def fetch(view, dtype=np.float32, what=""):
    """The tensor part of the view, after checking both guards byte for byte."""
    whole = _download(view)
    lo, hi = view.lo, view.lo + view.nbytes
    before = np.flatnonzero(whole[:lo] != view.image[:lo])
    after = np.flatnonzero(whole[hi:] != view.image[hi:])
    if before.size:
        raise AssertionError(f"{what}: offset +{view.offset}: guard BEFORE the tensor written, {before.size} bytes dirty, "
                             f"the nearest {lo - int(before[-1])} bytes before its first element")
    if after.size:
        raise AssertionError(f"{what}: offset +{view.offset}: guard BEHIND the tensor written, {after.size} bytes dirty, "
                             f"the first {int(after[0])} bytes past its last element")
    return whole[lo:hi].view(dtype).copy()


def check_guards(what, *views):
    for v in views:
        if v is not None:
            fetch(v, np.uint8, what)


def assert_untouched(view, what=""):
    """Nothing was launched on this buffer: tensor part and guards as uploaded."""
    whole = _download(view)
    dirty = np.flatnonzero(whole != view.image)
    assert dirty.size == 0, f"{what}: {dirty.size} bytes changed, the first at {int(dirty[0]) - view.lo} from the tensor"


def call(name, *args, layout=None):
    """One C-ABI call on the shared context, then a sync; returns (status, rn_last_error text)."""
    ctx, lib = R.get_ctx(), L.lib()
    if layout is not None:
        ctx.set_layout(_LAYOUT[layout])
    st = getattr(lib, name)(ctx.handle, *args)
    msg = (lib.rn_last_error(ctx.handle) or b"").decode() if st != L.RN_OK else ""
    ctx.sync()
    if layout is not None:
        ctx.set_layout(L.RN_LAYOUT_NCHW)
    return st, msg


def must(name, *args, layout=None):
    st, msg = call(name, *args, layout=layout)
    assert st == L.RN_OK, f"{name}: status {st} ({msg})"


def _dev(a, layout):
    a = np.asarray(a, dtype=np.float32)
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)) if layout == "nhwc" and a.ndim == 4 else a


def _host(flat, shape_nchw, layout):
    if layout == "nhwc" and len(shape_nchw) == 4:
        B, C, H, W = shape_nchw
        return flat.reshape(B, H, W, C).transpose(0, 3, 1, 2).copy()
    return flat.reshape(shape_nchw).copy()


def out_size(x, k, s, p):
    return (2 * p + x - k) // s + 1


# ---- the fp32 entry points ----------------------------------------------------------------------------
def run_relu(x, offs, inplace):
    what = f"rn_relu_forward n={x.size} inplace={inplace} offs={offs}"
    vi = place(x, offs.get("inp", 0))
    vo = vi if inplace else place_out(x.nbytes, offs.get("out", 0))
    must("rn_relu_forward", vi.ptr, vo.ptr, x.size)
    check_guards(what, vi)
    return fetch(vo, np.float32, what)


def run_add(a, b, offs, inplace):
    what = f"rn_add_forward n={a.size} inplace={inplace} offs={offs}"
    va, vb = place(a, offs.get("inp1", 0)), place(b, offs.get("inp2", 0))
    vo = va if inplace else place_out(a.nbytes, offs.get("out", 0))
    must("rn_add_forward", va.ptr, vb.ptr, vo.ptr, a.size)
    check_guards(what, va, vb)
    return fetch(vo, np.float32, what)


def run_batchnorm(x, w, b, m, v, layout, offs, inplace):
    what = f"rn_batchnorm2d_forward {layout} {x.shape} inplace={inplace} offs={offs}"
    B, C = x.shape[:2]
    vi = place(_dev(x, layout), offs.get("inp", 0))
    vo = vi if inplace else place_out(x.nbytes, offs.get("out", 0))
    vp = [place(t, offs.get(n, 0)) for n, t in (("weight", w), ("bias", b), ("mean", m), ("var", v))]
    must("rn_batchnorm2d_forward", vi.ptr, vo.ptr, *(t.ptr for t in vp), B, C, int(np.prod(x.shape[2:])), layout=layout)
    check_guards(what, vi, *vp)
    return _host(fetch(vo, np.float32, what), x.shape, layout)


def run_pool(kind, x, k, s, p, layout, offs):
    name = f"rn_{kind}pool2d_forward"
    what = f"{name} {layout} {x.shape} k={k} s={s} p={p} offs={offs}"
    B, C, H, W = x.shape
    ho, wo = out_size(H, k, s, p), out_size(W, k, s, p)
    vi = place(_dev(x, layout), offs.get("inp", 0), fill="inf" if kind == "max" else "nan")
    vo = place_out(B * C * ho * wo * 4, offs.get("out", 0))
    must(name, vi.ptr, vo.ptr, k, s, p, ho, wo, B, C, H, W, layout=layout)
    check_guards(what, vi)
    return _host(fetch(vo, np.float32, what), (B, C, ho, wo), layout)


def run_transpose(name, src, dst_shape, dims, offs):
    """rn_nchw_to_nhwc / rn_nhwc_to_nchw: src as the device holds it, dims = (B, C, H, W)."""
    what = f"{name} {dims} offs={offs}"
    vi, vo = place(src, offs.get("src", 0)), place_out(src.nbytes, offs.get("dst", 0))
    must(name, vi.ptr, vo.ptr, *dims)
    check_guards(what, vi)
    return fetch(vo, np.float32, what).reshape(dst_shape)


def run_pad(x, Cpad, border, offs, dt):
    """rn_nchw_to_nhwc_pad (dt=False, border 0) or rn_nchw_to_nhwc_pad_dt(RN_DTYPE_F32)."""
    B, C, H, W = x.shape
    what = f"rn_nchw_to_nhwc_pad{'_dt' if dt else ''} {x.shape} Cpad={Cpad} border={border} offs={offs}"
    Hp, Wp = H + 2 * border, W + 2 * border
    vi, vo = place(x, offs.get("src", 0)), place_out(B * Hp * Wp * Cpad * 4, offs.get("dst", 0))
    if dt:
        must("rn_nchw_to_nhwc_pad_dt", L.RN_DTYPE_F32, vi.ptr, vo.ptr, B, C, H, W, Cpad, border)
    else:
        assert border == 0
        must("rn_nchw_to_nhwc_pad", vi.ptr, vo.ptr, B, C, H, W, Cpad)
    check_guards(what, vi)
    return fetch(vo, np.float32, what).reshape(B, Hp, Wp, Cpad)


def pad_reference(x, Cpad, border):
    B, C, H, W = x.shape
    want = np.zeros((B, H + 2 * border, W + 2 * border, Cpad), dtype=np.float32)
    want[:, border:border + H, border:border + W, :C] = x.transpose(0, 2, 3, 1)
    return want


def run_linear(x, w, b, offs):
    what = f"rn_linear_forward {x.shape}->{w.shape[0]} bias={b is not None} offs={offs}"
    B, fin = x.shape
    fout = w.shape[0]
    vi, vw = place(x, offs.get("inp", 0)), place(w, offs.get("weight", 0))
    vb = place(b, offs.get("bias", 0)) if b is not None else None
    vo = place_out(B * fout * 4, offs.get("out", 0))
    must("rn_linear_forward", vi.ptr, vo.ptr, vw.ptr, vb.ptr if vb else None, B, fin, fout)
    check_guards(what, vi, vw, vb)
    return fetch(vo, np.float32, what).reshape(B, fout)


def linear_is_direct(fin, b, offs):
    """The dispatch of rn_linear_forward as include/rn_hip.h states it: the element-wise kernel (reference
    summation order) unless in_features % 32 == 0 and every operand sits on a 16-byte boundary."""
    names = ("inp", "out", "weight") + (("bias",) if b is not None else ())
    return fin % 32 != 0 or any(offs.get(n, 0) % 16 for n in names)


def packed_weight(w):
    """rn_conv2d_pack_weight of an OIHW weight, as host floats."""
    Cout, Cin, k, _ = w.shape
    n = int(L.lib().rn_conv2d_packed_weight_numel(Cin, Cout, k))
    vw, vp = place(w), place_out(n * 4)
    must("rn_conv2d_pack_weight", vw.ptr, vp.ptr, Cin, Cout, k)
    return fetch(vp, np.float32, f"rn_conv2d_pack_weight {w.shape}")


def run_conv_nhwc(x, w, s, p, scale, shift, residual, relu, offs):
    """rn_conv2d_nhwc_forward with an epilogue; NCHW host arrays in and out."""
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    what = f"rn_conv2d_nhwc_forward {x.shape} w={w.shape} s={s} p={p} offs={offs}"
    ho, wo = out_size(H, k, s, p), out_size(W, k, s, p)
    cs = int(L.lib().rn_conv2d_input_channels(Cin))
    xp = np.zeros((B, H, W, cs), dtype=np.float32)
    xp[..., :Cin] = x.transpose(0, 2, 3, 1)
    vi, vw = place(xp, offs.get("inp", 0)), place(packed_weight(w), offs.get("weight", 0))
    vsc = place(scale, offs.get("scale", 0)) if scale is not None else None
    vsh = place(shift, offs.get("shift", 0)) if shift is not None else None
    vr = place(_dev(residual, "nhwc"), offs.get("residual", 0)) if residual is not None else None
    vo = place_out(B * Cout * ho * wo * 4, offs.get("out", 0))
    ep = L.Epilogue(vsc.ptr if vsc else None, vsh.ptr if vsh else None, vr.ptr if vr else None, int(relu))
    must("rn_conv2d_nhwc_forward", vi.ptr, vo.ptr, vw.ptr, k, s, p, ho, wo, B, Cin, Cout, H, W, ctypes.byref(ep))
    check_guards(what, vi, vw, vsc, vsh, vr)
    return _host(fetch(vo, np.float32, what), (B, Cout, ho, wo), "nhwc")


def conv_nhwc_is_direct(Cin, k, offs):
    """rn_conv2d_nhwc_forward: the contraction needs in_channels % 32 == 0 (or the small-Cin stem form) and
    EVERY operand, the epilogue's included, on a 16-byte boundary; otherwise the element-wise kernel."""
    c4 = Cin <= 4 and k <= 8
    return not (Cin % 32 == 0 or c4) or k > 15 or any(v % 16 for v in offs.values())


def run_conv2d(x, w, s, p, layout, taps, offs):
    """rn_conv2d_forward (the reference's signature) with the context in `layout` and rn_ctx_set_nchw_taps(taps)."""
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    what = f"rn_conv2d_forward {layout} taps={taps} {x.shape} w={w.shape} s={s} p={p} offs={offs}"
    ho, wo = out_size(H, k, s, p), out_size(W, k, s, p)
    vi, vw = place(_dev(x, layout), offs.get("inp", 0)), place(w, offs.get("weight", 0))
    vo = place_out(B * Cout * ho * wo * 4, offs.get("out", 0))
    ctx = R.get_ctx()
    ctx.set_nchw_taps(taps)
    try:
        must("rn_conv2d_forward", vi.ptr, vo.ptr, vw.ptr, k, s, p, ho, wo, B, Cin, Cout, H, W, layout=layout)
    finally:
        ctx.set_nchw_taps(1)
    check_guards(what, vi, vw)
    return _host(fetch(vo, np.float32, what), (B, Cout, ho, wo), layout)


def conv2d_is_direct(case, layout, taps, offs):
    """The route rule of rn_conv2d_forward (include/rn_hip.h, "Alignment"): the NCHW-native kernel (1x1 /
    padding 0 with a weight on a 16-byte boundary, or k x k with the taps gathered) takes any 4-byte-aligned
    tensor; the NHWC contraction needs its caller-side operands on 16-byte boundaries (NHWC context: inp and
    out; NCHW context, transposing route: out), otherwise the direct kernel runs."""
    B, Cin, Cout, H, W, k, s, p = case
    if not (Cin % 32 == 0 or (Cin <= 4 and k <= 8)) or (layout == "nhwc" and Cin < 4):
        return True
    native = layout == "nchw" and Cin % 32 == 0 and k <= 7 and p <= 7 and s <= 8
    if native and k == 1 and p == 0 and offs.get("weight", 0) % 16 == 0:
        return False
    if native and (taps >= 2 or (taps == 1 and H * W >= 2048)):
        return False
    wide = (offs.get("inp", 0) | offs.get("out", 0)) if layout == "nhwc" else offs.get("out", 0)
    return wide % 16 != 0


def run_argmax(logits, offs):
    what = f"rn_argmax_forward {logits.shape} offs={offs}"
    B, C = logits.shape
    vi, vo = place(logits, offs.get("logits", 0)), place_out(B * 8, offs.get("idx", 0))
    must("rn_argmax_forward", vi.ptr, vo.ptr, B, C)
    check_guards(what, vi)
    return fetch(vo, np.uint64, what).astype(np.int64)


def offset_configs(names, offsets=(4, 8, 12)):
    """The all-aligned control, then for every offset each operand on its own and all of them together."""
    cfgs = [{}]
    for off in offsets:
        cfgs += [{n: off} for n in names]
        if len(names) > 1:
            cfgs.append({n: off for n in names})
    return cfgs
