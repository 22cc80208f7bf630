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

Contractions get a wider guard behind and before their OUTPUT.  A tile that does not start at column 0 and runs
one row past the tensor begins `col * es` bytes past the last element, so with rows longer than 256 bytes the
default guard can miss it entirely.  The typed runners (`run_conv_dt` and the ones after it) therefore pass
guard_bytes = 256 rows x the row bytes of that output, rounded up to 16 (`contraction_guard`): 256 rows is the
tallest tile any kernel here computes, so a whole tile written one tile height too far still lands in the guard.
That is a few hundred KB at the shapes of test_schedules_gpu.py.

`fetch(..., written=True)` adds the written-everywhere check: no element of the tensor part may still hold the
0xA5 fill (`unwritten`).  It is a condition, not a measurement: a legitimately written element equals the fill
only if the kernel's value is exactly fp32 0xA5A5A5A5 or bf16 0xA5A5 (-2.87e-16), which is negative and so
impossible behind a ReLU; a caller without a ReLU asserts on the CPU that its reference holds no such element
(`assert_no_poison`) before it trusts the check.

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


def unwritten(raw_bytes, elem_size):
    """The indices of the elements of `elem_size` bytes whose bytes ALL still hold the output fill."""
    b = np.ascontiguousarray(raw_bytes).reshape(-1).view(np.uint8)
    assert b.size % elem_size == 0
    return np.flatnonzero((b.reshape(-1, elem_size) == OUT_BYTE).all(axis=1))


def check_written(raw_bytes, elem_size, what="", row=None):
    """Raises when `unwritten` finds an element; `row` = elements per row, to name (row, channel) as well."""
    idx = unwritten(raw_bytes, elem_size)
    if idx.size:
        first, last = int(idx[0]), int(idx[-1])
        at = f" = (row, channel) {divmod(first, row)} .. {divmod(last, row)}" if row else ""
        raise AssertionError(f"{what}: {idx.size} elements never written (still 0x{OUT_BYTE:02X} bytes), "
                             f"the first at index {first}, the last at {last}{at}")


def assert_no_poison(ref, bf16, what=""):
    """The reference, rounded to the output's element type, holds no element with the fill's bit pattern."""
    from resnet_c_amd import ops
    bits = ops.to_bf16_bits(np.asarray(ref, dtype=np.float32)) if bf16 else np.asarray(ref, dtype=np.float32)
    assert unwritten(bits, 2 if bf16 else 4).size == 0, f"{what}: the reference itself holds the fill pattern"


def contraction_guard(row_bytes):
    """256 rows (the tallest tile) of the output, rounded up to 16 bytes: see the module docstring."""
    return -(-256 * row_bytes // 16) * 16


def fetch(view, dtype=np.float32, what="", written=False, row=None):
    """The tensor part of the view, after checking both guards byte for byte; written=True: and that no
    element of it still holds the output fill (`row`: elements per row, for the message)."""
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
    if written:
        check_written(whole[lo:hi], np.dtype(dtype).itemsize, what, row)
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


def run_conv2d(x, w, s, p, layout, taps, offs, guard_bytes=GUARD):
    """rn_conv2d_forward (the reference's signature) with the context in `layout` and rn_ctx_set_nchw_taps(taps);
    every element of the output must come back written (fetch(written=True); `guard_bytes`: the guard around the
    output).  That holds for every caller, test_views_gpu.py and tests/fuzz/view_fuzz.py included; their references
    have no ReLU and are not searched for the fill pattern: a random fp32 result is 0xA5A5A5A5 with probability
    2**-32 per element, and a hit would fail the run, not pass it."""
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    what = f"rn_conv2d_forward {layout} taps={taps} {x.shape} w={w.shape} s={s} p={p} offs={offs}"
    ho, wo = out_size(H, k, s, p), out_size(W, k, s, p)
    vi, vw = place(_dev(x, layout), offs.get("inp", 0)), place(w, offs.get("weight", 0))
    vo = place_out(B * Cout * ho * wo * 4, offs.get("out", 0), guard_bytes)
    ctx = R.get_ctx()
    ctx.set_nchw_taps(taps)
    try:
        must("rn_conv2d_forward", vi.ptr, vo.ptr, vw.ptr, k, s, p, ho, wo, B, Cin, Cout, H, W, layout=layout)
    finally:
        ctx.set_nchw_taps(1)
    check_guards(what, vi, vw)
    return _host(fetch(vo, np.float32, what, written=True, row=Cout if layout == "nhwc" else None), (B, Cout, ho, wo), layout)


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


# ---- the element-type tagged entry points (contractions, chains, the fused stem) -------------------------
# `launch_*` places every operand and makes the ONE call; it returns ((status, message), output views, input
# views) so that test_views_gpu.py can look at a refusal.  `run_*` asserts RN_OK, checks every guard and fetches
# the outputs with written=True.  Host arrays are NCHW fp32 (rows x channels for the chains); bf16 operands are
# uploaded as ops.to_bf16_bits of them and bf16 results come back widened to fp32 (exact).
def _bf(dt):
    return dt == L.RN_DTYPE_BF16


def _es(dt):
    return 2 if _bf(dt) else 4


def _np(dt):
    return np.uint16 if _bf(dt) else np.float32


def _typed(a, dt):
    from resnet_c_amd import ops
    a = np.ascontiguousarray(a, dtype=np.float32)
    return ops.to_bf16_bits(a) if _bf(dt) else a


def _act(a, dt):
    """NCHW host array -> the device's NHWC image in `dt`"""
    return _typed(np.asarray(a, dtype=np.float32).transpose(0, 2, 3, 1), dt)


def _widen(flat, dt):
    from resnet_c_amd import ops
    return ops.from_bf16_bits(flat) if _bf(dt) else flat


def _f32(v, off):
    return place(np.asarray(v, dtype=np.float32), off) if v is not None else None


def _ptr(v):
    return v.ptr if v is not None else None


def place_result(rows, row_elems, dt, offset_bytes=0):
    """A poisoned output of rows x row_elems elements between contraction-width guards."""
    return place_out(rows * row_elems * _es(dt), offset_bytes, contraction_guard(row_elems * _es(dt)))


def fetch_result(view, shape_nchw, dt, what):
    """guards, written-everywhere, then the NHWC result as an NCHW fp32 host array"""
    B, C, H, W = shape_nchw
    flat = _widen(fetch(view, _np(dt), what, written=True, row=C), dt)
    return flat.reshape(B, H, W, C).transpose(0, 3, 1, 2).copy()


def packed_weight_dt(w, dt):
    """rn_conv2d_pack_weight_dt of an OIHW weight: the panel as the device holds it (fp32 or bf16 bits)"""
    Cout, Cin, k, _ = w.shape
    n = int(L.lib().rn_conv2d_packed_weight_numel_dt(dt, Cin, Cout, k))
    vw, vp = place(np.asarray(w, dtype=np.float32)), place_out(n * _es(dt))
    must("rn_conv2d_pack_weight_dt", dt, vw.ptr, vp.ptr, Cin, Cout, k)
    return fetch(vp, _np(dt), f"rn_conv2d_pack_weight_dt {w.shape}")


def packed_pair_weight_dt(w, scale, w2, scale2, dt):
    """rn_conv2d_pack_weight_pair_dt: both weights, their scales folded in, as one panel"""
    Cout, Cin, k, _ = w.shape
    Cin2 = w2.shape[1]
    n = int(L.lib().rn_conv2d_packed_pair_weight_numel(Cin, Cout, k, Cin2))
    v1, v2, vp = place(np.asarray(w, dtype=np.float32)), place(np.asarray(w2, dtype=np.float32)), place_out(n * _es(dt))
    vs1, vs2 = _f32(scale, 0), _f32(scale2, 0)
    must("rn_conv2d_pack_weight_pair_dt", dt, v1.ptr, _ptr(vs1), v2.ptr, _ptr(vs2), vp.ptr, Cin, Cout, k, Cin2)
    return fetch(vp, _np(dt), f"rn_conv2d_pack_weight_pair_dt {w.shape} + {w2.shape}")


def launch_conv_dt(x, w, s, p, scale, shift, residual, relu, dt_in, dt_out, offs=None):
    """rn_conv2d_nhwc_forward_dt (in_channels a multiple of the 128-byte channel segment): f32 -> f32,
    bf16 -> bf16 or bf16 -> f32; the residual has the output's element type."""
    offs = offs or {}
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    assert Cin % (128 // _es(dt_in)) == 0, "whole channel segments (the small-Cin forms pad their image)"
    ho, wo = out_size(H, k, s, p), out_size(W, k, s, p)
    vi, vw = place(_act(x, dt_in), offs.get("inp", 0)), place(packed_weight_dt(w, dt_in), offs.get("weight", 0))
    vsc, vsh = _f32(scale, offs.get("scale", 0)), _f32(shift, offs.get("shift", 0))
    vr = place(_act(residual, dt_out), offs.get("residual", 0)) if residual is not None else None
    vo = place_result(B * ho * wo, Cout, dt_out, offs.get("out", 0))
    ep = L.Epilogue(_ptr(vsc), _ptr(vsh), _ptr(vr), int(relu))
    st = call("rn_conv2d_nhwc_forward_dt", dt_in, dt_out, vi.ptr, vo.ptr, vw.ptr, k, s, p, ho, wo, B, Cin, Cout, H, W,
              ctypes.byref(ep))
    return st, [vo], [vi, vw, vsc, vsh, vr]


def _ok(name, st):
    assert st[0] == L.RN_OK, f"{name}: status {st[0]} ({st[1]})"


def run_conv_dt(x, w, s, p, scale, shift, residual, relu, dt_in, dt_out, offs=None):
    B, _, H, W = x.shape
    Cout, _, k, _ = w.shape
    what = f"rn_conv2d_nhwc_forward_dt {dt_in}->{dt_out} {x.shape} w={w.shape} s={s} p={p} offs={offs}"
    st, (vo,), ins = launch_conv_dt(x, w, s, p, scale, shift, residual, relu, dt_in, dt_out, offs)
    _ok(what, st)
    check_guards(what, *ins)
    return fetch_result(vo, (B, Cout, out_size(H, k, s, p), out_size(W, k, s, p)), dt_out, what)


def launch_conv_pair_dt(x, w, x2, w2, s, p, stride2, scale, scale2, shift, residual, relu, dt, offs=None):
    """rn_conv2d_nhwc_pair_forward_dt: epilogue(conv(x, w * scale) + conv1x1(x2, w2 * scale2)), one element type"""
    offs = offs or {}
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    _, Cin2, H2, W2 = x2.shape
    ho, wo = out_size(H, k, s, p), out_size(W, k, s, p)
    vi, vi2 = place(_act(x, dt), offs.get("inp", 0)), place(_act(x2, dt), offs.get("second", 0))
    vw = place(packed_pair_weight_dt(w, scale, w2, scale2, dt), offs.get("weight", 0))
    vsh = _f32(shift, offs.get("shift", 0))
    vr = place(_act(residual, dt), offs.get("residual", 0)) if residual is not None else None
    vo = place_result(B * ho * wo, Cout, dt, offs.get("out", 0))
    ep, second = L.Epilogue(None, _ptr(vsh), _ptr(vr), int(relu)), L.ConvSecond(vi2.ptr, Cin2, H2, W2, stride2)
    st = call("rn_conv2d_nhwc_pair_forward_dt", dt, dt, vi.ptr, vo.ptr, vw.ptr, k, s, p, ho, wo, B, Cin, Cout, H, W,
              ctypes.byref(second), ctypes.byref(ep))
    return st, [vo], [vi, vi2, vw, vsh, vr]


def run_conv_pair_dt(x, w, x2, w2, s, p, stride2, scale, scale2, shift, residual, relu, dt, offs=None):
    B, _, H, W = x.shape
    Cout, _, k, _ = w.shape
    what = f"rn_conv2d_nhwc_pair_forward_dt {dt} {x.shape} + {x2.shape} -> {Cout} s={s} p={p} stride2={stride2} offs={offs}"
    st, (vo,), ins = launch_conv_pair_dt(x, w, x2, w2, s, p, stride2, scale, scale2, shift, residual, relu, dt, offs)
    _ok(what, st)
    check_guards(what, *ins)
    return fetch_result(vo, (B, Cout, out_size(H, k, s, p), out_size(W, k, s, p)), dt, what)


def launch_chain_dt(t2, x, w3, scale3, shift3, w1, scale1, shift1, dt, pair_w=None, pair_scale=None, offs=None):
    """rn_conv_chain_forward_dt, or with pair_w (the downsample weight; x is then its input x2, scale3 and
    pair_scale are folded into the panel and shift3 is the pair's shift) rn_conv_chain_pair_forward_dt.
    t2 / x: NCHW host arrays; y = [rows][channels] and t1 = [rows][next_mid] are the outputs."""
    offs = offs or {}
    B, mid, H, W = t2.shape
    C, N1, rows = w3.shape[0], w1.shape[0], B * H * W
    vt2, vx = place(_act(t2, dt), offs.get("t2", 0)), place(_act(x, dt), offs.get("x", 0))
    p3 = packed_weight_dt(w3, dt) if pair_w is None else packed_pair_weight_dt(w3, scale3, pair_w, pair_scale, dt)
    vw3, vw1 = place(p3, offs.get("w3", 0)), place(packed_weight_dt(w1, dt), offs.get("w1", 0))
    vsc3 = _f32(scale3, offs.get("scale3", 0)) if pair_w is None else None
    vsh3 = _f32(shift3, offs.get("shift3", 0))
    vsc1, vsh1 = _f32(scale1, offs.get("scale1", 0)), _f32(shift1, offs.get("shift1", 0))
    vy, vt1 = place_result(rows, C, dt, offs.get("y", 0)), place_result(rows, N1, dt, offs.get("t1", 0))
    if pair_w is None:
        st = call("rn_conv_chain_forward_dt", dt, vt2.ptr, vx.ptr, vy.ptr, vw3.ptr, _ptr(vsc3), _ptr(vsh3), vt1.ptr,
                  vw1.ptr, _ptr(vsc1), _ptr(vsh1), rows, mid, C, N1)
    else:
        st = call("rn_conv_chain_pair_forward_dt", dt, vt2.ptr, vx.ptr, vy.ptr, vw3.ptr, _ptr(vsh3), vt1.ptr, vw1.ptr,
                  _ptr(vsc1), _ptr(vsh1), rows, mid, x.shape[1], C, N1)
    return st, [vy, vt1], [vt2, vx, vw3, vw1, vsc3, vsh3, vsc1, vsh1]


def run_chain_dt(t2, x, w3, scale3, shift3, w1, scale1, shift1, dt, pair_w=None, pair_scale=None, offs=None):
    """(y, t1) as NCHW fp32 host arrays, both checked for guards and written-everywhere"""
    B, _, H, W = t2.shape
    C, N1 = w3.shape[0], w1.shape[0]
    what = f"rn_conv_chain{'_pair' if pair_w is not None else ''}_forward_dt {dt} {t2.shape} -> {C} -> {N1} offs={offs}"
    st, (vy, vt1), ins = launch_chain_dt(t2, x, w3, scale3, shift3, w1, scale1, shift1, dt, pair_w, pair_scale, offs)
    _ok(what, st)
    check_guards(what, *ins)
    return fetch_result(vy, (B, C, H, W), dt, what + ": y"), fetch_result(vt1, (B, N1, H, W), dt, what + ": t1")


def stem_out_sizes(H, W):
    ho, wo = out_size(H, 7, 2, 3), out_size(W, 7, 2, 3)
    return ho, wo, out_size(ho, 3, 2, 1), out_size(wo, 3, 2, 1)


def launch_stem_pool(form, x, w, scale, shift, dt, offs=None):
    """form "padded": rn_stem_pool_forward_dt on the bordered NHWC image (3 channels in fp32, 4 in bf16);
    "nchw": rn_stem_pool_nchw_forward_dt on the fp32 NCHW image; "y": rn_stem_conv_pool_nchw_forward (fp32),
    which also writes the stem tensor -- outputs [pooled, stem tensor]."""
    offs = offs or {}
    B, Cin, H, W = x.shape
    ho, wo, ph, pw = stem_out_sizes(H, W)
    n = int(L.lib().rn_stem_pool_packed_weight_numel(dt))
    v0, vp = place(np.asarray(w, dtype=np.float32)), place_out(n * _es(dt))
    must("rn_stem_pool_pack_weight_dt", dt, v0.ptr, vp.ptr, Cin)
    vw = place(fetch(vp, _np(dt), "rn_stem_pool_pack_weight_dt"), offs.get("weight", 0))
    vsc, vsh = _f32(scale, offs.get("scale", 0)), _f32(shift, offs.get("shift", 0))
    vo = place_result(B * ph * pw, 64, dt, offs.get("out", 0))
    if form == "y":
        assert not _bf(dt)
        vi, vy = place(np.asarray(x, dtype=np.float32), offs.get("inp", 0)), place_result(B * ho * wo, 64, dt, offs.get("y", 0))
        st = call("rn_stem_conv_pool_nchw_forward", vi.ptr, vy.ptr, vo.ptr, vw.ptr, _ptr(vsc), _ptr(vsh), B, Cin, H, W)
        return st, [vo, vy], [vi, vw, vsc, vsh]
    if form == "nchw":
        vi = place(np.asarray(x, dtype=np.float32), offs.get("inp", 0))
        st = call("rn_stem_pool_nchw_forward_dt", dt, vi.ptr, vo.ptr, vw.ptr, _ptr(vsc), _ptr(vsh), 1, B, Cin, H, W)
        return st, [vo], [vi, vw, vsc, vsh]
    vi = place(_typed(pad_reference(np.asarray(x, dtype=np.float32), 4 if _bf(dt) else 3, 3), dt), offs.get("inp", 0))
    st = call("rn_stem_pool_forward_dt", dt, vi.ptr, vo.ptr, vw.ptr, _ptr(vsc), _ptr(vsh), 1, B, H + 6, W + 6)
    return st, [vo], [vi, vw, vsc, vsh]


def run_stem_pool(form, x, w, scale, shift, dt, offs=None):
    """The pooled tensor [B,64,PH,PW]; form "y": (pooled, stem tensor [B,64,Ho,Wo]).  NCHW fp32 host arrays."""
    B, _, H, W = x.shape
    ho, wo, ph, pw = stem_out_sizes(H, W)
    what = f"fused stem ({form}) {dt} {x.shape} offs={offs}"
    st, outs, ins = launch_stem_pool(form, x, w, scale, shift, dt, offs)
    _ok(what, st)
    check_guards(what, *ins)
    pooled = fetch_result(outs[0], (B, 64, ph, pw), dt, what + ": pooled")
    return (pooled, fetch_result(outs[1], (B, 64, ho, wo), dt, what + ": stem tensor")) if form == "y" else pooled


def offset_configs(names, offsets=(4, 8, 12)):
    """The all-aligned control, then for every offset each operand on its own and all of them together."""
    cfgs = [{}]
    for off in offsets:
        cfgs += [{n: off} for n in names]
        if len(names) > 1:
            cfgs.append({n: off for n in names})
    return cfgs
