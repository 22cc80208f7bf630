"""Exact-integer geometry sweep: operands, int64 reference, geometry lists and edge classes (no GPU, no kernel).

The window geometry (H, W, k, stride, pad, dilation) is computed independently by every k x k convolution
route (row-major masks, the DIL instantiation, the pixel-major walk, the bf16 wide tiles and the strip ring, the
grouped super-group masks, the direct kernels, the NCHW gather).  On small-integer operands every partial sum is
an exactly representable integer in any summation order, so every route must return the int64 reference bit for
bit: tests/test_geometry_gpu.py compares with np.array_equal, tests/test_geometry_host.py shows on the CPU that
the lists below reach every edge class a route's domain admits and tell wrong window arithmetic apart.

  operands(case, seed)      x in [-3, 3]; w: per (output channel, tap) exactly two input channels of its group
                            with +-1 (one when Cg == 1); scale in {1, 2, -1}; shift in [-4, 4]; residual in [-8, 8]
  reference(...)            convolution + epilogue in int64, numpy only
  exact_bound(...)          the same expression on absolute values: < 256 where bf16 is stored, < 2**24 otherwise
  geometries(route)         deterministic list of (B, H, W, k, s, p, d)
  edge_classes(H, W, ...)   the classes a geometry hits, from the window arithmetic alone
  emulate(..., flaw)        a gather-style convolution with one deliberate mistake in its window arithmetic
  first_difference(...)     the message of a failure: output pixel, channel, got, want, edge classes
"""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "B Cin Cout G H W k s p d")

CLASSES = ("clip_lo", "clip_hi", "clip_both", "lo_without_hi", "leftover", "out_one", "in_one", "single_tap",
           "deep_pad", "no_pad", "axes_differ", "next_image")

# (B, H, W): H = 1, W = 1, W = 2, H != W, odd and even sides up to 9, B >= 2
PLANES = ((1, 1, 1), (1, 1, 5), (2, 5, 1), (1, 2, 2), (2, 3, 2), (1, 3, 3), (1, 4, 7), (2, 5, 4), (1, 6, 6),
          (2, 7, 5), (1, 8, 9), (2, 9, 9), (3, 2, 5), (1, 9, 3))
# the strip kernel: 3x3 / stride 1 / pad 1 on planes with H, W in {1, 2, 3, 5, 8}, B in {1, 3}
STRIP_PLANES = tuple((B, H, W) for B in (1, 3) for H in (1, 2, 3, 5, 8) for W in (1, 2, 3, 5, 8))

ROUTES = ("row_major", "dil", "pixel_major", "bf16_tile", "bf16_wide", "bf16_strip", "grouped", "direct", "nchw")
MFMA_ROUTES = ROUTES[:7]
CAP = 96      # geometries per route


def _domain(route):
    """the (k, s, p, d) a route is swept over"""
    if route == "row_major":
        return [(k, s, p, 1) for k in (2, 3, 4, 5, 7) for s in (1, 2, 3) for p in range(k + 1)]
    if route == "dil":      # p != d included; d >= H and W < span come from the small planes
        return [(k, s, p, d) for k in (2, 3, 5) for d in (2, 3) for s in (1, 2) for p in sorted({0, 1, d, d + 1, d * (k - 1)})
                if d * (k - 1) + 1 <= 9 + 2 * p]     # (the span fits the largest plane)
    if route == "pixel_major":
        return [(k, s, p, 1) for k in (2, 3, 5) for s in (1, 2, 3) for p in range(1, k)]
    if route in ("bf16_tile", "bf16_wide"):
        return [(k, s, p, d) for k in (2, 3) for d in (1, 2) for s in (1, 2, 3) for p in range(0, d * (k - 1) + 2)]
    if route == "bf16_strip":
        return [(3, 1, 1, 1)]
    if route == "grouped":
        return [(3, s, p, d) for s in (1, 2, 3) for p in range(4) for d in (1, 2, 3)]
    if route == "direct":
        return [(k, s, p, d) for k in (1, 2, 3, 4) for d in (1, 2) for s in (1, 2) for p in range(3) if k > 1 or d == 1]
    if route == "nchw":
        return [(k, s, p, 1) for k in (2, 3, 5) for s in (1, 2, 3) for p in range(k + 1)]
    raise KeyError(route)


def out_size(n, k, s, p, d=1):
    span = d * (k - 1) + 1
    return (n + 2 * p - span) // s + 1 if n + 2 * p >= span else 0


def _axis_classes(n, k, s, p, d):
    span = d * (k - 1) + 1
    out = out_size(n, k, s, p, d)
    got = set()
    starts = [o * s - p for o in range(out)]
    lo = [x0 < 0 for x0 in starts]
    hi = [x0 + span - 1 >= n for x0 in starts]
    inside = [sum(0 <= x0 + t * d < n for t in range(k)) for x0 in starts]
    if any(lo):
        got.add("clip_lo")
    if any(hi):
        got.add("clip_hi")
    if any(a and b for a, b in zip(lo, hi)):
        got.add("clip_both")
    if p > 0 and not any(hi):
        got.add("lo_without_hi")
    if (n + 2 * p - span) % s != 0:
        got.add("leftover")
    if out == 1:
        got.add("out_one")
    if n == 1:
        got.add("in_one")
    if any(i == 1 for i in inside):
        got.add("single_tap")
    if 2 * p > span - 1:
        got.add("deep_pad")
    if p == 0:
        got.add("no_pad")
    return got


def edge_classes(H, W, k, s, p, d, B=1):
    """the names of CLASSES this geometry hits (a frozenset): the union over rows and columns, `axes_differ`
    where the two axes' sets differ, `next_image` for B >= 2 with a clipped window"""
    rows, cols = _axis_classes(H, k, s, p, d), _axis_classes(W, k, s, p, d)
    got = rows | cols
    if rows != cols:
        got.add("axes_differ")
    if B >= 2 and got & {"clip_lo", "clip_hi"}:
        got.add("next_image")
    return frozenset(got)


def classes_of(geom):
    B, H, W, k, s, p, d = geom
    return edge_classes(H, W, k, s, p, d, B)


@functools.lru_cache(maxsize=None)
def geometries(route):
    """(B, H, W, k, s, p, d): the route's domain crossed with the planes, valid output sizes only, at most CAP of
    them.  Kept, in this order: for every edge class the first geometry that hits it, one plane for every
    (k, s, p, d) of the domain (walking through the planes), then an even stride through the rest."""
    planes = STRIP_PLANES if route == "bf16_strip" else PLANES
    full = [(B, H, W, k, s, p, d) for (k, s, p, d) in _domain(route) for (B, H, W) in planes
            if out_size(H, k, s, p, d) >= 1 and out_size(W, k, s, p, d) >= 1]
    if route == "pixel_major":      # eligible only when every output pixel has a tap inside the image
        full = [g for g in full if _every_window_has_a_tap(g)]
    keep, seen = [], set()

    def add(g):
        if g not in seen and len(keep) < CAP:
            seen.add(g)
            keep.append(g)

    for c in CLASSES:
        for g in full:
            if c in classes_of(g):
                add(g)
                break
    by_dom = collections.OrderedDict()
    for g in full:
        by_dom.setdefault(g[3:], []).append(g)
    for i, gs in enumerate(by_dom.values()):
        add(gs[(5 * i) % len(gs)])
    rest = [g for g in full if g not in seen]
    room = CAP - len(keep)
    if room > 0 and rest:
        step = max(1, len(rest) // room)
        for g in rest[::step]:
            add(g)
    return tuple(keep)


def _every_window_has_a_tap(geom):
    B, H, W, k, s, p, d = geom
    for n in (H, W):
        for o in range(out_size(n, k, s, p, d)):
            if not any(0 <= o * s - p + t * d < n for t in range(k)):
                return False
    return True


def representatives(route, k_min=0):
    """one listed geometry (of kernel size k_min or more) per edge class the list hits: {class: geometry}"""
    reps = {}
    for g in geometries(route):
        if g[3] >= k_min:
            for c in classes_of(g):
                reps.setdefault(c, g)
    return reps


def class_table():
    """{route: {class: count of listed geometries that hit it}}"""
    return {r: {c: sum(c in classes_of(g) for g in geometries(r)) for c in CLASSES} for r in ROUTES}


def format_table(table):
    w = max(len(r) for r in table) + 1
    lines = [" " * w + " ".join(f"{c[:9]:>9}" for c in CLASSES) + "   listed"]
    for r, row in table.items():
        lines.append(f"{r:<{w}}" + " ".join(f"{row[c]:>9}" for c in CLASSES) + f"   {len(geometries(r)):>6}")
    return "\n".join(lines)


# (Cin, Cout, groups) per route.  grouped: Cg = 1, 2, 4 (nq = 1, the block-diagonal pack; Cg = 1 is depthwise), 32, 64
# and 96 (nq = 1, 2, 3); direct: Cin = 5 has no whole channel segment, (24 -> 36, G = 12) is no super-group shape.
CHANNELS = {"row_major": ((32, 40, 1),), "dil": ((32, 40, 1),), "pixel_major": ((32, 40, 1),), "bf16_tile": ((64, 40, 1),),
            "bf16_wide": ((64, 40, 1),), "bf16_strip": ((64, 64, 1), (128, 128, 1)),
            "grouped": ((32, 32, 32), (64, 64, 32), (128, 128, 32), (64, 64, 2), (128, 128, 2), (192, 192, 2)),
            "direct": ((5, 7, 1), (24, 36, 12)), "nchw": ((32, 40, 1),)}


@functools.lru_cache(maxsize=None)
def cases(route):
    """every Case the GPU sweep launches for the route: the listed geometries on each channel configuration; for
    the pixel-major route also every third geometry at B = 66 (a second image block at BM 64); for the pixel-major
    and the row-major route the edge-class representatives at Cin 128 as well (k = 3: 36 K tiles, the chunked K
    sum, whose fold points fall inside taps that the pixel-major walk skips)"""
    out = [Case(B, cin, cout, G, H, W, k, s, p, d) for (cin, cout, G) in CHANNELS[route]
           for (B, H, W, k, s, p, d) in geometries(route)]
    if route == "pixel_major":
        out += [Case(66, 32, 40, 1, H, W, k, s, p, d) for (B, H, W, k, s, p, d) in geometries(route)[::3]]
    if route in ("pixel_major", "row_major"):
        reps = sorted(set(representatives(route, k_min=3).values()), key=geometries(route).index)      # 36+ K tiles
        out += [Case(B, 128, 40, 1, H, W, k, s, p, d) for (B, H, W, k, s, p, d) in reps]
    return tuple(out)


def geom_of(case):
    c = Case(*case)
    return (c.B, c.H, c.W, c.k, c.s, c.p, c.d)


def seed_of(case):
    return 1 + sum((i + 1) * int(v) for i, v in enumerate(case))


# ---- operands -------------------------------------------------------------------------------------------------
def operands(case, seed, epilogue=True):
    """x [B,Cin,H,W], w [Cout,Cin/G,k,k], scale, shift [Cout], residual [B,Cout,Ho,Wo] as float32 arrays holding
    small integers (module docstring); scale = shift = residual = None without `epilogue`"""
    c = Case(*case)
    g = np.random.default_rng(seed)
    cg = c.Cin // c.G
    x = g.integers(-3, 4, (c.B, c.Cin, c.H, c.W)).astype(np.float32)
    w = np.zeros((c.Cout, cg, c.k, c.k), dtype=np.float32)
    nz = min(2, cg)
    o, kh, kw = np.meshgrid(np.arange(c.Cout), np.arange(c.k), np.arange(c.k), indexing="ij")
    # per (output channel, tap) `nz` distinct channels: the nz smallest of a random permutation's ranks
    ch = np.argsort(g.random((c.Cout, c.k, c.k, cg)), axis=-1)[..., :nz]
    sign = g.choice(np.float32([-1, 1]), (c.Cout, c.k, c.k, nz))
    for j in range(nz):
        w[o, ch[..., j], kh, kw] = sign[..., j]
    if not epilogue:
        return x, w, None, None, None
    scale = g.choice(np.float32([1, 2, -1]), c.Cout)
    shift = g.integers(-4, 5, c.Cout).astype(np.float32)
    ho, wo = out_size(c.H, c.k, c.s, c.p, c.d), out_size(c.W, c.k, c.s, c.p, c.d)
    residual = g.integers(-8, 9, (c.B, c.Cout, ho, wo)).astype(np.float32)
    return x, w, scale, shift, residual


def _i64(a):
    a = np.asarray(a)
    r = np.rint(a).astype(np.int64)
    assert np.array_equal(r, a), "operands must hold integers"
    return r


def _conv_i64(x, w, s, p, d, G):
    """zero-padded image, one strided slice per tap, one einsum over the groups' channels per tap"""
    B, Cin, H, W = x.shape
    Cout, cg, k, _ = w.shape
    assert Cin == cg * G and Cout % G == 0
    ho, wo = out_size(H, k, s, p, d), out_size(W, k, s, p, d)
    assert ho >= 1 and wo >= 1
    xp = np.zeros((B, Cin, H + 2 * p, W + 2 * p), dtype=np.int64)
    xp[:, :, p:p + H, p:p + W] = x
    out = np.zeros((B, G, Cout // G, ho, wo), dtype=np.int64)
    wg = w.reshape(G, Cout // G, cg, k, k)
    for kh in range(k):
        for kw in range(k):
            patch = xp[:, :, kh * d:kh * d + (ho - 1) * s + 1:s, kw * d:kw * d + (wo - 1) * s + 1:s]
            out += np.einsum("bgchw,goc->bgohw", patch.reshape(B, G, cg, ho, wo), wg[:, :, :, kh, kw])
    return out.reshape(B, Cout, ho, wo)


def _epilogue_i64(y, scale, shift, residual, relu):
    if scale is not None:
        y = y * scale[None, :, None, None]
    if shift is not None:
        y = y + shift[None, :, None, None]
    if residual is not None:
        y = y + residual
    return np.maximum(y, 0) if relu else y


def reference(x, w, s, p, d=1, G=1, scale=None, shift=None, residual=None, relu=False):
    """int64 [B,Cout,Ho,Wo]: relu(conv(x, w) * scale + shift + residual), every part optional"""
    opt = lambda a: None if a is None else _i64(a)
    return _epilogue_i64(_conv_i64(_i64(x), _i64(w), s, p, d, G), opt(scale), opt(shift), opt(residual), relu)


def exact_bound(x, w, s, p, d=1, G=1, scale=None, shift=None, residual=None):
    """the largest value of the reference's expression on absolute values (no ReLU): every partial sum of every
    summation order, and the fused multiply-add of the epilogue, stay below it in magnitude"""
    a = lambda t: None if t is None else np.abs(_i64(t))
    return int(_epilogue_i64(_conv_i64(a(x), a(w), s, p, d, G), a(scale), a(shift), a(residual), False).max())


# ---- a second, gather-style convolution, with deliberate mistakes -------------------------------------------------
FLAWS = ("no_far_clip", "next_image", "ceil_size", "dilate_rows_only")


def emulate(x, w, s, p, d=1, G=1, flaw=None):
    """The convolution as a kernel computes it: a flat NHWC address per (output pixel, tap), a validity test, a
    gather.  flaw None is correct (held to `reference` in tests/test_geometry_host.py);
      no_far_clip        only `>= 0` is tested: a window past the right / bottom edge reads the next row / image
      next_image         rows are tested against the whole batch, not the image: padding rows read the neighbour
      ceil_size          the output size rounds up: the leftover rows get an output of their own
      dilate_rows_only   kernel columns are 1 apart, kernel rows d apart
    An address outside the whole tensor reads 0, as a bounds-checked buffer load does."""
    x, w = _i64(x), _i64(w)
    B, Cin, H, W = x.shape
    Cout, cg, k, _ = w.shape
    dh, dw = d, (1 if flaw == "dilate_rows_only" else d)
    ho, wo = out_size(H, k, s, p, d), out_size(W, k, s, p, d)
    if flaw == "ceil_size":
        span = d * (k - 1) + 1
        ho, wo = -(-(H + 2 * p - span) // s) + 1, -(-(W + 2 * p - span) // s) + 1
    flat = np.concatenate([x.transpose(0, 2, 3, 1).reshape(B * H * W, Cin), np.zeros((1, Cin), np.int64)])
    b = np.arange(B)[:, None, None]
    oh, ow = np.arange(ho)[None, :, None], np.arange(wo)[None, None, :]
    out = np.zeros((B, ho, wo, G, Cout // G), dtype=np.int64)
    wg = w.reshape(G, Cout // G, cg, k, k)
    for kh in range(k):
        for kw in range(k):
            ih, iw = oh * s - p + kh * dh + 0 * ow, ow * s - p + kw * dw + 0 * oh
            if flaw == "no_far_clip":
                ok = (ih >= 0) & (iw >= 0)
            elif flaw == "next_image":
                ok = (b * H + ih >= 0) & (b * H + ih < B * H) & (iw >= 0) & (iw < W)
            else:
                ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
            addr = (b * H + ih) * W + iw
            ok = ok & (addr >= 0) & (addr < B * H * W)
            patch = flat[np.where(ok, addr, B * H * W)]
            out += np.einsum("bhwgc,goc->bhwgo", patch.reshape(B, ho, wo, G, cg), wg[:, :, :, kh, kw])
    return out.reshape(B, ho, wo, Cout).transpose(0, 3, 1, 2)


# ---- the message of a failure -----------------------------------------------------------------------------------
def first_difference(got, want, geom, what=""):
    """None when got == want element for element (same shape); otherwise the text that names the first differing
    element: output pixel, channel, got, want, how many differ, and the geometry's edge classes"""
    got, want = np.asarray(got), np.asarray(want)
    names = ", ".join(sorted(classes_of(geom)))
    head = f"{what}: geometry (B, H, W, k, s, p, d) = {tuple(geom)} [{names}]"
    if got.shape != want.shape:
        return f"{head}: shape {got.shape}, reference {want.shape}"
    bad = np.argwhere(~(got == want))       # (a NaN differs)
    if bad.size == 0:
        return None
    b, c, oh, ow = (int(v) for v in bad[0])
    return (f"{head}: {len(bad)} of {got.size} elements differ, the first at image {b}, output pixel (oh, ow) = "
            f"({oh}, {ow}), channel {c}: got {float(got[b, c, oh, ow])!r}, want {float(want[b, c, oh, ow])!r}")
