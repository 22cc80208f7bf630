"""tests/geometry.py on the CPU: the int64 reference against torch, the exactness condition, the edge classes every
route's list reaches, the pixel-major plan on the listed geometries, and that the lists tell wrong window
arithmetic apart (emulations in the manner of tests/test_written_host.py).  Prints the table route x class."""
import ctypes

import numpy as np
import pytest

import geometry as GEO
import views as V
from resnet_c_amd import _lib as L
from test_dilation_host import conv64
from test_tap_skip_host import invalid_pairs, tile_of

# Classes a route's domain cannot produce, each with its reason; every other class must be hit by the route's list.
EXCLUDED = {
    "row_major": {},
    "dil": {},
    "pixel_major": {"no_pad": "pixel-major requires pad >= 1"},
    "bf16_tile": {},
    "bf16_wide": {},
    "bf16_strip": {"no_pad": "the strip kernel is 3x3 / stride 1 / pad 1 only",
                   "leftover": "stride 1 leaves no row unread",
                   "deep_pad": "pad 1 = (span - 1) / 2",
                   "lo_without_hi": "stride 1 with pad 1: the last window always reaches past the far edge"},
    "grouped": {},
    "direct": {},
    "nchw": {},
}


def test_planes_hold_what_the_sweep_needs():
    P = GEO.PLANES
    assert any(H == 1 for _, H, _ in P) and any(W == 1 for _, _, W in P) and any(W == 2 for _, _, W in P)
    assert any(H != W for _, H, W in P) and any(B >= 2 for B, _, _ in P)
    sides = {n for _, H, W in P for n in (H, W)}
    assert sides >= set(range(1, 10))
    assert {(H, W) for _, H, W in GEO.STRIP_PLANES} == {(h, w) for h in (1, 2, 3, 5, 8) for w in (1, 2, 3, 5, 8)}
    assert {B for B, _, _ in GEO.STRIP_PLANES} == {1, 3}


def test_lists_are_deterministic_valid_and_capped():
    for route in GEO.ROUTES:
        gs = GEO.geometries(route)
        assert 0 < len(gs) <= GEO.CAP and len(set(gs)) == len(gs), route
        assert gs == GEO.geometries.__wrapped__(route), route
        dom = set(GEO._domain(route))
        for (B, H, W, k, s, p, d) in gs:
            assert (k, s, p, d) in dom and GEO.out_size(H, k, s, p, d) >= 1 and GEO.out_size(W, k, s, p, d) >= 1
        assert {g[3:] for g in gs} == dom, f"{route}: a (k, s, p, d) of the domain is on no listed plane"
    # what the issue names for single routes
    assert any(d >= H for (_, H, W, k, s, p, d) in GEO.geometries("dil"))
    assert any(W < d * (k - 1) + 1 for (_, H, W, k, s, p, d) in GEO.geometries("dil"))
    assert any(p != d for (_, H, W, k, s, p, d) in GEO.geometries("dil"))
    assert {c.Cin // c.G for c in GEO.cases("grouped")} == {1, 2, 4, 32, 64, 96}
    pm = GEO.cases("pixel_major")
    assert sum(c.B == 66 for c in pm) >= len(GEO.geometries("pixel_major")) // 3
    for route in ("pixel_major", "row_major"):      # every class of the list again on the chunked K sum (36+ K tiles)
        wide = [c for c in GEO.cases(route) if c.Cin == 128]
        assert all(c.k * c.k * c.Cin // 32 >= 32 and c.Cout % 4 == 0 for c in wide)
        hit = set().union(*(GEO.classes_of(GEO.geom_of(c)) for c in wide))
        assert hit == {c for c in GEO.CLASSES if c not in EXCLUDED[route]}, route


def test_edge_classes_on_hand_worked_geometries():
    ec = GEO.edge_classes
    # 3x3 / 1 / 1 on 1 x 5: rows have one tap inside and are clipped on both sides, columns are not
    got = ec(1, 5, 3, 1, 1, 1)
    assert got == {"clip_lo", "clip_hi", "clip_both", "out_one", "in_one", "single_tap", "axes_differ"}
    # 3x3 / 2 / 1 on 6 x 6: padding at the top and on the left only, one row left over
    assert ec(6, 6, 3, 2, 1, 1) == {"clip_lo", "lo_without_hi", "leftover"}
    # no padding, stride 3 on 7: windows 0-2, 3-5; row 6 unread
    assert ec(7, 7, 3, 3, 0, 1) == {"no_pad", "leftover"}
    # pad 2 > 1, two images
    assert ec(4, 4, 3, 1, 2, 1, B=2) == {"clip_lo", "clip_hi", "deep_pad", "single_tap", "next_image"}
    # dilation 2 on a 3-wide image: span 5 covers it from every position
    assert "clip_both" in ec(3, 3, 3, 1, 2, 2) and "single_tap" in ec(3, 3, 3, 1, 2, 2)


def test_every_route_hits_every_class_its_domain_admits():
    table = GEO.class_table()
    print("\ngeometry: listed geometries per route and edge class\n" + GEO.format_table(table))
    for route in GEO.ROUTES:
        assert set(EXCLUDED[route]) <= set(GEO.CLASSES)
        for c in GEO.CLASSES:
            if c in EXCLUDED[route]:
                assert table[route][c] == 0, f"{route}: {c} was excluded ({EXCLUDED[route][c]}) but is hit"
            else:
                assert table[route][c] > 0, f"{route}: no listed geometry hits {c}"


def _reference_of(case, epilogue):
    c = GEO.Case(*case)
    x, w, sc, sh, res = GEO.operands(c, GEO.seed_of(c), epilogue)
    return c, x, w, sc, sh, res


def test_reference_is_torchs_float64_convolution():
    """every case of the row-major route, and one representative per edge class of every other route"""
    todo = list(GEO.cases("row_major"))
    for route in GEO.ROUTES[1:]:
        reps = set(GEO.representatives(route).values())
        first = {}
        for c in GEO.cases(route):
            if GEO.geom_of(c) in reps:
                first.setdefault((GEO.geom_of(c), c.Cin, c.G) if route in ("grouped", "direct") else GEO.geom_of(c), c)
        todo += list(first.values())
    for case in todo:
        c, x, w, sc, sh, res = _reference_of(case, True)
        raw = GEO.reference(x, w, c.s, c.p, c.d, c.G)
        t64 = conv64(x, w, c.s, c.p, c.d, c.G)
        assert raw.dtype == np.int64 and raw.shape == t64.shape and np.array_equal(raw, t64), case
        assert np.array_equal(GEO.emulate(x, w, c.s, c.p, c.d, c.G), raw), case      # the second implementation
        full = GEO.reference(x, w, c.s, c.p, c.d, c.G, sc, sh, res, True)
        bc = lambda v: v.astype(np.float64)[None, :, None, None]
        assert np.array_equal(full, np.maximum(t64 * bc(sc) + bc(sh) + res, 0)), case
    print(f"\ngeometry: int64 reference == torch float64 on {len(todo)} cases")


@pytest.mark.parametrize("route", GEO.ROUTES)
def test_operands_and_exact_bound(route):
    """the operands are what the module says, and the exactness condition holds for every case of the list"""
    bf16 = route.startswith("bf16")
    worst = 0
    for case in GEO.cases(route):
        c, x, w, sc, sh, res = _reference_of(case, True)
        assert c.k <= (3 if bf16 else 7)
        assert np.abs(x).max() <= 3 and np.array_equal(x, np.rint(x))
        nz = (w != 0).sum(axis=1)
        assert set(np.unique(w)) <= {-1.0, 0.0, 1.0} and (nz == min(2, c.Cin // c.G)).all(), case
        assert set(np.unique(sc)) <= {1.0, 2.0, -1.0} and np.abs(sh).max() <= 4 and np.abs(res).max() <= 8
        bound = GEO.exact_bound(x, w, c.s, c.p, c.d, c.G, sc, sh, res)
        assert bound <= 6 * c.k * c.k * 2 + 12
        assert bound < (256 if bf16 else 2 ** 24), case
        worst = max(worst, bound)
        ref = GEO.reference(x, w, c.s, c.p, c.d, c.G, sc, sh, res, False)
        V.assert_no_poison(ref, bf16, str(case))
    print(f"\ngeometry: {route}: {len(GEO.cases(route))} cases, largest exactness bound {worst}")


def test_pixel_major_plan_on_every_listed_geometry():
    for c in GEO.cases("pixel_major"):
        shape = (c.B, c.Cin, c.Cout, c.H, c.W, c.k, c.s, c.p)
        bad, ho, wo = invalid_pairs(shape)
        for cand in (1, 4):
            sk = ctypes.c_uint64()
            st = L.lib().rn_conv_tap_skip_plan(L.RN_DTYPE_F32, *shape, 1, cand, None, None, ctypes.byref(sk), None)
            assert st == 1, (c, cand)
            bm, bn = tile_of(shape, cand)
            assert int(sk.value) == bad * (c.Cin // 32) * -(-c.Cout // bn) * -(-c.B // bm), (c, cand)


# ---- the lists discriminate -------------------------------------------------------------------------------------
# flaw -> the property it breaks: a geometry can show the flaw only if it has the property
PROPERTY = {
    "no_far_clip": lambda g: "clip_hi" in GEO.classes_of(g),
    "next_image": lambda g: "next_image" in GEO.classes_of(g),
    "ceil_size": lambda g: "leftover" in GEO.classes_of(g),
    "dilate_rows_only": lambda g: g[6] > 1 and g[3] > 1,
}


# (flaw, route) whose domain does not contain the property, with the reason
NO_PROPERTY = {
    ("ceil_size", "bf16_strip"): "stride 1 leaves no row over",
    ("dilate_rows_only", "row_major"): "d = 1 (the dilated geometries are the route dil)",
    ("dilate_rows_only", "pixel_major"): "pixel-major requires d = 1",
    ("dilate_rows_only", "bf16_strip"): "the strip kernel requires d = 1",
    ("dilate_rows_only", "nchw"): "the gathering kernel has no dilated form",
}


@pytest.mark.parametrize("flaw", GEO.FLAWS)
def test_flawed_window_arithmetic_fails_the_equality_check(flaw):
    line = []
    for route in GEO.ROUTES:
        has = [g for g in GEO.geometries(route) if PROPERTY[flaw](g)]
        if not has:      # the route's domain does not contain the property
            assert (flaw, route) in NO_PROPERTY, (flaw, route)
            continue
        assert (flaw, route) not in NO_PROPERTY, (flaw, route)
        cin, cout, G = GEO.CHANNELS[route][-1]
        caught = 0
        for g in has:
            B, H, W, k, s, p, d = g
            c = GEO.Case(B, cin, cout, G, H, W, k, s, p, d)
            x, w, _, _, _ = GEO.operands(c, GEO.seed_of(c), False)
            want = GEO.reference(x, w, s, p, d, G)
            msg = GEO.first_difference(GEO.emulate(x, w, s, p, d, G, flaw), want, g, flaw)
            if msg is not None:
                caught += 1
                assert "got" in msg or "shape" in msg
        line.append(f"{route} {caught}/{len(has)}")
        assert caught >= 1, f"{flaw}: no listed geometry of {route} notices it"
    print(f"\ngeometry: {flaw} noticed on (geometries that notice / geometries with the property): " + ", ".join(line))


def test_failure_message_names_pixel_channel_values_and_classes():
    g = (2, 5, 4, 3, 2, 1, 1)
    want = np.arange(2 * 3 * 3 * 2).reshape(2, 3, 3, 2)
    assert GEO.first_difference(want.copy(), want, g) is None
    got = want.astype(np.float32)
    got[1, 2, 0, 1] = -7
    msg = GEO.first_difference(got, want, g, "route x")
    for part in ("route x", "(2, 5, 4, 3, 2, 1, 1)", "image 1", "(oh, ow) = (0, 1)", "channel 2", "got -7.0", "want 31.0",
                 "1 of 36", "clip_lo", "next_image"):
        assert part in msg, (part, msg)
    assert "shape" in GEO.first_difference(got[:, :, :2], want, g)
    got[0, 0, 0, 0] = np.nan
    assert "image 0" in GEO.first_difference(got, want, g)
