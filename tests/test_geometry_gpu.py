"""Exact-integer geometry sweep over every k x k convolution route (tests/geometry.py holds the operands, the int64
reference, the lists and the edge classes; tests/test_geometry_host.py shows on the CPU what the lists reach).

Every launch goes through the typed runners on views (tests/views.py and the runners of test_schedules_gpu,
test_tap_skip_gpu, test_dilation_gpu): a fresh 0xA5 output between contraction-width guard bands, NaN guards around
every input, fetch(written=True).  The result must be np.array_equal to the int64 reference (bf16 results are
widened first, which is exact).  No tolerance: on these operands every partial sum of every summation order is an
integer below 2**24 (below 256 where bf16 is stored), see geometry.exact_bound.

A geometry counts for a route only if the evidence of the table shows that the route ran:

  route         forced by                                   evidence
  row_major     schedule(tile 1, 4, 0), tap_skip(1)         the tap-skip counters do not move (run_counted)
  dil           the same through the dilated entry point    the entry point (d >= 2 has no other fp32 MFMA kernel)
  pixel_major   tap_skip(2), tiles 1 and 4                  counters = (1, planned K tiles) (run_counted)
  bf16_tile     tiles 1 and 4, bf16 -> bf16 and -> fp32     the debug stamps say "tile"
  bf16_wide     candidates 9 and 14 on the list, all six    the debug stamps say "wide"
                on one geometry per edge class
  bf16_strip    the last candidate                          the debug stamps say "strip"
  grouped       every operand on a 16-byte boundary         the documented rule: shape (k = 3, Cin == Cout, % 32, Cg
                                                            divides or is a multiple of 32) + alignment
  direct        Cin = 5, and (24 -> 36, G = 12)             no whole channel segment / no super-group shape
  nchw          set_nchw_taps(2) against (0)                mode 2 issues fewer launches than mode 0

Beyond the table: the row-major route also runs its edge-class representatives at Cin 128 (the chunked K sum), as the
pixel-major route does, and the four-wave routes run their representatives on the other candidates as well (2, 3 and
the resident grids 5-8).  The grouped route goes through test_dilation_gpu.run_nhwc_dt / run_forward (with d = 1 they
issue the undilated launch) because test_grouped_gpu.run_grouped* neither widen the guard bands nor check "written
everywhere"; run_grouped_nhwc is used on top, on the d = 1 geometries.

Canary.  That integer sums leave the fp32 and bf16 MFMA paths bit-exact is an assumption.  Each of the seven MFMA
routes first runs one canary whose compared windows lie wholly inside the image (pad 0, stride 1; the pixel-major
and strip routes need pad 1 and compare the interior pixels only; the DIL route exists only at d >= 2 and runs
d = 2).  If a canary is not bit-exact the cause is not geometry: that route alone is then held to the project's
bounds against the same reference (test_ops_gpu.assert_close with K terms, bf16_ref.assert_bf16_rounded).  The
outcomes on the MI355X are in profiles/geometry/README.md.

Epilogue.  The representative of every edge class runs both with scale, shift, residual and ReLU and raw; the other
geometries alternate.  A failure names route, geometry, first differing output pixel and channel, got and want,
and the geometry's edge classes (geometry.first_difference); a test reports every failing geometry, not the first."""
import functools

import numpy as np
import pytest

import bf16_ref as BR
import geometry as GEO
import test_dilation_gpu as DG
import test_grouped_gpu as GG
import test_tap_skip_gpu as TS
import views as V
from resnet_c_amd import _lib as L
from test_ops_gpu import assert_close
from test_schedules_gpu import launches_of, schedule

pytestmark = pytest.mark.gpu

F32, BF16 = L.RN_DTYPE_F32, L.RN_DTYPE_BF16
TYPES = {"bf16": (BF16, BF16), "bf16_f32": (BF16, F32)}
NCAND = 15      # 8 four-wave candidates, 6 wide tiles, the strip kernel


def shape8(c):
    return (c.B, c.Cin, c.Cout, c.H, c.W, c.k, c.s, c.p)


def fast_group_shape(c):
    """the documented rule of the super-group kernel (include/rn_hip.h)"""
    cg = c.Cin // c.G
    return c.G >= 2 and c.k == 3 and c.Cin == c.Cout and c.Cin % 32 == 0 and (32 % cg == 0 or cg % 32 == 0)


# ---- one launch per (route, variant) ----------------------------------------------------------------------------
def launch(route, variant, c, x, w, sc, sh, res, relu):
    """the result (NCHW fp32 host array) of ONE launch of `route`; raises where the evidence says another kernel ran"""
    if route == "row_major":
        return TS.run_counted(shape8(c), variant, 1, x, w, c.s, c.p, sc, sh, res, relu)
    if route == "pixel_major":
        return TS.run_counted(shape8(c), variant, 2, x, w, c.s, c.p, sc, sh, res, relu)
    if route == "dil":
        assert c.d >= 2
        with schedule(tile=variant), TS.tap_skip(1):
            return DG.run_nhwc_dt(x, w, c.s, c.p, c.d, 1, sc, sh, res, relu, F32, F32)
    if route in ("bf16_tile", "bf16_wide", "bf16_strip"):
        if route == "bf16_tile":
            (dt_in, dt_out), cand, want = TYPES[variant[0]], variant[1], "tile"
        else:
            (dt_in, dt_out), cand, want = (BF16, BF16), variant, route[5:]
        run = lambda: DG.run_nhwc_dt(x, w, c.s, c.p, c.d, 1, sc, sh, res, relu, dt_in, dt_out)
        if route == "bf16_strip":
            run = lambda: V.run_conv_dt(x, w, c.s, c.p, sc, sh, res, relu, BF16, BF16)
        got, kernel, grid = DG.kernel_of_launch(run, cand)
        assert kernel == want and grid > 0, f"{route} {variant} {c}: the {kernel} kernel ran, grid {grid}"
        return got
    if route == "grouped":
        assert fast_group_shape(c), c
        if variant == "packed":
            return DG.run_nhwc_dt(x, w, c.s, c.p, c.d, c.G, sc, sh, res, relu, F32, F32)
        if variant == "undilated":
            assert c.d == 1
            return GG.run_grouped_nhwc(x, w, c.s, c.p, c.G, sc, sh, res, relu, {})
        assert sc is None and sh is None and res is None and not relu
        return DG.run_forward(x, w, c.s, c.p, c.d, c.G, variant)
    if route == "direct":
        assert not fast_group_shape(c) and c.Cin % 32 != 0 and c.Cin > 4
        assert sc is None and sh is None and res is None and not relu
        return DG.run_forward(x, w, c.s, c.p, c.d, c.G, variant)
    if route == "nchw":
        assert c.d == 1 and c.G == 1 and sc is None and not relu
        guard = V.contraction_guard(c.Cout * 4)
        got0, n0 = launches_of(lambda: V.run_conv2d(x, w, c.s, c.p, "nchw", 0, {}, guard_bytes=guard))
        got2, n2 = launches_of(lambda: V.run_conv2d(x, w, c.s, c.p, "nchw", 2, {}, guard_bytes=guard))
        assert 0 < n2 < n0, f"nchw {c}: {n2} launches gathering, {n0} transposing: the gathering kernel did not run"
        assert np.array_equal(got0, got2), f"nchw {c}: the two routes differ"
        return got2
    raise KeyError(route)


FIRST_VARIANT = {"row_major": 1, "dil": 1, "pixel_major": 1, "bf16_tile": ("bf16", 1), "bf16_wide": 9, "bf16_strip": NCAND,
                 "grouped": "packed"}
LAUNCHES_PER_CALL = {"nchw": 2}
HAS_EPILOGUE = {"row_major", "dil", "pixel_major", "bf16_tile", "bf16_wide", "bf16_strip"}

# (case, interior): the compared windows lie wholly inside the image
CANARIES = {
    "row_major": (GEO.Case(2, 32, 40, 1, 6, 7, 3, 1, 0, 1), False),
    "dil": (GEO.Case(2, 32, 40, 1, 7, 8, 3, 1, 0, 2), False),
    "pixel_major": (GEO.Case(2, 32, 40, 1, 6, 7, 3, 1, 1, 1), True),
    "bf16_tile": (GEO.Case(2, 64, 40, 1, 6, 7, 3, 1, 0, 1), False),
    "bf16_wide": (GEO.Case(2, 64, 40, 1, 6, 7, 3, 1, 0, 1), False),
    "bf16_strip": (GEO.Case(3, 64, 64, 1, 5, 8, 3, 1, 1, 1), True),
    "grouped": (GEO.Case(2, 128, 128, 32, 6, 7, 3, 1, 0, 1), False),
}


def prepared(c, epilogue, bf16_out, bf16_in=None):
    """operands and the int64 reference of one case; the exactness condition in its closed form, 6 k^2 * 2 + 12 (the
    host test evaluates geometry.exact_bound itself on every case of every list); below 256 wherever bf16 is read
    or stored"""
    x, w, sc, sh, res = GEO.operands(c, GEO.seed_of(c), epilogue)
    assert 6 * c.k * c.k * 2 + 12 < (256 if bf16_out or bf16_in else 2 ** 24), c
    ref = GEO.reference(x, w, c.s, c.p, c.d, c.G, sc, sh, res, epilogue)
    V.assert_no_poison(ref, bf16_out, str(c))
    return x, w, sc, sh, res, ref


@functools.lru_cache(maxsize=None)
def canary(route):
    """(bit-exact, largest |got - want|) of the route's canary; the fp32 / direct routes outside the table count as exact"""
    if route not in CANARIES:
        return True, 0.0
    c, interior = CANARIES[route]
    assert c.s == 1 and c.p == (1 if interior else 0)
    bf16_out = route.startswith("bf16")
    x, w, sc, sh, res, ref = prepared(c, False, bf16_out, bf16_out)
    got = launch(route, FIRST_VARIANT[route], c, x, w, None, None, None, False)
    assert got.shape == ref.shape
    if interior:
        got, ref = got[:, :, 1:-1, 1:-1], ref[:, :, 1:-1, 1:-1]
        assert ref.size > 0
    diff = float(np.abs(got.astype(np.float64) - ref).max())
    exact = bool(np.array_equal(got, ref))
    print(f"\ngeometry: canary {route} {tuple(c)}{' (interior pixels)' if interior else ''}: "
          f"{'bit-exact' if exact else 'NOT bit-exact'}, largest |got - want| = {diff:g}")
    return exact, diff


class Sweep:
    """the launches of one test: compares, counts, collects every failing geometry"""

    totals = {}     # route -> [launches, set of geometries that counted]

    def __init__(self, route, name):
        self.route, self.name, self.launches, self.counted, self.failures = route, name, 0, set(), []
        self.exact = canary(route)[0]

    def run(self, variant, c, epilogue):
        bf16_out = self.route.startswith("bf16") and not (self.route == "bf16_tile" and variant[0] == "bf16_f32")
        x, w, sc, sh, res, ref = prepared(c, epilogue, bf16_out, self.route.startswith("bf16"))
        what = f"{self.route} {variant} Cin {c.Cin} Cout {c.Cout} G {c.G} {'epilogue' if epilogue else 'raw'}"
        got = launch(self.route, variant, c, x, w, sc, sh, res, epilogue)
        self.launches += LAUNCHES_PER_CALL.get(self.route, 1)
        if self.exact:
            msg = GEO.first_difference(got, ref, GEO.geom_of(c), what)
            if msg is not None:
                self.failures.append(msg)
                return
        elif bf16_out:
            BR.assert_bf16_rounded(got, ref.astype(np.float64), c.Cin // c.G * c.k * c.k, what)
        else:
            assert_close(got, ref.astype(np.float64), c.Cin // c.G * c.k * c.k + (4 if epilogue else 0))
        self.counted.add(GEO.geom_of(c))

    def sweep(self, variant, cases, both=()):
        """every case once, with the epilogue on every other one; the cases whose geometry is in `both` raw AND with it"""
        for i, c in enumerate(cases):
            if self.route not in HAS_EPILOGUE and not (self.route == "grouped" and variant in ("packed", "undilated")):
                self.run(variant, c, False)
            elif GEO.geom_of(c) in both:
                self.run(variant, c, True)
                self.run(variant, c, False)
            else:
                self.run(variant, c, i % 2 == 0)

    def done(self, listed):
        t = Sweep.totals.setdefault(self.route, [0, set()])
        t[0] += self.launches
        t[1] |= self.counted
        print(f"\ngeometry: {self.name}: {self.launches} launches, {len(self.counted)} of {listed} geometries counted"
              f"{'' if self.exact else ' (canary not exact: held to the value bounds)'}")
        assert not self.failures, f"{len(self.failures)} launches differ from the int64 reference:\n" + "\n".join(self.failures[:12])
        assert len(self.counted) == listed, f"{self.name}: {listed - len(self.counted)} listed geometries did not count"


def reps(route):
    return set(GEO.representatives(route).values())


def listed(route, **where):
    return [c for c in GEO.cases(route) if all(getattr(c, k) == v for k, v in where.items())]


# ---- the canaries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", GEO.MFMA_ROUTES)
def test_canary(route):
    exact, diff = canary(route)
    assert exact == (diff == 0.0)
    if not exact:      # not a geometry failure: the sweep of this route falls back to the value bounds (module docstring)
        c, _ = CANARIES[route]
        assert diff <= 6 * c.k * c.k, f"canary {route}: off by {diff}, more than any rounding of these sums explains"


# ---- 1. fp32 four-wave, row-major ---------------------------------------------------------------------------------
# (and the edge-class representatives at Cin 128: the chunked K sum of the row-major kernel)
@pytest.mark.parametrize("tile", [1, 4, 0])
def test_row_major(tile):
    sw = Sweep("row_major", f"test_row_major[{tile}]")
    sw.sweep(tile, GEO.cases("row_major"), reps("row_major") | {GEO.geom_of(c) for c in listed("row_major", Cin=128)})
    sw.done(len(GEO.geometries("row_major")))


# ---- beyond the table: the other four-wave candidates on the edge-class representatives ------------------------------
# 2 and 3 are the 128x64 and 64x128 tiles, 5-8 the four tiles walked by a resident grid; the evidence of each route
# as above
OTHER = [2, 3, 5, 6, 7, 8]


@pytest.mark.parametrize("route", ["row_major", "dil", "pixel_major", "bf16_tile"])
def test_other_candidates_on_the_representatives(route):
    cases = [c for c in GEO.cases(route) if GEO.geom_of(c) in reps(route) or c.Cin == 128]
    sw = Sweep(route, f"test_other_candidates_on_the_representatives[{route}]")
    for cand in OTHER:
        sw.sweep(("bf16", cand) if route == "bf16_tile" else cand, cases, {GEO.geom_of(c) for c in cases})
    sw.done(len({GEO.geom_of(c) for c in cases}))


# ---- 2. fp32 four-wave, the DIL instantiation -----------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 4, 0])
def test_dil(tile):
    sw = Sweep("dil", f"test_dil[{tile}]")
    sw.sweep(tile, GEO.cases("dil"), reps("dil"))
    sw.done(len(GEO.geometries("dil")))


# ---- 3. fp32 pixel-major ------------------------------------------------------------------------------------------
# the list at its own B, a third of it again at B = 66 (two image blocks at BM 64, one ragged block at BM 128) and
# the edge-class representatives at Cin 128 (the chunked K sum for k = 3 and 5)
@pytest.mark.parametrize("part", ["listed", "b66", "cin128"])
@pytest.mark.parametrize("tile", [1, 4])
def test_pixel_major(tile, part):
    cases = [c for c in GEO.cases("pixel_major")
             if (part == "cin128") == (c.Cin == 128) and (part == "b66") == (c.B == 66 and c.Cin == 32)]
    sw = Sweep("pixel_major", f"test_pixel_major[{tile}-{part}]")
    sw.sweep(tile, cases, {GEO.geom_of(c) for c in cases} if part == "cin128" else reps("pixel_major"))
    sw.done(len({GEO.geom_of(c) for c in cases}))


# ---- 4. bf16 four-wave ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 4])
@pytest.mark.parametrize("types", sorted(TYPES))
def test_bf16_tile(types, tile):
    sw = Sweep("bf16_tile", f"test_bf16_tile[{types}-{tile}]")
    sw.sweep((types, tile), GEO.cases("bf16_tile"), reps("bf16_tile"))
    sw.done(len(GEO.geometries("bf16_tile")))


# ---- 5. bf16 wide tiles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cand", range(9, NCAND))
def test_bf16_wide(cand):
    assert L.lib().rn_conv_tile_candidates() == NCAND
    whole = cand in (9, 14)
    cases = [c for c in GEO.cases("bf16_wide") if whole or GEO.geom_of(c) in reps("bf16_wide")]
    sw = Sweep("bf16_wide", f"test_bf16_wide[{cand}]")
    sw.sweep(cand, cases, reps("bf16_wide"))
    sw.done(len(cases))


# ---- 6. bf16 strip --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 128])
def test_bf16_strip(C):
    assert L.lib().rn_conv_tile_candidates() == NCAND
    cases = listed("bf16_strip", Cin=C)
    sw = Sweep("bf16_strip", f"test_bf16_strip[{C}]")
    sw.sweep(NCAND, cases, {GEO.geom_of(c) for c in cases})      # every plane with the residual and without
    sw.done(len(cases))


# ---- 7. grouped fast path -------------------------------------------------------------------------------------------
# the packed NHWC entry point on the whole list (epilogue as above) through test_dilation_gpu.run_nhwc_dt, which for
# d = 1 issues the launch of rn_conv2d_grouped_nhwc_forward_dt and, unlike test_grouped_gpu.run_grouped*, puts the
# output between contraction-width bands and checks it written everywhere; the drop-in entry point (OIHW weight packed
# per call) on every fourth geometry and the representatives, writing NCHW (out_nchw) and, for the representatives,
# NHWC; and the undilated entry point itself (test_grouped_gpu.run_grouped_nhwc: 256-byte bands, no written check) on
# the d = 1 geometries
@pytest.mark.parametrize("cg", GEO.CHANNELS["grouped"], ids=lambda t: f"C{t[0]}-G{t[2]}")
def test_grouped(cg):
    cases = listed("grouped", Cin=cg[0], G=cg[2])
    sw = Sweep("grouped", f"test_grouped[C{cg[0]}-G{cg[2]}]")
    sw.sweep("packed", cases, reps("grouped"))
    dropin = [c for i, c in enumerate(cases) if i % 4 == 0 or GEO.geom_of(c) in reps("grouped")]
    sw.sweep("nchw", dropin)
    sw.sweep("nhwc", [c for c in cases if GEO.geom_of(c) in reps("grouped")])
    sw.sweep("undilated", [c for c in cases if c.d == 1])
    sw.done(len(cases))


# ---- 8. the direct kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("ch", GEO.CHANNELS["direct"], ids=lambda t: f"{t[0]}to{t[1]}-G{t[2]}")
def test_direct(ch, layout):
    cases = listed("direct", Cin=ch[0], G=ch[2])
    sw = Sweep("direct", f"test_direct[{ch[0]}to{ch[1]}-G{ch[2]}-{layout}]")
    sw.sweep(layout, cases)
    sw.done(len(cases))


# ---- 9. the NCHW gathering kernel -----------------------------------------------------------------------------------
def test_nchw_gather():
    sw = Sweep("nchw", "test_nchw_gather")
    sw.sweep(None, GEO.cases("nchw"))
    sw.done(len(GEO.geometries("nchw")))


def test_totals():
    """the record of the run (after the sweeps above): launches and counted geometries per route"""
    for route in GEO.ROUTES:
        n, counted = Sweep.totals.get(route, [0, set()])
        print(f"\ngeometry: total {route}: {n} launches, {len(counted)} of {len({GEO.geom_of(c) for c in GEO.cases(route)})} geometries counted, "
              f"canary {'exact' if canary(route)[0] else 'NOT exact'}")
