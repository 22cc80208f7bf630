"""tests/views.py: the written-everywhere check discriminates, and the value bounds alone do not.

Numpy emulations of a contraction's output, 150 rows x 72 channels behind a ReLU (about half of the expected
values are exactly 0): a correct result is copied over the 0xA5 image that `place_out` uploads, then what a
wrong schedule would skip -- one 64 x 64 tile of the ragged last row of tiles, one whole M panel, one single
element, the last row -- is restored to 0xA5.  `unwritten` reports exactly those elements, for 2-byte and
4-byte elements, and nothing for the complete result.

The same emulations on ReLU-zero positions PASS test_ops_gpu.assert_close and bf16_ref.assert_bf16_rounded:
the fill reads as -2.9e-16, within either bound of an expected 0.  That is why test_schedules_gpu.py asks for
the explicit check (fetch(..., written=True)) on every launch."""
import numpy as np
import pytest

import bf16_ref as BR
import views as V
from resnet_c_amd import ops
from test_ops_gpu import assert_close

ROWS, COUT, K = 150, 72, 576      # 64-row tiles: two whole M panels and a ragged third; a ragged second N tile
HOLES = {
    "tile": (slice(128, ROWS), slice(0, 64)),      # the 64-wide tile of the ragged last row of tiles
    "panel": (slice(64, 128), slice(0, COUT)),     # one whole M panel
    "element": (slice(77, 78), slice(41, 42)),
    "last row": (slice(ROWS - 1, ROWS), slice(0, COUT)),
}


def result():
    """an fp32 result behind a ReLU, as float64 reference and fp32 values"""
    ref = np.maximum(np.random.default_rng(7).standard_normal((ROWS, COUT)), 0.0)
    assert 0.4 < (ref == 0).mean() < 0.6
    return ref, ref.astype(np.float32)


def image_of(vals, es):
    """the bytes of the tensor part after a launch that wrote `vals` everywhere"""
    bits = ops.to_bf16_bits(vals) if es == 2 else np.ascontiguousarray(vals, dtype=np.float32)
    img = np.full(ROWS * COUT * es, V.OUT_BYTE, dtype=np.uint8)
    img[:] = bits.reshape(-1).view(np.uint8)
    return img


def poke(img, es, hole, only=None):
    """restore the elements of `hole` (of those, only where `only` is set) to the fill"""
    mask = np.zeros((ROWS, COUT), dtype=bool)
    mask[hole] = True
    if only is not None:
        mask &= only
    out = img.copy().reshape(ROWS * COUT, es)
    out[mask.reshape(-1)] = V.OUT_BYTE
    return out.reshape(-1), np.flatnonzero(mask.reshape(-1))


def values(img, es):
    flat = ops.from_bf16_bits(img.view(np.uint16)) if es == 2 else img.view(np.float32)
    return flat.reshape(ROWS, COUT)


@pytest.mark.parametrize("es", [2, 4])
def test_complete_result_with_relu_zeros_reports_nothing(es):
    _, vals = result()
    assert V.unwritten(image_of(vals, es), es).size == 0
    V.check_written(image_of(vals, es), es, "complete", COUT)
    V.assert_no_poison(vals, es == 2)
    # an untouched output is unwritten everywhere
    assert V.unwritten(np.full(ROWS * COUT * es, V.OUT_BYTE, np.uint8), es).size == ROWS * COUT


@pytest.mark.parametrize("es", [2, 4])
@pytest.mark.parametrize("hole", sorted(HOLES))
def test_unwritten_reports_exactly_the_skipped_elements(hole, es):
    _, vals = result()
    img, want = poke(image_of(vals, es), es, HOLES[hole])
    assert want.size == {"tile": 22 * 64, "panel": 64 * COUT, "element": 1, "last row": COUT}[hole]
    assert np.array_equal(V.unwritten(img, es), want)
    with pytest.raises(AssertionError) as e:
        V.check_written(img, es, f"emulated {hole}", COUT)
    msg = str(e.value)
    first, last = int(want[0]), int(want[-1])
    assert f"emulated {hole}: {want.size} elements never written" in msg
    assert f"the first at index {first}, the last at {last}" in msg
    assert f"(row, channel) {divmod(first, COUT)} .. {divmod(last, COUT)}" in msg
    # without the row length: indices only
    with pytest.raises(AssertionError) as e:
        V.check_written(img, es, "flat")
    assert "(row, channel)" not in str(e.value) and f"index {first}" in str(e.value)


def test_a_half_restored_element_counts_as_written():
    """all bytes of the element must hold the fill: a store that changed any of them is a store"""
    _, vals = result()
    img = image_of(vals, 4)
    img[4 * 100:4 * 100 + 3] = V.OUT_BYTE
    assert V.unwritten(img, 4).size == 0


@pytest.mark.parametrize("hole", ["element", "tile"])
def test_the_value_bounds_accept_an_unwritten_relu_zero(hole):
    """The blind spot: the skipped elements whose expected value is a ReLU zero.  Both value bounds of the suite
    accept the fill there; `unwritten` names every one of them."""
    ref, vals = result()
    where = HOLES[hole]
    if hole == "element":       # the nearest ReLU zero to the element of HOLES
        r, c = np.argwhere(ref == 0)[np.argmin(np.abs(np.argwhere(ref == 0) - (77, 41)).sum(axis=1))]
        where = (slice(r, r + 1), slice(c, c + 1))
    for es in (2, 4):
        img, want = poke(image_of(vals, es), es, where, only=ref == 0)
        assert want.size == (1 if hole == "element" else int((ref[where] == 0).sum())) and want.size >= 1
        got = values(img, es)
        assert (got.reshape(-1)[want] < 0).all() and (np.abs(got.reshape(-1)[want]) < 3e-16).all()    # the fill, -2.9e-16
        if es == 4:
            assert_close(got, ref, K + 4)                              # ... passes the fp32 bound
        else:
            BR.assert_bf16_rounded(got, ref, K, "unwritten ReLU zeros")    # ... and the per-element bf16 bound
        assert np.array_equal(V.unwritten(img, es), want)              # the explicit check does not
        with pytest.raises(AssertionError, match="never written"):
            V.check_written(img, es, "blind spot", COUT)
