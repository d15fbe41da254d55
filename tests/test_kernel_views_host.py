"""The poisoned-view helper (tests/kernel_views.py) checked without a device: the host image is numpy alone, a
corruption planted anywhere in the frame is caught and located, the interior round-trips exactly.  This is the proof
that the frame checks of tests/test_gpu_views.py can fail."""
import numpy as np
import pytest

from kernel_views import (GUARD, LAYOUTS, POISON, POISON_INPUT, PoisonView, assert_frame_untouched, assert_unchanged,
                          frame_violation, layout_geometry, locate, roundup4)

SHAPES = [(1, 1), (5, 7), (37, 131), (36, 132)]


def word(view, r, c):
    """backing word of element (r, c) in the view's coordinates (anywhere in the frame)"""
    return (GUARD + r) * view.stride + view.c0 + c


def test_poison_is_a_quiet_nan_pattern():
    for p in (POISON, POISON_INPUT):
        f = np.array([p], np.uint32).view(np.float32)[0]
        assert np.isnan(f) and (int(p) >> 22) & 1 == 1  # exponent all ones, quiet bit set
    assert POISON != POISON_INPUT


@pytest.mark.parametrize("layout", LAYOUTS)
def test_input_poison_copied_into_an_output_frame_is_caught(layout):
    """what a copying kernel that runs past a row's end does: the source's padding lands in the destination's"""
    a = np.ones((5, 7), np.float32)
    src = PoisonView(a, layout, device=False, poison=POISON_INPUT)
    assert (src.raw() == POISON_INPUT).sum() == src.words - 35 and not (src.raw() == POISON).any()
    assert_frame_untouched(src)
    dst = PoisonView.empty(5, 7, layout, device=False)
    dst._host[word(dst, 2, 7)] = src.raw()[word(src, 2, 7)]
    with pytest.raises(AssertionError, match="column padding"):
        assert_frame_untouched(dst)
    # the hole this closes: with one pattern for both, the same copy is invisible
    same = PoisonView(a, layout, device=False)
    dst2 = PoisonView.empty(5, 7, layout, device=False)
    dst2._host[word(dst2, 2, 7)] = same.raw()[word(same, 2, 7)]
    assert_frame_untouched(dst2)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_geometry(rows, cols, layout):
    c0, S = layout_geometry(cols, layout)
    v = PoisonView.empty(rows, cols, layout, device=False)
    assert (v.c0, v.stride) == (c0, S) and S >= cols
    assert v.words == (2 * GUARD + rows) * (c0 + S)
    origin = GUARD * S + c0
    if layout == "tight":
        assert c0 == 0 and S == roundup4(cols) and origin % 4 == 0
    elif layout == "offset":
        assert c0 == 4 and S == roundup4(cols) + 12 and origin % 4 == 0
    else:
        assert c0 == 1 and S == cols + 3
    # the last interior element lies inside the buffer with GUARD whole rows after it
    assert word(v, rows - 1, cols - 1) + GUARD * S < v.words


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_interior_round_trips_and_frame_is_poison(rows, cols, layout):
    a = np.random.default_rng(rows * 1000 + cols).standard_normal((rows, cols)).astype(np.float32)
    a[0, 0] = -0.0
    a[-1, -1] = np.float32(1e-45)  # a denormal: bits, not values
    v = PoisonView(a, layout, device=False)
    np.testing.assert_array_equal(v.numpy().view(np.uint32), a.view(np.uint32))
    raw = v.raw()
    assert raw.dtype == np.uint32 and raw.size == v.words
    assert (raw == POISON).sum() == v.words - rows * cols
    assert_frame_untouched(v)
    assert_unchanged(v, raw)
    # integers keep their bits too (class ids, row indices)
    ids = np.arange(-2, cols - 2, dtype=np.int32)
    vi = PoisonView.vector(ids, layout, device=False)
    assert vi.dtype == np.int32 and vi.rows == 1
    np.testing.assert_array_equal(vi.numpy()[0], ids)
    # an empty view: the interior is poison as well
    e = PoisonView.empty(rows, cols, layout, device=False)
    assert (e.raw() == POISON).all() and np.isnan(e.numpy()).all()


def plant(view, r, c, value=np.uint32(0)):
    view._host[word(view, r, c)] = value


PLANTS = [
    ("column padding", lambda v: (v.rows // 2, v.cols)),          # the first padding word of a middle row
    ("column padding", lambda v: (v.rows - 1, v.cols)),           # ... of the last row
    ("guard rows above", lambda v: (-1, 0)),                      # the row just above the view
    ("guard rows above", lambda v: (-GUARD, v.cols - 1)),         # the first guard row
    ("guard rows below", lambda v: (v.rows, 0)),                  # the row just below
    ("guard rows below", lambda v: (v.rows + GUARD - 1, 1)),      # the last guard row
    ("c0 band", lambda v: (0, -1)),                               # the word before element (0, 0)
    ("c0 band", lambda v: (v.rows - 1, -v.c0)),                   # the band's first word, last row
]
# (the tight layout has no c0 band; every layout has column padding at these widths)
PLANT_CASES = [(layout, k) for layout in LAYOUTS for k, (place, _) in enumerate(PLANTS)
               if not (place == "c0 band" and layout == "tight")]


@pytest.mark.parametrize("rows,cols", [(5, 7), (37, 131)])
@pytest.mark.parametrize("layout,k", PLANT_CASES)
def test_planted_corruption_is_caught_and_located(rows, cols, layout, k):
    place, where = PLANTS[k]
    a = np.ones((rows, cols), np.float32)
    v = PoisonView(a, layout, device=False)
    r, c = where(v)
    assert (place != "c0 band" or v.c0 > 0) and (place != "column padding" or v.stride - v.c0 > cols)
    before = v.raw()
    plant(v, r, c)
    with pytest.raises(AssertionError) as ei:
        assert_frame_untouched(v, "planted")
    msg = str(ei.value)
    assert place in msg and f"(row {r}, col {c})" in msg, msg
    with pytest.raises(AssertionError):
        assert_unchanged(v, before, "planted")
    # the interior itself is not the frame: writing it is what an output does
    v2 = PoisonView(a, layout, device=False)
    plant(v2, rows - 1, cols - 1, np.uint32(7))
    assert_frame_untouched(v2)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_another_nan_in_the_frame_is_a_failure(layout):
    """compared as uint32: a NaN with another payload (what 0 * POISON or POISON + 1 gives) is a written word"""
    v = PoisonView(np.zeros((4, 6), np.float32), layout, device=False)
    other = np.array([np.nan], np.float32).view(np.uint32)[0]
    assert other != POISON
    plant(v, 4, 2, other)
    assert "guard rows below" in frame_violation(v.raw(), 4, 6, layout)
    # and the very first / very last word of the buffer count
    for idx in (0, v.words - 1):
        w = PoisonView(np.zeros((4, 6), np.float32), layout, device=False)
        w._host[idx] = np.uint32(1)
        assert frame_violation(w.raw(), 4, 6, layout) is not None
        assert locate(idx, 4, 6, layout)[0] in ("guard rows above", "guard rows below")
