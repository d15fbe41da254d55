"""The poisoned-view helper (tests/kernel_views.py) checked without a device: the host image is numpy alone, a
corruption planted anywhere in the frame is caught and located, the interior round-trips exactly.  This is the proof
that the frame checks of tests/test_gpu_views.py, tests/test_gpu_rnn_views.py and tests/test_gpu_rbm_views.py can
fail.  The 8-byte views (float64 / uint64 interiors over the same uint32 words) have their own cases at the end."""
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
    elif layout == "shifted":
        assert c0 == 1 and S == roundup4(cols) + 8 and S % 4 == 0 and origin % 4 == 1
    else:
        assert layout == "odd" and c0 == 1 and S == cols + 3
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


@pytest.mark.parametrize("cols", [1, 3, 4, 5, 10, 39, 64, 136, 429, 8532])
@pytest.mark.parametrize("rows", [0, 1, 33])
def test_shifted_is_the_least_the_layer_kernels_allow(rows, cols):
    """the base 4 bytes past a 16-byte boundary (the backing buffer is an allocation: 16-byte aligned and more), the
    stride a multiple of 4 elements -- so every row origin is off 16 bytes by the same 4 -- and the view's pointer
    is where element (0, 0) lies"""
    c0, S = layout_geometry(cols, "shifted")
    assert (GUARD * S + c0) * 4 % 16 == 4 and S % 4 == 0 and S >= cols + 8
    v = PoisonView(np.arange(rows * cols, dtype=np.float32).reshape(rows, cols), "shifted", rows=rows, cols=cols,
                   device=False) if rows else PoisonView.empty(0, cols, "shifted", device=False)
    assert (v.c0, v.stride) == (c0, S)
    for r in range(rows):
        assert word(v, r, 0) * 4 % 16 == 4
    if rows:
        assert v.raw()[word(v, 0, 0)] == np.float32(0).view(np.uint32)
        assert v.raw()[word(v, rows - 1, cols - 1)] == np.float32(rows * cols - 1).view(np.uint32)
        assert v.raw()[word(v, 0, -1)] == POISON and v.raw()[word(v, rows - 1, cols)] == POISON
    # a vector (bias, packed parameters, mask words as one row) is 4-byte aligned in the same way
    vec = PoisonView.vector(np.zeros(cols, np.float32), "shifted", device=False)
    assert word(vec, 0, 0) * 4 % 16 == 4 and vec.rows == 1


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


# ---- 8-byte views (float64 / uint64): two words per element, the same checks on words ------------------------------
WIDE_LAYOUTS = ("tight", "offset")


@pytest.mark.parametrize("dtype", [np.float64, np.uint64])
@pytest.mark.parametrize("layout", WIDE_LAYOUTS)
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 3), (1, 130), (3, 5)])
def test_wide_view_geometry_and_round_trip(rows, cols, layout, dtype):
    a = (np.arange(rows * cols, dtype=np.uint64) * np.uint64(0x0123456789ABCDEF)).view(dtype).reshape(rows, cols)
    v = PoisonView(a, layout, dtype=dtype, device=False)
    c0, S = layout_geometry(2 * cols, layout)
    assert (v.wpe, v.wcols, v.c0, v.wstride, v.stride) == (2, 2 * cols, c0, S, S // 2)
    assert c0 % 2 == 0 and S % 2 == 0 and (GUARD * S + c0) % 2 == 0  # the base is 8-byte aligned
    assert v.words == (2 * GUARD + rows) * (c0 + S)
    got = v.numpy()
    assert got.dtype == np.dtype(dtype) and got.shape == (rows, cols)
    np.testing.assert_array_equal(got.view(np.uint64), a.view(np.uint64))
    raw = v.raw()
    assert raw.dtype == np.uint32 and (raw == POISON).sum() == v.words - 2 * rows * cols
    assert_frame_untouched(v)
    assert_unchanged(v, raw)
    e = PoisonView.empty(rows, cols, layout, dtype, device=False)
    assert (e.raw() == POISON).all()
    ev = PoisonView.empty_vector(cols, layout, dtype, device=False)
    assert ev.rows == 1 and ev.wcols == 2 * cols and (ev.raw() == POISON).all()
    vv = PoisonView.vector(a[0], layout, device=False, dtype=dtype)
    np.testing.assert_array_equal(vv.numpy()[0].view(np.uint64), a[0].view(np.uint64))


def wword(view, r, wc):
    """backing word of word column wc of row r of an 8-byte view (anywhere in the frame)"""
    return (GUARD + r) * view.wstride + view.c0 + wc


WIDE_PLANTS = [
    ("column padding", lambda v: (v.rows // 2, v.wcols)),      # the first padding word after a row's last element
    ("column padding", lambda v: (v.rows - 1, v.wcols + 1)),   # the high word of the element one past the end
    ("guard rows above", lambda v: (-1, 0)),
    ("guard rows above", lambda v: (-GUARD, v.wcols - 1)),
    ("guard rows below", lambda v: (v.rows, 0)),
    ("guard rows below", lambda v: (v.rows + GUARD - 1, 1)),
    ("c0 band", lambda v: (0, -1)),                            # the high word of the element before (0, 0)
    ("c0 band", lambda v: (v.rows - 1, -v.c0)),
]
WIDE_PLANT_CASES = [(layout, k) for layout in WIDE_LAYOUTS for k, (place, _) in enumerate(WIDE_PLANTS)
                    if not (place == "c0 band" and layout == "tight")]


@pytest.mark.parametrize("rows,cols", [(1, 3), (3, 5)])   # 6 and 10 word columns: padding in both layouts
@pytest.mark.parametrize("layout,k", WIDE_PLANT_CASES)
def test_wide_view_planted_word_is_caught_and_located(rows, cols, layout, k):
    place, where = WIDE_PLANTS[k]
    v = PoisonView(np.ones((rows, cols)), layout, dtype=np.float64, device=False)
    assert v.wstride - v.c0 > v.wcols + 1
    r, wc = where(v)
    before = v.raw()
    v._host[wword(v, r, wc)] = np.uint32(0)
    with pytest.raises(AssertionError) as ei:
        assert_frame_untouched(v, "planted")
    msg = str(ei.value)
    assert place in msg and f"(row {r}, col {wc})" in msg, msg
    with pytest.raises(AssertionError):
        assert_unchanged(v, before, "planted")
    # one word of an interior element is not the frame
    v2 = PoisonView(np.ones((rows, cols)), layout, dtype=np.float64, device=False)
    v2._host[wword(v2, rows - 1, v2.wcols - 1)] = np.uint32(7)
    assert_frame_untouched(v2)


@pytest.mark.parametrize("layout", WIDE_LAYOUTS)
@pytest.mark.parametrize("half", [0, 1])
def test_wide_pure_input_changed_interior_is_caught(layout, half):
    """either word of an element of a pure 8-byte input (softmax pairs, argmax keys)"""
    keys = np.arange(1, 8, dtype=np.uint64) << np.uint64(33)
    v = PoisonView.vector(keys, layout, device=False, poison=POISON_INPUT, dtype=np.uint64)
    assert not (v.raw() == POISON).any()
    assert_unchanged(v, v.initial)
    v._host[wword(v, 0, 2 * 3 + half)] ^= np.uint32(1)
    assert_frame_untouched(v)  # the frame is intact: only assert_unchanged sees it
    with pytest.raises(AssertionError, match="interior.*row 0, col %d" % (6 + half)):
        assert_unchanged(v, v.initial, "keys")


@pytest.mark.parametrize("dtype", [np.float64, np.uint64])
def test_wide_view_refuses_the_odd_layout(dtype):
    """a misaligned address must never reach a 64-bit atomic: the request fails in Python"""
    for make in (lambda: PoisonView(np.zeros((1, 4)), "odd", dtype=dtype, device=False),
                 lambda: PoisonView.empty(2, 3, "odd", dtype, device=False),
                 lambda: PoisonView.empty_vector(5, "odd", dtype, device=False),
                 lambda: PoisonView.vector(np.zeros(5), "odd", device=False, dtype=dtype)):
        with pytest.raises(ValueError, match="8-byte"):
            make()
    PoisonView(np.zeros((1, 4), np.float32), "odd", device=False)  # 4-byte views keep it
    # `shifted` has an odd c0 too: its base is 4 bytes past a 16-byte boundary, never 8-byte aligned
    for make in (lambda: PoisonView(np.zeros((1, 4)), "shifted", dtype=dtype, device=False),
                 lambda: PoisonView.empty(2, 3, "shifted", dtype, device=False),
                 lambda: PoisonView.empty_vector(5, "shifted", dtype, device=False),
                 lambda: PoisonView.vector(np.zeros(5), "shifted", device=False, dtype=dtype)):
        with pytest.raises(ValueError, match="8-byte"):
            make()
    PoisonView(np.zeros((1, 4), np.float32), "shifted", device=False)
