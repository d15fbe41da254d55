"""Poisoned caller-owned views for the kernel tests (tests/test_gpu_views.py, tests/test_gpu_rnn_views.py,
tests/test_gpu_rbm_views.py, tests/test_gpu_layer_views.py, tests/test_kernel_views_host.py).

DeviceArray hands every kernel a matrix at an allocation base, with a stride that is a multiple of 64 floats and
zero-filled padding.  A PoisonView is what the C ABI actually allows: a [rows x cols] window somewhere inside a
larger buffer, with a tight or odd stride, a base that is no more aligned than the header promises, and every word
around it -- guard rows above and below, the band before a row's first column, the column padding -- holding one
fixed quiet-NaN bit pattern (POISON).

  PoisonView(a, layout)              a in the interior, poison everywhere else
  PoisonView.empty(r, c, layout)     the interior is poison too: an output must write every element
  PoisonView.vector(v, layout)       a 1 x n view (bias, momentum, scale[], slab-sum rows, class ids, row indices):
                                     a poisoned band before and after, 16-B aligned in `tight` / `offset`,
                                     4-B aligned (4 bytes past a 16-B boundary) in `shifted` / `odd`
  assert_frame_untouched(view)       every word of the backing buffer outside [rows x cols] is still POISON
                                     (compared as uint32: another NaN is a failure too); names the first offender
  assert_unchanged(view, before)     the whole backing buffer is bit-identical to `before` (view.raw() taken
                                     before the call, or view.initial, the image that was uploaded): a pure input

Layouts (S = row stride in elements, c0 = elements between the 16-B aligned row origin and the view's column 0;
GUARD = 3 rows of S elements above and below):
  tight    c0 = 0, S = roundup4(cols)       no padding at all where cols % 4 == 0
  offset   c0 = 4, S = roundup4(cols) + 12  rows neither 64-float nor 256-B aligned; the base 16-B aligned, no more
  shifted  c0 = 1, S = roundup4(cols) + 8   the base 4 bytes past a 16-B boundary, the stride a multiple of 4: the
                                            least the shared / discrete / sparse layer kernels' headers allow
                                            (every row origin is off 16 bytes: their masked scalar loads)
  odd      c0 = 1, S = cols + 3             a 4-B aligned base and a stride that is no multiple of 4: only for entry
                                            points whose header allows any stride (the GEMM family rejects it)
The backing buffer has (GUARD + rows + GUARD) * (c0 + S) words; element (r, c) of the view is word
(GUARD + r) * S + c0 + c, so .ptr = base + (GUARD * S + c0) * 4.

8-byte operands (float64 / uint64: softmax pairs, statistics accumulators, argmax keys).  The backing buffer stays
uint32 words and the frame holds the same POISON word, so every check still compares words; an element is two words,
the geometry is that of a 4-byte view of 2 * cols word columns (.wcols, .wstride; .stride stays in elements), and the
places a check names are in word columns.  Only `tight` and `offset` exist: c0 and S are even there, so the base is
8-byte aligned, as the 64-bit atomics and loads on these operands need; asking for `shifted` or `odd` (c0 odd)
raises ValueError.

What the poison can and cannot show.  A read outside the matrix is visible only when it reaches a stored output:
NaN times zero is NaN, so a kernel that multiplies a stray operand by a zero weight does not hide it, and a stray
row that enters a fused sum poisons the sum.  A read whose value is discarded is NOT detectable this way -- and the
GEMM's edge clamps make such reads on purpose (they re-read the matrix's last row / column, never the frame, and
drop the product).  A write outside the matrix is always visible: the frame check covers every word of the backing
buffer -- with one exception that a second pattern closes.  A copying kernel (a gather, a transpose) that runs past
a row's end reads poison from its source's padding and stores it into its destination's padding: the same bits as
before.  So a pure input may be built with poison=POISON_INPUT, another quiet-NaN payload; its padding copied into
an output's frame is then a written word (without it only the `tight` layout, where such an overrun lands in the
next row or the guard rows, would notice).

The host image is built with numpy alone; PoisonView(..., device=False) keeps it in host memory so that the checks
themselves can be tested without a GPU (tests/test_kernel_views_host.py plants corruptions and expects each to be
caught and located).
"""
import numpy as np

POISON = np.uint32(0x7FC5A5A5)        # a quiet NaN with a recognisable payload
POISON_INPUT = np.uint32(0x7FC1D00D)  # the same for a pure input's buffer (see the module docstring)
GUARD = 3
LAYOUTS = ("tight", "offset", "shifted", "odd")


def roundup4(n):
    return (int(n) + 3) & ~3


def layout_geometry(cols, layout):
    """(c0, S) of a view of `cols` columns"""
    if layout == "tight":
        return 0, roundup4(cols)
    if layout == "offset":
        return 4, roundup4(cols) + 12
    if layout == "shifted":
        return 1, roundup4(cols) + 8
    if layout == "odd":
        return 1, int(cols) + 3
    raise ValueError(f"unknown layout {layout!r}")


def host_image(a, rows, cols, layout, dtype=np.float32, poison=POISON):
    """the backing buffer as flat uint32 words: poison everywhere, `a` (or poison, a is None) in the interior"""
    c0, S = layout_geometry(cols, layout)
    img = np.full((2 * GUARD + rows) * (c0 + S), poison, np.uint32)
    if a is not None:
        a = np.ascontiguousarray(np.asarray(a, dtype=dtype)).reshape(rows, -1)  # (cols counts words)
        img[interior_index(rows, cols, layout)] = a.view(np.uint32).reshape(-1)
    return img


def interior_index(rows, cols, layout):
    """flat word indices of the view's elements, row-major"""
    c0, S = layout_geometry(cols, layout)
    r = np.arange(rows, dtype=np.int64)[:, None]
    c = np.arange(cols, dtype=np.int64)[None, :]
    return ((GUARD + r) * S + c0 + c).reshape(-1)


def locate(idx, rows, cols, layout):
    """name the place of backing word idx relative to the view: (place, row, col); row / col in the view's own
    coordinates (a negative col: the c0 band before that row's first column)"""
    c0, S = layout_geometry(cols, layout)
    rel = int(idx) - (GUARD * S + c0)
    row, col = rel // S, rel % S
    if col >= S - c0:           # the last c0 words of a stride period precede the next row's column 0
        row, col = row + 1, col - S
    if row < 0:
        return "guard rows above", row, col
    if row >= rows:
        return "guard rows below", row, col
    if col < 0:
        return "c0 band", row, col
    if col >= cols:
        return "column padding", row, col
    return "interior", row, col


def frame_violation(raw, rows, cols, layout, poison=POISON):
    """None, or a message naming the first word outside [rows x cols] that is not the poison pattern"""
    raw = np.asarray(raw).view(np.uint32).reshape(-1)
    c0, S = layout_geometry(cols, layout)
    assert raw.size == (2 * GUARD + rows) * (c0 + S), "not this view's backing buffer"
    frame = np.ones(raw.size, bool)
    frame[interior_index(rows, cols, layout)] = False
    bad = np.flatnonzero(frame & (raw != poison))
    if bad.size == 0:
        return None
    place, r, c = locate(bad[0], rows, cols, layout)
    return (f"{bad.size} frame word(s) written; first in the {place} at (row {r}, col {c}) of a {rows} x {cols} "
            f"'{layout}' view: 0x{int(raw[bad[0]]):08x} (as float {raw[bad[0]:bad[0] + 1].view(np.float32)[0]!r})")


class PoisonView:
    def __init__(self, a, layout, rows=None, cols=None, dtype=None, device=True, poison=POISON):
        if a is not None:
            a = np.asarray(a)
            if a.ndim == 1:
                a = a.reshape(1, -1)
            rows, cols = a.shape
            dtype = dtype or (np.int32 if a.dtype.kind in "iu" else np.float32)
        self.rows, self.cols, self.layout = int(rows), int(cols), layout
        self.dtype = np.dtype(dtype or np.float32)
        assert self.dtype.itemsize in (4, 8)
        self.wpe = self.dtype.itemsize // 4  # words per element
        if self.wpe == 2 and layout not in ("tight", "offset"):
            raise ValueError(f"an 8-byte view exists only in the tight and offset layouts (c0 even), not in {layout!r}")
        self.wcols = self.cols * self.wpe    # the view's width in words: what the geometry and the checks use
        self.c0, self.wstride = layout_geometry(self.wcols, layout)
        assert self.wstride % self.wpe == 0 and (GUARD * self.wstride + self.c0) % self.wpe == 0
        self.stride = self.wstride // self.wpe  # in elements, as the kernels take it
        self._index = interior_index(self.rows, self.wcols, layout)
        self.poison = np.uint32(poison)
        img = host_image(a, self.rows, self.wcols, layout, self.dtype, self.poison)
        self.words = img.size
        self.initial = img.copy()  # what the buffer held before any call: the `before` of a pure input
        if device:
            from tnet_amd import DeviceArray
            self._host = None
            self.backing = DeviceArray(1, self.words, np.uint32, stride=self.words, zero=False)
            self.backing.upload(img.reshape(1, -1))
            self.ptr = self.backing.ptr + (GUARD * self.wstride + self.c0) * 4
        else:
            self._host, self.backing, self.ptr = img, None, None

    @classmethod
    def empty(cls, rows, cols, layout, dtype=np.float32, device=True):
        return cls(None, layout, rows, cols, dtype, device)

    @classmethod
    def vector(cls, v, layout, device=True, poison=POISON, dtype=None):
        return cls(np.asarray(v).reshape(1, -1), layout, dtype=dtype, device=device, poison=poison)

    @classmethod
    def empty_vector(cls, n, layout, dtype=np.float32, device=True):
        return cls(None, layout, 1, n, dtype, device)

    @property
    def dim(self):
        from tnet_amd._lib import MatrixDim
        return MatrixDim(self.rows, self.cols, self.stride)

    def raw(self):
        """the whole backing buffer as uint32 words (a copy)"""
        if self._host is not None:
            return self._host.copy()
        return self.backing.numpy().reshape(-1)

    def numpy(self):
        """the interior only"""
        return self.raw()[self._index].view(self.dtype).reshape(self.rows, self.cols)


def assert_frame_untouched(view, what="", raw=None):
    """`raw`: a view.raw() the caller already fetched (saves a second copy)"""
    msg = frame_violation(view.raw() if raw is None else raw, view.rows, view.wcols, view.layout, view.poison)
    assert msg is None, f"{what}: {msg}"


def assert_unchanged(view, before_raw, what=""):
    now = view.raw()
    bad = np.flatnonzero(now != np.asarray(before_raw).view(np.uint32).reshape(-1))
    if bad.size:
        place, r, c = locate(bad[0], view.rows, view.wcols, view.layout)
        raise AssertionError(f"{what}: a pure input changed: {bad.size} word(s), first in the {place} at "
                             f"(row {r}, col {c}) of a {view.rows} x {view.cols} '{view.layout}' view")
