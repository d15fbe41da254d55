"""The shared, discrete and sparse layer kernels (gemm_shared.hip, gemm_discrete.hip, gemm_sparse.hip on the tile core
gemm_tile.h) on caller-owned views.

tests/test_gpu_shared.py, test_gpu_discrete.py and test_gpu_sparse.py hand these kernels DeviceArrays: an allocation
base, 64-float strides, zero-filled padding, so every 16-byte switch of the tile core's loads is always on and a stray
read enters the product as 0 * w.  Here every operand is a PoisonView (tests/kernel_views.py) in one of
  tight    no padding where cols % 4 == 0, base 16-byte aligned
  offset   base 16-byte aligned and no more, rows neither 64-float nor 256-byte aligned
  shifted  base 4 bytes past a 16-byte boundary, stride a multiple of 4: the least the headers of these families allow;
           aligned16() of that operand is false, so its tiles go through load_tile's masked scalar side
  mixed-N  operand N `shifted`, every other one `offset` (N over the operands that carry a vec switch)
with pure inputs poisoned by POISON_INPUT.  After each call Frame.done() (tests/test_gpu_views.py) holds: status OK;
every output's and in-place operand's frame intact as uint32; no NaN in an interior (outputs start as poison); every
pure input bit-identical.  The interiors meet the bounds the entry points already have:
  forward / backward / gradient   |got - ref| <= 2e-5 * (|A||B|) + 1e-6 against float64 (test_gpu_shared.py)
  update: W                       2e-5 * |scale| * (|X|^T |E|) + 2e-7 * |W| + 1e-7; corr 2e-5 * (|X|^T |E|) + 1e-6;
                                  bias rtol 1e-5 atol 1e-6, its momentum rtol 1e-5 atol 1e-5 (test_shared_update,
                                  test_discrete_update)
  sparse update                   W, corrW, accu as test_sparse_update (2e-5 * [|scale|] * mag + 2e-7 * |ref| + 1e-7),
                                  exact zeros under the mask, bias as above; mask kernels exact
  gradients                       test_gpu_dp_layers.py's: 2e-5 * mag + 1e-6, bias rtol 1e-5 atol 1e-5
Bit equality: the vector and the scalar side of load_tile put the same values into the same LDS slots and tile and
slice choice depend on the shape alone, so every layout's result equals the `tight` one bit for bit -- asserted
everywhere except in the two loop-routed classes, where the 16-byte aligned layouts run the library's dense GEMM per
window / block and `shifted` must stay on the batched / grouped launch (for the discrete layer that is asserted too:
`shifted` equals `tight` with tnet_discrete_loop_routing(0), bit for bit).

Tiles and slices, worked out from pick_tile / plan_update / route (T: 2 = 64x64, 4 = 128x128; count = what pick_tile
compares with 200; Z = K slices; k-tile 16, slab 32):

shared (rows, n_inst, in, out)   forward            backward           update: plan count -> kchunk, kslices; launch
  (33, 3, 39, 10)                3 -> T2, grid 3    3 -> T2, grid 3    3 -> T2; 32, 2 (32 + 1 rows); Z 6, count 6, T2
  (70, 2, 72, 136)               4 -> T2, grid 12   2 -> T2, grid 8    4 -> T2; 32, 3 (32 + 32 + 6); Z 6, count 12, T2
  (37, 200, 5, 3)                200 -> T4, 200     200 -> T4, 200     200 -> T4; 32, 2 (32 + 5); Z 400, count 400, T4
  (130, 200, 8, 4)               400 -> T4, 400     400 -> T4, 400     200 -> T4; 64, 3 (64 + 64 + 2); Z 600, T4
      (two tile rows per instance forward and backward; steps 8 and 4: the vector side where the base allows it;
      steps 5, 3, 39, 10: the scalar side in every layout for X / E, W still by its base)
  (1024, 2, 512, 512)            rows*in*out = 2^28: per-window loop (tnet_affine_fwd / tnet_sgemm) in tight / offset;
                                 shifted / mixed: batched, 64 -> T2, grid 256
  tnet_shared_grad (20, 1, 12677, 135): cdiv(12677,128) * cdiv(135,128) = 100 * 2 = 200 -> T4; rows <= 32 and one
      instance: Z = 1, the DIRECT store from the accumulators, 200 workgroups in two tile columns
  (the update's plan takes T from n_inst, the launch from Z = n_inst * kslices: for (37, 200, 5, 3) 200 and 400, both
  T = 4 -- the plan's count is the one the issue's "200" names)

discrete (rows, blocks)                          forward (tile cols x rows)   backward              update
  (33, [(39,10),(1,7),(5,3)])                    3 x 1, T2                    3 x 1, T2             3 tiles, 2 slices
  (70, [(72,136),(8,8),(200,40)])                5 x 2, T2; k-tiles 5, 1, 13  7 x 2, T2; 9, 1, 3    11 tiles, 3 slices
                                                                                                    of 2, 2, 1 k-tiles
  BIG_FB (260, [(8519,13),(13,8519)])            68 x 3 = 204 >= 200, 675 >= 3 * 204: T4            --
  BIG_UPD (70, [(1300,1290),(900,1290)])         --                           --                    209 tiles (756 >=
                                                                                                    627): T4, 3 slices
  BIG_UPD's blocks at 20 rows, tnet_discrete_grad: one slice, the DIRECT T4 store into the packed gradient
  (512, RAGGED), (512, [(40,64),(120,256),(280,704)]): backward; 8 x 8 = 64 workgroups < 256, max out 704 >= 600:
      per-block loop in tight / offset (RAGGED through the staged copy and tnetF_rearrange), grouped T2 in shifted

sparse (rows, n_in, n_out), forms 1, 2, 1|0x20, 2|0x20: T2 or T4 as forced
  (33, 39, 10)    1 tile; sliced: 2 slices (32 + 1)        (16, 24, 33)   1 tile, 1 slice; a row of 2 mask words
  (70, 72, 136)   T2: 6 tiles, 3 slices; T4: 2 tiles, 3    (0, 8, 8)      K = 0: momentum, mask, L1, L2 only
  (40, 1290, 1601) form 0, shifted: 21 x 26 = 546 >= 512 tiles: the automatic single launch
mask kernels (rows, n_out): (3, 33) (4, 64) (5, 300: two 256-thread column blocks, a partial last word); ldmask
tight (= ceil(n_out/32)), padded (a multiple of 4 above it) and odd.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_gpu_discrete as td  # noqa: E402
import test_gpu_shared as ts  # noqa: E402
import test_gpu_sparse as tp  # noqa: E402
from kernel_views import POISON, POISON_INPUT, PoisonView  # noqa: E402
from test_gpu_views import TNET_ERR_ARG, Frame, S, within  # noqa: E402
from tnet_amd import DiscretePlan  # noqa: E402
from tnet_amd._lib import MatrixDim, lib  # noqa: E402

rnd = ts.rnd
BASE = ["tight", "offset", "shifted"]


def layouts(*mixed):
    return BASE + [f"mixed-{m}" for m in mixed]


class LFrame(Frame):
    """Frame with a layout per operand name: `mixed-N` puts operand N in `shifted` and the others in `offset`"""

    def lay(self, name):
        if self.layout.startswith("mixed-"):
            return "shifted" if name == self.layout[6:] else "offset"
        return self.layout

    def inp(self, a, name=None):
        return Frame.inp(self, a, self.lay(name))

    def inp_rows0(self, cols, name=None):
        """a pure input without rows: a valid pointer into a buffer that is poison throughout"""
        v = PoisonView(None, self.lay(name), 0, cols, poison=POISON_INPUT)
        self.ins.append(v)
        return v

    def out(self, rows, cols, name=None, dtype=np.float32):
        return Frame.out(self, rows, cols, self.lay(name), dtype)

    def io(self, a, name=None):
        return Frame.io(self, a, self.lay(name))

    def words(self, image, name, pure):
        """a flat uint32 image (packed parameters, a bit matrix with its row padding) as a 1 x n view: a pure input
        (poison POISON_INPUT around it) or an in-place operand / output"""
        v = PoisonView(np.asarray(image, np.uint32).reshape(1, -1), self.lay(name), dtype=np.uint32,
                       poison=POISON_INPUT if pure else POISON)
        (self.ins if pure else self.outs).append(v)
        return v


def same_bits(got, ref, what):
    a = np.ascontiguousarray(got).view(np.uint32)
    b = np.ascontiguousarray(ref).view(np.uint32)
    assert a.shape == b.shape, what
    bad = np.argwhere(a != b)
    at = tuple(bad[0]) if bad.size else ()
    assert not bad.size, f"{what}: {len(bad)} element(s) differ in bits from the tight layout's, first at {bad[0]}: " \
                         f"{np.ascontiguousarray(got)[at]!r} against {np.ascontiguousarray(ref)[at]!r}"


def same_bits_all(got, ref, what):
    assert got.keys() == ref.keys()
    for k in got:
        same_bits(got[k], ref[k], f"{what}: {k}")


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# =====================================================================================================================
# <sharedlinearity>
# =====================================================================================================================
SHARED_SHAPES = [(33, 3, 39, 10), (70, 2, 72, 136), (37, 200, 5, 3), (130, 200, 8, 4)]
SHARED_LOOP = (1024, 2, 512, 512)
SHARED_DIRECT = (20, 1, 12677, 135)
UPDATE_VARIANTS = [(0.0, True), (0.5, True), (0.0, False)]  # (mmt, corrW / corr_b given): test_shared_update's


def test_the_tile_table_of_the_docstring():
    """pick_tile's counts (gemm_shared.hip:142, gemm_tile.h:279) restated: which shapes reach T = 4"""
    def cdiv(a, b):
        return -(-a // b)

    def count(M, N, batch):
        return cdiv(M, 128) * cdiv(N, 128) * batch

    def plan(rows, n, n_in, n_out):
        T = 4 if count(n_in, n_out, n) >= 200 else 2
        tiles = cdiv(n_in, 32 * T) * cdiv(n_out, 32 * T)
        want = max(1, min(min(cdiv(512, tiles * n), 64), cdiv(max(rows, 1), 32)))
        kchunk = cdiv(cdiv(max(rows, 1), want), 32) * 32
        return count(n_in, n_out, n), kchunk, cdiv(max(rows, 1), kchunk)

    for (rows, n, n_in, n_out), fwd, bwd, upd in zip(SHARED_SHAPES, (3, 4, 200, 400), (3, 2, 200, 400),
                                                     ((3, 32, 2), (4, 32, 3), (200, 32, 2), (200, 64, 3))):
        assert count(rows, n_out, n) == fwd and count(rows, n_in, n) == bwd and plan(rows, n, n_in, n_out) == upd
    rows, n, n_in, n_out = SHARED_DIRECT
    assert plan(rows, n, n_in, n_out) == (200, 32, 1) and rows <= 32
    rows, n, n_in, n_out = SHARED_LOOP
    assert rows * n_in * n_out == 1 << 28 and count(rows, n_out, n) == 64 == count(rows, n_in, n)


def shared_loops(shape):
    rows, _, n_in, n_out = shape
    return rows * n_in * n_out >= 1 << 28 and (n_in | n_out) & 3 == 0


@functools.lru_cache(maxsize=None)
def shared_fwd_case(shape):
    rows, n, n_in, n_out = shape
    X, W, b = rnd((rows, n * n_in), 1), rnd((n_in, n_out), 2, 0.1), rnd(n_out, 3)
    return frozen(X, W, b, *ts.fwd_ref(X, W, b, n))


def run_shared_fwd(shape, layout):
    rows, n, n_in, n_out = shape
    X, W, b, z, mag = shared_fwd_case(shape)
    f = LFrame(layout, f"shared_fwd {shape} {layout}")
    vX, vW, vb = f.inp(X, "X"), f.inp(W, "W"), f.inp(b, "b")
    vY = f.out(rows, n * n_out, "Y")
    got, = f.done(lib().tnet_shared_fwd(vX.ptr, vX.dim, vW.ptr, vW.dim, vb.ptr, n, vY.ptr, vY.dim, S()))
    err = np.abs(got - z)
    print(f"{f.what}: max err / bound {float((err / (2e-5 * mag + 1e-6)).max()):.3f}")
    within(got, z, 2e-5 * mag + 1e-6, f.what)
    return got


shared_fwd_tight = functools.lru_cache(maxsize=None)(lambda shape: run_shared_fwd(shape, "tight"))


@pytest.mark.parametrize("layout", layouts("X", "W"))
@pytest.mark.parametrize("shape", SHARED_SHAPES + [SHARED_LOOP], ids=str)
def test_shared_fwd_views(shape, layout):
    if layout == "tight":
        shared_fwd_tight(shape)
    else:
        got = run_shared_fwd(shape, layout)
        if not shared_loops(shape):
            same_bits(got, shared_fwd_tight(shape), f"shared_fwd {shape} {layout}")


@functools.lru_cache(maxsize=None)
def shared_bwd_case(shape):
    rows, n, n_in, n_out = shape
    E, W = rnd((rows, n * n_out), 4), rnd((n_in, n_out), 5, 0.1)
    return frozen(E, W, *ts.bwd_ref(E, W, n))


def run_shared_bwd(shape, layout):
    rows, n, n_in, n_out = shape
    E, W, z, mag = shared_bwd_case(shape)
    f = LFrame(layout, f"shared_bwd {shape} {layout}")
    vE, vW = f.inp(E, "E"), f.inp(W, "W")
    vO = f.out(rows, n * n_in, "Eo")
    got, = f.done(lib().tnet_shared_bwd(vE.ptr, vE.dim, vW.ptr, vW.dim, n, vO.ptr, vO.dim, S()))
    err = np.abs(got - z)
    print(f"{f.what}: max err / bound {float((err / (2e-5 * mag + 1e-6)).max()):.3f}")
    within(got, z, 2e-5 * mag + 1e-6, f.what)
    return got


shared_bwd_tight = functools.lru_cache(maxsize=None)(lambda shape: run_shared_bwd(shape, "tight"))


@pytest.mark.parametrize("layout", layouts("E", "W"))
@pytest.mark.parametrize("shape", SHARED_SHAPES + [SHARED_LOOP], ids=str)
def test_shared_bwd_views(shape, layout):
    if layout == "tight":
        shared_bwd_tight(shape)
    else:
        got = run_shared_bwd(shape, layout)
        if not shared_loops(shape):
            same_bits(got, shared_bwd_tight(shape), f"shared_bwd {shape} {layout}")


@functools.lru_cache(maxsize=None)
def shared_upd_case(shape):
    rows, n, n_in, n_out = shape
    X, E = rnd((rows, n * n_in), 6), rnd((rows, n * n_out), 7, 0.01)
    W, corr = rnd((n_in, n_out), 8, 0.1), rnd((n_in, n_out), 9, 0.01)
    b, cb = rnd(n_out, 10), rnd(n_out, 11, 0.01)
    g, mag, gb, _ = ts.upd_ref(X, E, n, n_in, n_out)
    return frozen(X, E, W, corr, b, cb) + (g, mag, gb)


def run_shared_update(shape, layout, variant):
    """test_shared_update on views; X / E without rows where rows == 0 (K = 0: momentum and weight decay only)"""
    rows, n, n_in, n_out = shape
    mmt, with_corr = variant
    X, E, W, corr, b, cb, g, mag, gb = shared_upd_case(shape)
    scale, l2 = -0.3 / max(rows * n, 1), -1e-4
    f = LFrame(layout, f"shared_update {shape} {layout} mmt {mmt} corr {with_corr}")
    if rows:
        vX, vE = f.inp(X, "X"), f.inp(E, "E")
    else:
        vX, vE = f.inp_rows0(n * n_in, "X"), f.inp_rows0(n * n_out, "E")
    vW, vb = f.io(W, "W"), f.io(b, "b")
    vC, vcb = (f.io(corr, "corr"), f.io(cb, "cb")) if with_corr else (None, None)
    st = lib().tnet_shared_update(vX.ptr, vX.dim, vE.ptr, vE.dim, n, vW.ptr, vW.dim, vC.ptr if vC else None,
                                  vC.stride if vC else 0, vb.ptr, vcb.ptr if vcb else None, scale, mmt, l2, S())
    got = dict(zip(("W", "b", "corr", "cb"), f.done(st)))
    c = g + mmt * corr if with_corr else g   # with momentum 0 the kernel still stores c = g + 0 * corr
    w = W + scale * c
    w = w + l2 * w
    tol = 2e-5 * abs(scale) * mag + 2e-7 * np.abs(W) + 1e-7
    print(f"{f.what}: W max err / tol {float((np.abs(got['W'] - w) / tol).max()):.3f}")
    within(got["W"], w, tol, f.what + " W")
    cbr = gb + mmt * cb if with_corr else gb
    np.testing.assert_allclose(got["b"].reshape(-1), b + scale * cbr, rtol=1e-5, atol=1e-6)
    if with_corr:
        within(got["corr"], c, 2e-5 * mag + 1e-6, f.what + " corrW")
        np.testing.assert_allclose(got["cb"].reshape(-1), cbr, rtol=1e-5, atol=1e-5)
    return got


shared_update_tight = functools.lru_cache(maxsize=None)(lambda shape, v: run_shared_update(shape, "tight", v))


@pytest.mark.parametrize("layout", layouts("X", "E"))
@pytest.mark.parametrize("shape", SHARED_SHAPES + [(0, 3, 39, 10)], ids=str)
def test_shared_update_views(shape, layout):
    for variant in UPDATE_VARIANTS:
        if layout == "tight":
            shared_update_tight(shape, variant)
        else:
            same_bits_all(run_shared_update(shape, layout, variant), shared_update_tight(shape, variant),
                          f"shared_update {shape} {layout} {variant}")


@functools.lru_cache(maxsize=None)
def shared_grad_case(shape):
    rows, n, n_in, n_out = shape
    X, E = rnd((rows, n * n_in), 1), rnd((rows, n * n_out), 2, 0.01)
    g, mag, gb, _ = ts.upd_ref(X, E, n, n_in, n_out)
    return frozen(X, E) + (g, mag, gb)


def run_shared_grad(shape, layout):
    rows, n, n_in, n_out = shape
    X, E, g, mag, gb = shared_grad_case(shape)
    f = LFrame(layout, f"shared_grad {shape} {layout}")
    vX, vE = f.inp(X, "X"), f.inp(E, "E")
    vG, vB = f.out(n_in, n_out, "G"), f.out(1, n_out, "gradB")
    G, B = f.done(lib().tnet_shared_grad(vX.ptr, vX.dim, vE.ptr, vE.dim, n, vG.ptr, vG.dim, vB.ptr, S()))
    print(f"{f.what}: max err / bound {float((np.abs(G - g) / (2e-5 * mag + 1e-6)).max()):.3f}")
    within(G, g, 2e-5 * mag + 1e-6, f.what)
    np.testing.assert_allclose(B.reshape(-1), gb, rtol=1e-5, atol=1e-5)
    return dict(G=G, gradB=B)


shared_grad_tight = functools.lru_cache(maxsize=None)(lambda shape: run_shared_grad(shape, "tight"))


@pytest.mark.parametrize("layout", layouts("X", "E"))
@pytest.mark.parametrize("shape", [SHARED_DIRECT, (37, 200, 5, 3)], ids=str)
def test_shared_grad_views_128_tile(shape, layout):
    """T = 4 in the DIRECT form (one slice: the accumulators go straight to G, the column sums to gradB) and through
    the workspace and the slice sum (400 slices)"""
    if layout == "tight":
        shared_grad_tight(shape)
    else:
        same_bits_all(run_shared_grad(shape, layout), shared_grad_tight(shape), f"shared_grad {shape} {layout}")


def test_shared_rejections():
    """a stride off 4 and a base off 4 bytes, operand by operand: TNET_ERR_ARG, nothing written"""
    rows, n, n_in, n_out = 5, 2, 8, 4
    L, s = lib(), S()
    f = LFrame("offset", "shared rejections")
    v = dict(X=f.inp(rnd((rows, n * n_in), 1)), E=f.inp(rnd((rows, n * n_out), 2)), W=f.io(rnd((n_in, n_out), 3)),
             Y=f.out(rows, n * n_out), Eo=f.out(rows, n * n_in), C=f.io(rnd((n_in, n_out), 4)), b=f.io(rnd(n_out, 5)),
             cb=f.io(rnd(n_out, 6)), G=f.out(n_in, n_out), gB=f.out(1, n_out))

    def P(k, bad):
        return v[k].ptr + 2 * (bad == ("p", k))

    def D(k, bad):
        return MatrixDim(v[k].rows, v[k].cols, v[k].stride + 2 * (bad == ("s", k)))

    calls = {
        "fwd": (lambda x: L.tnet_shared_fwd(P("X", x), D("X", x), P("W", x), D("W", x), P("b", x), n, P("Y", x),
                                            D("Y", x), s), "XWY", "b"),
        "bwd": (lambda x: L.tnet_shared_bwd(P("E", x), D("E", x), P("W", x), D("W", x), n, P("Eo", x), D("Eo", x), s),
                ("E", "W", "Eo"), ()),
        "update": (lambda x: L.tnet_shared_update(P("X", x), D("X", x), P("E", x), D("E", x), n, P("W", x), D("W", x),
                                                  P("C", x), D("C", x).stride, P("b", x), P("cb", x), -0.1, 0.5, 0.0,
                                                  s), "XEWC", ("b", "cb")),
        "grad": (lambda x: L.tnet_shared_grad(P("X", x), D("X", x), P("E", x), D("E", x), n, P("G", x), D("G", x),
                                              P("gB", x), s), "XEG", ("gB",)),
    }
    for name, (call, mats, vecs) in calls.items():
        for k in mats:
            f.what = f"shared_{name}: stride of {k} off 4"
            f.rejected(call(("s", k)))
        for k in tuple(mats) + tuple(vecs):
            f.what = f"shared_{name}: base of {k} off 4 bytes"
            f.rejected(call(("p", k)))


# =====================================================================================================================
# <discretelinearity>
# =====================================================================================================================
def T(blocks):
    return tuple(tuple(b) for b in blocks)


D_SMALL = [(33, T([(39, 10), (1, 7), (5, 3)])), (70, T([(72, 136), (8, 8), (200, 40)]))]
BIG_FB, BIG_UPD = (td.BIG_FB[0], T(td.BIG_FB[1])), (td.BIG_UPD[0], T(td.BIG_UPD[1]))
D_LOOP = [(td.LOOP_SHAPES[0][0], T(td.LOOP_SHAPES[0][1])), (td.LOOP_SHAPES[3][0], T(td.LOOP_SHAPES[3][1]))]
D_IDS = td.ids


@functools.lru_cache(maxsize=None)
def plan_for(blocks):
    return DiscretePlan(blocks)


def sums(blocks):
    return sum(b[0] for b in blocks), sum(b[1] for b in blocks)


def test_the_discrete_shapes_of_the_docstring():
    """pick_tile (gemm_discrete.hip) restated for the shapes that must reach T = 4, and loop_class for those that
    must be routed"""
    def cdiv(a, b):
        return -(-a // b)

    def tile(blocks, rows, width):
        big = sum(width(b, 128) for b in blocks) * (cdiv(rows, 128) if rows else 1)
        small = sum(width(b, 64) for b in blocks) * (cdiv(rows, 64) if rows else 1)
        return 4 if big >= 200 and small >= 3 * big else 2

    rows, blocks = BIG_FB
    assert tile(blocks, rows, lambda b, t: cdiv(b[1], t)) == 4 and tile(blocks, rows, lambda b, t: cdiv(b[0], t)) == 4
    rows, blocks = BIG_UPD
    assert tile(blocks, 0, lambda b, t: cdiv(b[0], t) * cdiv(b[1], t)) == 4
    for rows, blocks in D_SMALL:
        assert tile(blocks, 0, lambda b, t: cdiv(b[0], t) * cdiv(b[1], t)) == 2
    for rows, blocks in D_LOOP:
        assert rows >= 512 and sum(cdiv(b[0], 64) for b in blocks) * cdiv(rows, 64) < 256
        assert max(b[1] for b in blocks) >= 200 * len(blocks) and all(b[1] % 4 == 0 for b in blocks)


def packed_image(plan, Ws, poison):
    """the blocks in the plan's layout as uint32 words, `poison` in the stride padding [out_k, ld_k)"""
    out = np.full(plan.floats, poison, np.uint32)
    fl = out.view(np.float32)
    for W, (ni, no), (off, ld) in zip(Ws, plan.blocks, plan.layout):
        fl[off:off + ni * ld].reshape(ni, ld)[:, :no] = W
    return out


def unpack_checked(plan, words, poison, what):
    """the blocks of a packed buffer; its stride padding must still hold the poison"""
    words = np.ascontiguousarray(words).reshape(-1)
    pad = plan.padding(words)
    assert np.all(pad == poison), f"{what}: {int((pad != poison).sum())} word(s) of the stride padding written"
    return plan.unpack(words.view(np.float32))


def discrete_loops(shape):
    return shape in D_LOOP


@functools.lru_cache(maxsize=None)
def discrete_fwd_case(shape):
    rows, blocks = shape
    n_in, n_out = sums(blocks)
    X, Ws, b = rnd((rows, n_in), 1), td.gen_blocks(blocks, 2), rnd(n_out, 3)
    return frozen(X, b, *Ws)[:2] + (Ws,) + td.fwd_ref(X, Ws, b)


def run_discrete_fwd(shape, layout):
    rows, blocks = shape
    plan = plan_for(blocks)
    X, b, Ws, z, mag = discrete_fwd_case(shape)
    f = LFrame(layout, f"discrete_fwd {D_IDS([shape])[0]} {layout}")
    vX, vb = f.inp(X, "X"), f.inp(b, "b")
    vW = f.words(packed_image(plan, Ws, POISON_INPUT), "W", pure=True)
    vY = f.out(rows, sums(blocks)[1], "Y")
    got, = f.done(lib().tnet_discrete_fwd(vX.ptr, vX.dim, vW.ptr, plan.ptr, vb.ptr, vY.ptr, vY.dim, S()))
    print(f"{f.what}: max err / bound {float((np.abs(got - z) / (2e-5 * mag + 1e-6)).max()):.3f}")
    within(got, z, 2e-5 * mag + 1e-6, f.what)
    return got


discrete_fwd_tight = functools.lru_cache(maxsize=None)(lambda shape: run_discrete_fwd(shape, "tight"))


@pytest.mark.parametrize("layout", layouts("X", "W"))
@pytest.mark.parametrize("shape", D_SMALL + [BIG_FB], ids=D_IDS(D_SMALL + [BIG_FB]))
def test_discrete_fwd_views(shape, layout):
    if layout == "tight":
        discrete_fwd_tight(shape)
    else:
        same_bits(run_discrete_fwd(shape, layout), discrete_fwd_tight(shape), f"discrete_fwd {layout}")


@functools.lru_cache(maxsize=None)
def discrete_bwd_case(shape):
    rows, blocks = shape
    E, Ws = rnd((rows, sums(blocks)[1]), 4), td.gen_blocks(blocks, 5)
    frozen(E, *Ws)
    return (E, Ws) + td.bwd_ref(E, Ws)


def run_discrete_bwd(shape, layout, routing=1):
    rows, blocks = shape
    plan = plan_for(blocks)
    E, Ws, z, mag = discrete_bwd_case(shape)
    f = LFrame(layout, f"discrete_bwd {D_IDS([shape])[0]} {layout} routing {routing}")
    vE = f.inp(E, "E")
    vW = f.words(packed_image(plan, Ws, POISON_INPUT), "W", pure=True)
    vO = f.out(rows, sums(blocks)[0], "Eo")
    lib().tnet_discrete_loop_routing(routing)
    try:
        st = lib().tnet_discrete_bwd(vE.ptr, vE.dim, vW.ptr, plan.ptr, vO.ptr, vO.dim, S())
    finally:
        lib().tnet_discrete_loop_routing(1)
    got, = f.done(st)
    print(f"{f.what}: max err / bound {float((np.abs(got - z) / (2e-5 * mag + 1e-6)).max()):.3f}")
    within(got, z, 2e-5 * mag + 1e-6, f.what)
    return got


discrete_bwd_tight = functools.lru_cache(maxsize=None)(lambda shape: run_discrete_bwd(shape, "tight"))
discrete_bwd_grouped = functools.lru_cache(maxsize=None)(lambda shape: run_discrete_bwd(shape, "tight", routing=0))


@pytest.mark.parametrize("layout", layouts("E", "W"))
@pytest.mark.parametrize("shape", D_SMALL + [BIG_FB] + D_LOOP, ids=D_IDS(D_SMALL + [BIG_FB] + D_LOOP))
def test_discrete_bwd_views(shape, layout):
    """the routed class: tight / offset take the per-block loop (RAGGED writes the staged copy and scatters it onto Eo,
    whose stripe origins 39 and 159 are off 16 bytes), an operand that is only 4-byte aligned keeps the call on the
    grouped launch -- which then gives the grouped launch's bits"""
    if layout == "tight":
        discrete_bwd_tight(shape)
        return
    got = run_discrete_bwd(shape, layout)
    if not discrete_loops(shape):
        same_bits(got, discrete_bwd_tight(shape), f"discrete_bwd {layout}")
    elif layout != "offset":
        same_bits(got, discrete_bwd_grouped(shape), f"discrete_bwd {layout} against the grouped launch")


@functools.lru_cache(maxsize=None)
def discrete_upd_case(shape):
    rows, blocks = shape
    n_in, n_out = sums(blocks)
    X, E = rnd((rows, n_in), 6), rnd((rows, n_out), 7, 0.01)
    Ws, corrs = td.gen_blocks(blocks, 8), td.gen_blocks(blocks, 9, 0.01)
    b, cb = rnd(n_out, 10), rnd(n_out, 11, 0.01)
    frozen(X, E, b, cb, *Ws, *corrs)
    return (X, E, Ws, corrs, b, cb) + td.upd_ref(X, E, blocks)


def run_discrete_update(shape, layout, variant):
    """test_discrete_update on views: Wp and corrp are 1 x floats views whose stride padding is poison as well"""
    rows, blocks = shape
    mmt, with_corr = variant
    plan = plan_for(blocks)
    X, E, Ws, corrs, b, cb, g, mag, gb = discrete_upd_case(shape)
    scale, l2 = -0.3 / max(rows, 1), -1e-4
    f = LFrame(layout, f"discrete_update {D_IDS([shape])[0]} {layout} mmt {mmt} corr {with_corr}")
    if rows:
        vX, vE = f.inp(X, "X"), f.inp(E, "E")
    else:
        vX, vE = f.inp_rows0(sums(blocks)[0], "X"), f.inp_rows0(sums(blocks)[1], "E")
    vW, vb = f.words(packed_image(plan, Ws, POISON), "W", pure=False), f.io(b, "b")
    vC, vcb = (f.words(packed_image(plan, corrs, POISON), "corr", pure=False), f.io(cb, "cb")) if with_corr \
        else (None, None)
    st = lib().tnet_discrete_update(vX.ptr, vX.dim, vE.ptr, vE.dim, plan.ptr, vW.ptr, vC.ptr if vC else None, vb.ptr,
                                    vcb.ptr if vcb else None, scale, mmt, l2, S())
    got = dict(zip(("W", "b", "corr", "cb"), f.done(st)))
    got_w = unpack_checked(plan, got["W"], POISON, f.what + " Wp")
    got_c = unpack_checked(plan, got["corr"], POISON, f.what + " corrp") if with_corr else None
    for k, W in enumerate(Ws):
        c = g[k] + mmt * corrs[k] if with_corr else g[k]
        w = W + scale * c
        w = w + l2 * w
        within(got_w[k], w, 2e-5 * abs(scale) * mag[k] + 2e-7 * np.abs(W) + 1e-7, f"{f.what} W_{k}")
        if with_corr:
            within(got_c[k], c, 2e-5 * mag[k] + 1e-6, f"{f.what} corr_{k}")
    cbr = gb + mmt * cb if with_corr else gb
    np.testing.assert_allclose(got["b"].reshape(-1), b + scale * cbr, rtol=1e-5, atol=1e-6)
    if with_corr:
        np.testing.assert_allclose(got["cb"].reshape(-1), cbr, rtol=1e-5, atol=1e-5)
    return got


discrete_update_tight = functools.lru_cache(maxsize=None)(lambda shape, v: run_discrete_update(shape, "tight", v))
D_UPD = D_SMALL + [(0, T([(5, 3), (2, 6)])), BIG_UPD]


@pytest.mark.parametrize("layout", layouts("X", "E"))
@pytest.mark.parametrize("shape", D_UPD, ids=D_IDS(D_UPD))
def test_discrete_update_views(shape, layout):
    """(the update reads W only in the combine launch, element by element: X and E carry its vec switches)"""
    for variant in (UPDATE_VARIANTS[1:2] if shape == BIG_UPD else UPDATE_VARIANTS):  # BIG_UPD: 11 MB a buffer
        if layout == "tight":
            discrete_update_tight(shape, variant)
        else:
            same_bits_all(run_discrete_update(shape, layout, variant), discrete_update_tight(shape, variant),
                          f"discrete_update {layout} {variant}")


BIG_GRAD = (20, BIG_UPD[1])  # rows <= 32: one slice, T = 4 -- tests/test_gpu_dp_layers.py's blocks stay at T = 2


@functools.lru_cache(maxsize=None)
def discrete_grad_case(shape):
    rows, blocks = shape
    n_in, n_out = sums(blocks)
    X, E = rnd((rows, n_in), 3), rnd((rows, n_out), 4, 0.01)
    return frozen(X, E) + td.upd_ref(X, E, blocks)


def run_discrete_grad(shape, layout):
    rows, blocks = shape
    plan = plan_for(blocks)
    X, E, g, mag, gb = discrete_grad_case(shape)
    f = LFrame(layout, f"discrete_grad {D_IDS([shape])[0]} {layout}")
    vX, vE = f.inp(X, "X"), f.inp(E, "E")
    vG, vB = f.out(1, plan.floats, "G", np.uint32), f.out(1, sums(blocks)[1], "gradB")
    Gp, B = f.done(lib().tnet_discrete_grad(vX.ptr, vX.dim, vE.ptr, vE.dim, plan.ptr, vG.ptr, vB.ptr, S()))
    for k, G in enumerate(unpack_checked(plan, Gp, POISON, f.what + " Gp")):
        within(G, g[k], 2e-5 * mag[k] + 1e-6, f"{f.what} G_{k}")   # (an unwritten element is poison: NaN fails)
    np.testing.assert_allclose(B.reshape(-1), gb, rtol=1e-5, atol=1e-5)
    return dict(Gp=Gp, gradB=B)


discrete_grad_tight = functools.lru_cache(maxsize=None)(lambda shape: run_discrete_grad(shape, "tight"))


@pytest.mark.parametrize("layout", layouts("X", "E"))
def test_discrete_grad_views_direct_128_tile(layout):
    if layout == "tight":
        discrete_grad_tight(BIG_GRAD)
    else:
        same_bits_all(run_discrete_grad(BIG_GRAD, layout), discrete_grad_tight(BIG_GRAD), f"discrete_grad {layout}")


def test_discrete_rejections():
    rows, blocks = 5, T([(8, 4), (3, 5)])
    plan = plan_for(blocks)
    n_in, n_out = sums(blocks)
    L, s = lib(), S()
    f = LFrame("offset", "discrete rejections")
    Ws = td.gen_blocks(blocks, 1)
    v = dict(X=f.inp(rnd((rows, n_in), 1)), E=f.inp(rnd((rows, n_out), 2)), Y=f.out(rows, n_out), Eo=f.out(rows, n_in),
             W=f.words(packed_image(plan, Ws, POISON), "W", pure=False),
             C=f.words(packed_image(plan, Ws, POISON), "C", pure=False), b=f.io(rnd(n_out, 5)), cb=f.io(rnd(n_out, 6)),
             G=f.out(1, plan.floats, None, np.uint32), gB=f.out(1, n_out))

    def P(k, bad):
        return v[k].ptr + 2 * (bad == ("p", k))

    def D(k, bad):
        return MatrixDim(v[k].rows, v[k].cols, v[k].stride + 2 * (bad == ("s", k)))

    calls = {
        "fwd": (lambda x: L.tnet_discrete_fwd(P("X", x), D("X", x), P("W", x), plan.ptr, P("b", x), P("Y", x),
                                              D("Y", x), s), "XY", ("W", "b")),
        "bwd": (lambda x: L.tnet_discrete_bwd(P("E", x), D("E", x), P("W", x), plan.ptr, P("Eo", x), D("Eo", x), s),
                ("E", "Eo"), ("W",)),
        "update": (lambda x: L.tnet_discrete_update(P("X", x), D("X", x), P("E", x), D("E", x), plan.ptr, P("W", x),
                                                    P("C", x), P("b", x), P("cb", x), -0.1, 0.5, 0.0, s),
                   "XE", ("W", "C", "b", "cb")),
        "grad": (lambda x: L.tnet_discrete_grad(P("X", x), D("X", x), P("E", x), D("E", x), plan.ptr, P("G", x),
                                                P("gB", x), s), "XE", ("G", "gB")),
    }
    for name, (call, mats, vecs) in calls.items():
        for k in mats:
            f.what = f"discrete_{name}: stride of {k} off 4"
            f.rejected(call(("s", k)))
        for k in tuple(mats) + tuple(vecs):
            f.what = f"discrete_{name}: base of {k} off 4 bytes"
            f.rejected(call(("p", k)))


# =====================================================================================================================
# <sparselinearity>
# =====================================================================================================================
SPARSE_SHAPES = [(33, 39, 10), (16, 24, 33), (70, 72, 136), (0, 8, 8)]
SPARSE_FORMS = [tp.FORM_SINGLE, tp.FORM_SLICED, tp.FORM_SINGLE | tp.TILE128, tp.FORM_SLICED | tp.TILE128]
# the mask's word stride, rotated over the layouts (the header allows any ldmask >= ceil(n_out / 32))
LDMASK_OF = {"tight": "tight", "offset": "padded", "shifted": "odd", "mixed-X": "padded", "mixed-E": "odd"}


def ldmask_for(n_out, kind):
    nwords = (n_out + 31) // 32
    if kind == "tight":
        return nwords
    if kind == "padded":
        return ((nwords + 3) & ~3) + 4
    return nwords + 1 if nwords % 2 == 0 else nwords + 2   # odd, and above the row's words


def mask_image(mask, ldmask, poison):
    """the bit matrix as flat words, `poison` in the words past ceil(cols / 32) of every row"""
    return tp.pack_host(mask, ldmask, fill=int(poison)).reshape(-1)


@pytest.fixture
def sparse_form():
    """the form knob is a global of the library: back to the automatic choice whatever a test did"""
    yield lib().tnet_sparse_update_form
    lib().tnet_sparse_update_form(tp.FORM_AUTO)


@functools.lru_cache(maxsize=None)
def sparse_case(shape):
    rows, n_in, n_out = shape
    X, E, W, corr, accu, mask, b, cb = tp.inputs(rows, n_in, n_out, 0.3)
    scale, mmt, l2 = -0.3 / max(rows, 1), 0.5, -1e-4
    alive = np.abs(W[mask != 0])
    l1c = float(np.quantile(alive, 1 / 3))   # test_sparse_update's: a third of the surviving weights fall under it
    ref = tp.update_ref(X, E, W, corr, accu, mask, b, cb, scale, mmt, l1c, l2)
    return frozen(X, E, W, corr, accu, mask, b, cb) + ((scale, mmt, l1c, l2), ref)


def run_sparse_update(shape, form, layout):
    rows, n_in, n_out = shape
    X, E, W, corr, accu, mask, b, cb, (scale, mmt, l1c, l2), ref = sparse_case(shape)
    ldmask = ldmask_for(n_out, LDMASK_OF[layout])
    f = LFrame(layout, f"sparse_update {shape} form {form:#x} {layout} ldmask {ldmask}")
    if rows:
        vX, vE = f.inp(X, "X"), f.inp(E, "E")
    else:
        vX, vE = f.inp_rows0(n_in, "X"), f.inp_rows0(n_out, "E")
    vW, vC, vA = f.io(W, "W"), f.io(corr, "corr"), f.io(accu, "accu")
    vb, vcb = f.io(b, "b"), f.io(cb, "cb")
    vM = f.words(mask_image(mask, ldmask, POISON_INPUT), "bits", pure=True)
    lib().tnet_sparse_update_form(form)
    try:
        st = lib().tnet_sparse_update(vX.ptr, vX.dim, vE.ptr, vE.dim, vW.ptr, vW.dim, vC.ptr, vC.stride, vA.ptr,
                                      vA.stride, vM.ptr, ldmask, vb.ptr, vcb.ptr, scale, mmt, l1c, l2, S())
    finally:
        lib().tnet_sparse_update_form(tp.FORM_AUTO)
    got = dict(zip(("W", "corr", "accu", "b", "cb"), f.done(st)))
    within(got["W"], ref["W"], 2e-5 * abs(scale) * ref["mag"] + 2e-7 * np.abs(ref["W"]) + 1e-7, f.what + " W")
    within(got["corr"], ref["corr"], 2e-5 * ref["mag"] + 2e-7 * np.abs(ref["corr"]) + 1e-7, f.what + " corrW")
    within(got["accu"], ref["accu"], 2e-5 * ref["mag"] + 2e-7 * np.abs(ref["accu"]) + 1e-7, f.what + " accu")
    assert np.all(got["W"][mask == 0] == 0.0), f.what                # exactly 0.0 under the mask
    np.testing.assert_allclose(got["b"].reshape(-1), ref["b"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["cb"].reshape(-1), ref["cb"], rtol=1e-5, atol=1e-5)
    return got


sparse_update_tight = functools.lru_cache(maxsize=None)(lambda shape, form: run_sparse_update(shape, form, "tight"))


@pytest.mark.parametrize("layout", layouts("X", "E"))
@pytest.mark.parametrize("shape", SPARSE_SHAPES, ids=str)
def test_sparse_update_views(shape, layout, sparse_form):
    for form in SPARSE_FORMS:
        if layout == "tight":
            sparse_update_tight(shape, form)
        else:
            same_bits_all(run_sparse_update(shape, form, layout), sparse_update_tight(shape, form),
                          f"sparse_update {shape} form {form:#x} {layout}")


def test_sparse_update_views_automatic_single_launch(sparse_form):
    """546 tiles of 64x64: the automatic choice is the single launch, here with X and E through the scalar loads"""
    run_sparse_update(tp.PAST, tp.FORM_AUTO, "shifted")


MASK_SHAPES = [(3, 33), (4, 64), (5, 300)]
LDMASK_KINDS = ["tight", "padded", "odd"]


@pytest.mark.parametrize("layout", BASE)
@pytest.mark.parametrize("rows,n_out", MASK_SHAPES)
def test_mask_pack_unpack_views(rows, n_out, layout):
    """test_mask_pack_unpack on views: every word below ceil(n_out / 32) written (they start as poison), bits at
    columns >= n_out zero, the words past it still poison; the float matrix comes back exactly"""
    mask = tp.draw_mask((rows, n_out), 0.5, 400 + n_out)
    nwords = (n_out + 31) // 32
    for kind in LDMASK_KINDS:
        ldmask = ldmask_for(n_out, kind)
        assert ldmask >= nwords and (kind != "odd" or ldmask % 2 == 1) and (kind != "tight" or ldmask == nwords)
        f = LFrame(layout, f"mask_pack {rows} x {n_out} {layout} ldmask {ldmask}")
        vF = f.inp(mask * 2.5)                                       # any nonzero value is a 1
        vM = f.out(1, rows * ldmask, None, np.uint32)
        words, = f.done(lib().tnet_sparse_mask_pack(vF.ptr, vF.dim, vM.ptr, ldmask, S()))
        words = words.reshape(rows, ldmask)
        np.testing.assert_array_equal(words, tp.pack_host(mask, ldmask, fill=int(POISON)), err_msg=f.what)
        if n_out % 32:
            assert np.all(words[:, nwords - 1] >> np.uint32(n_out % 32) == 0)
        f = LFrame(layout, f"mask_unpack {rows} x {n_out} {layout} ldmask {ldmask}")
        vM = f.words(mask_image(mask, ldmask, POISON_INPUT), "bits", pure=True)
        vO = f.out(rows, n_out)
        got, = f.done(lib().tnet_sparse_mask_unpack(vM.ptr, ldmask, vO.ptr, vO.dim, S()))
        np.testing.assert_array_equal(got, mask, err_msg=f.what)


@pytest.mark.parametrize("layout", BASE)
@pytest.mark.parametrize("rows,n_out", MASK_SHAPES)
def test_mask_update_views(rows, n_out, layout):
    """test_mask_update_is_exact's data on views: W and the bit matrix in place, accu a pure input"""
    thr, unsp, nframes = np.float32(1e-3), np.float32(0.5), 960
    rng = np.random.default_rng(500 + n_out)
    mask = tp.draw_mask((rows, n_out), 0.5, 501 + n_out)
    pool = np.array([thr, np.nextafter(thr, np.float32(0)), -thr, -np.nextafter(thr, np.float32(0)), 0.0, 5e-4, -5e-4,
                     2e-3, -0.3, np.nextafter(thr, np.float32(1))], np.float32)
    W = pool[rng.integers(0, len(pool), (rows, n_out))]
    edge = np.float32(unsp * np.float32(nframes))
    apool = np.array([edge, np.nextafter(edge, np.float32(np.inf)), -np.nextafter(edge, np.float32(np.inf)), -edge,
                      0.0, 0.25 * edge, -4.0 * edge, 3.0 * edge], np.float32)
    accu = apool[rng.integers(0, len(apool), (rows, n_out))]
    Wr, mr = tp.mask_update_ref(W, mask, accu, thr, unsp, nframes)
    assert (mr != mask).any()
    for kind in LDMASK_KINDS:
        ldmask = ldmask_for(n_out, kind)
        f = LFrame(layout, f"mask_update {rows} x {n_out} {layout} ldmask {ldmask}")
        vW, vA = f.io(W), f.inp(accu)
        vM = f.words(mask_image(mask, ldmask, POISON), "bits", pure=False)
        st = lib().tnet_sparse_mask_update(vW.ptr, vW.dim, vM.ptr, ldmask, vA.ptr, vA.stride, float(thr), float(unsp),
                                           float(nframes), S())
        gotW, words = f.done(st)
        np.testing.assert_array_equal(words.reshape(rows, ldmask), tp.pack_host(mr, ldmask, fill=int(POISON)),
                                      err_msg=f.what)
        np.testing.assert_array_equal(gotW.view(np.uint32), Wr.view(np.uint32), err_msg=f.what)


def test_sparse_rejections():
    rows, n_in, n_out = 5, 8, 40
    L, s = lib(), S()
    f = LFrame("offset", "sparse rejections")
    mask = tp.draw_mask((n_in, n_out), 0.5, 7)
    v = dict(X=f.inp(rnd((rows, n_in), 1)), E=f.inp(rnd((rows, n_out), 2)), W=f.io(rnd((n_in, n_out), 3)),
             C=f.io(rnd((n_in, n_out), 4)), A=f.io(rnd((n_in, n_out), 5)), b=f.io(rnd(n_out, 6)),
             cb=f.io(rnd(n_out, 7)),
             M=f.words(mask_image(mask, 3, POISON), "bits", pure=False), F=f.io(mask), G=f.out(n_in, n_out),
             gB=f.out(1, n_out))

    def P(k, bad):
        return v[k].ptr + 2 * (bad == ("p", k))

    def D(k, bad):
        return MatrixDim(v[k].rows, v[k].cols, v[k].stride + 2 * (bad == ("s", k)))

    calls = {
        "update": (lambda x: L.tnet_sparse_update(P("X", x), D("X", x), P("E", x), D("E", x), P("W", x), D("W", x),
                                                  P("C", x), D("C", x).stride, P("A", x), D("A", x).stride, P("M", x),
                                                  3, P("b", x), P("cb", x), -0.1, 0.5, 0.0, 0.0, s),
                   "XEWCA", ("M", "b", "cb")),
        "grad": (lambda x: L.tnet_sparse_grad(P("X", x), D("X", x), P("E", x), D("E", x), P("G", x), D("G", x),
                                              P("gB", x), s), "XEG", ("gB",)),
        "apply": (lambda x: L.tnet_sparse_apply(P("W", x), D("W", x), P("F", x), D("F", x).stride, P("C", x),
                                                D("C", x).stride, P("A", x), D("A", x).stride, P("M", x), 3, 0,
                                                n_in * v["W"].stride, -0.1, 0.5, 0.0, 0.0, s), "WFCA", ("M",)),
        "mask_pack": (lambda x: L.tnet_sparse_mask_pack(P("F", x), D("F", x), P("M", x), 3, s), "F", ("M",)),
        "mask_unpack": (lambda x: L.tnet_sparse_mask_unpack(P("M", x), 3, P("F", x), D("F", x), s), "F", ("M",)),
        "mask_update": (lambda x: L.tnet_sparse_mask_update(P("W", x), D("W", x), P("M", x), 3, P("A", x),
                                                            D("A", x).stride, 1e-3, 0.5, 1.0, s), "WA", ("M",)),
    }
    for name, (call, mats, vecs) in calls.items():
        for k in mats:
            f.what = f"sparse_{name}: stride of {k} off 4"
            f.rejected(call(("s", k)))
        for k in tuple(mats) + tuple(vecs):
            f.what = f"sparse_{name}: base of {k} off 4 bytes"
            f.rejected(call(("p", k)))
