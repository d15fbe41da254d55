"""The dense kernels (gemm_f32.hip, reduce.hip, elementwise.hip, frontend.hip) on caller-owned views.

Every other kernel test hands the kernels DeviceArrays: a hipMalloc base, a stride that is a multiple of 64 floats,
zero-filled padding that numpy() drops again.  Here every operand is a PoisonView (tests/kernel_views.py): a tight or
offset (or, where the header allows any stride, odd) window inside a buffer whose every other word is a quiet-NaN
bit pattern.  After each call
  * the status is TNET_OK,
  * every output and in-place operand has its whole frame intact (assert_frame_untouched: guard rows, the band before
    column 0, the column padding, compared as uint32) and no NaN in its interior -- outputs start as poison, so every
    element must have been written, and a value read from outside a matrix shows wherever it reaches a stored result,
  * every pure input's buffer is bit-identical to what was uploaded (assert_unchanged),
  * the interior meets the bound of the entry point's existing test (tests/test_gpu_kernels.py docstring):
      GEMM-shaped results  |got - ref| <= 2e-5 * (|A||B|)_ij + 1e-6 against an fp64 product
      sigmoid / diff-sigmoid / slab-sum / SGD forms: as test_affine_fwd, test_affine_bwd_dsig,
      test_affine_bwd_colsum, test_colsum_slab_sums, test_affine_update*
      exact ops bit for bit; add_scaled / sgd rtol 1e-6 atol 1e-6; log rtol 2e-6; softmax rtol 2e-5; statistics
      rtol 1e-5.
Frame.done() below is where those checks are made for every call of this module.

Shapes of part A (the smallest at which each GEMM path can still go wrong), as (M, N, K) for tnet_sgemm and as
(rows, n_in, n_out) for the affine family:
  (33, 65, 31)     no full k-tile, every dimension off 4
  (70, 135, 150)   two full 64-deep k-tiles and a tail with K % 4 == 2, N % 4 == 3, M off 32
  (130, 72, 192)   whole k-tiles in an odd count, N % 4 == 0 (direct forms eligible), M % 4 != 0
  (128, 256, 128)  px_exact()'s M % BM == 0 && N % BN == 0 holds for the 64x128 forward (M = rows, N = n_out), the
                   64x128 backward (M = rows, N = n_in) and the 128x128 update (M = n_in, N = n_out): the
                   exact-prefetch and direct forms run (the bias-slab epilogues' extra condition, at least 16 tile
                   rows, needs n_in >= 2048 and is covered at full size by tests/test_gpu_kernels.py)
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as orc  # noqa: E402
from kernel_views import POISON_INPUT, PoisonView, assert_frame_untouched, assert_unchanged  # noqa: E402
from test_gpu_kernels import GEMM_CFGS, gemm_ref, rnd, slab_sums  # noqa: E402
from tnet_amd import DeviceArray  # noqa: E402
from tnet_amd._lib import MatrixDim, check, lib  # noqa: E402

TNET_OK, TNET_ERR_ARG = 0, -1  # include/tnet_kernels.h
FLT_MIN = np.float32(1.1754944e-38)
U = 2.0 ** -24  # fp32 unit roundoff

VIEW_SHAPES = [(33, 65, 31), (70, 135, 150), (130, 72, 192), (128, 256, 128)]
GEMM_LAYOUTS = ["tight", "offset"]
ALL_LAYOUTS = ["tight", "offset", "odd"]
# one configuration per kernel family: the planner, the 32x32 glds kernel, the 16x16 ring, the direct forms (the ring
# where not exact), split-K + combine4 -- and the two ring / direct configurations whose tiles px_exact() needs at
# (128, 256, 128): the 64x128 forward / backward and the 128x128 update
AFFINE_CFGS = ["auto", "g64x64k32s4w4", "m64x64k32s4w41", "m64x64a4", "m64x128c8", "m64x64k32s4w41+sk2",
               "m64x128k64s2", "m128x128a4"]


def S():
    return lib().tnet_stream()


def _cfg_fixture(names):
    @pytest.fixture(params=names)
    def fx(request):
        check(lib().tnet_gemm_config(request.param.encode()))
        yield request.param
        check(lib().tnet_gemm_config(b"auto"))
    return fx


gemm_cfg = _cfg_fixture(GEMM_CFGS)
affine_cfg = _cfg_fixture(AFFINE_CFGS)


class Frame:
    """the operands of one call: inputs (must stay bit-identical), outputs (interior poison before the call) and
    in-place operands (real interior, poison around)"""

    def __init__(self, layout, what):
        self.layout, self.what = layout, what
        self.ins, self.outs = [], []

    def inp(self, a, layout=None):
        # (a pure input's frame holds another NaN payload than an output's: a copy of one into the other shows)
        v = PoisonView(a, layout or self.layout, poison=POISON_INPUT)
        self.ins.append(v)
        return v

    def out(self, rows, cols, layout=None, dtype=np.float32):
        v = PoisonView.empty(rows, cols, layout or self.layout, dtype)
        self.outs.append(v)
        return v

    def io(self, a, layout=None):
        v = PoisonView(a, layout or self.layout)
        self.outs.append(v)
        return v

    def done(self, status):
        """status OK; every output / in-place operand: frame untouched, interior without NaN; every pure input
        unchanged.  Returns the outputs' interiors in the order they were declared."""
        assert status == TNET_OK, f"{self.what}: status {status}"
        got = []
        for k, v in enumerate(self.outs):
            raw = v.raw()
            assert_frame_untouched(v, f"{self.what}: output {k}", raw=raw)
            a = raw[v._index].view(v.dtype).reshape(v.rows, v.cols)
            if v.dtype == np.float32:
                assert not np.isnan(a).any(), \
                    f"{self.what}: output {k}: {int(np.isnan(a).sum())} NaN, first at {np.argwhere(np.isnan(a))[0]}"
            got.append(a)
        for k, v in enumerate(self.ins):
            assert_unchanged(v, v.initial, f"{self.what}: input {k}")
        return got

    def rejected(self, status):
        """TNET_ERR_ARG and nothing launched: every operand's buffer bit-identical"""
        assert status == TNET_ERR_ARG, f"{self.what}: status {status}, expected TNET_ERR_ARG"
        for k, v in enumerate(self.ins + self.outs):
            assert_unchanged(v, v.initial, f"{self.what}: operand {k}")


def within(got, ref, tol, what):
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} element(s) off, worst {err[bad].max():.3e} at " \
                          f"{np.argwhere(bad)[0]} (tolerance there {np.broadcast_to(tol, err.shape)[bad][0]:.3e})"


# ------------------------------------------------------------------------------------------------------------------
# Part A: the GEMM family
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sgemm_case(M, N, K, ta, tb):
    A = rnd((K, M) if ta == "T" else (M, K), 1)
    B = rnd((N, K) if tb == "T" else (K, N), 2)
    C0 = rnd((M, N), 3)
    ref, mag = gemm_ref(ta, tb, A, B)
    for a in (A, B, C0, ref, mag):
        a.setflags(write=False)
    return A, B, C0, ref, mag


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("M,N,K", VIEW_SHAPES)
def test_sgemm_views(M, N, K, layout, gemm_cfg):
    """all four transposes, alpha 0.75, beta 0 (C starts as poison and must come out finite: beta == 0 reads no C)
    and beta 0.5 (C in place)"""
    alpha = 0.75
    for ta, tb in (("N", "N"), ("N", "T"), ("T", "N"), ("T", "T")):
        A, B, C0, ref, mag = sgemm_case(M, N, K, ta, tb)
        for beta in (0.0, 0.5):
            f = Frame(layout, f"sgemm {ta}{tb} beta {beta}")
            vA, vB = f.inp(A), f.inp(B)
            vC = f.io(C0) if beta else f.out(M, N)
            st = lib().tnet_sgemm(ta.encode(), tb.encode(), M, N, K, alpha, vA.ptr, vA.stride, vB.ptr, vB.stride, beta,
                                  vC.ptr, vC.stride, S())
            got, = f.done(st)
            within(got, alpha * ref + beta * C0, 2e-5 * (alpha * mag + np.abs(beta * C0)) + 1e-6, f.what)


@functools.lru_cache(maxsize=None)
def affine_case(rows, n_in, n_out):
    d = dict(X=rnd((rows, n_in), 6), W=rnd((n_in, n_out), 7, 0.1), b=rnd(n_out, 8), b_in=rnd(n_in, 108),
             E=rnd((rows, n_out), 9), Es=rnd((rows, n_out), 13, 0.01),
             Yb=(1 / (1 + np.exp(-rnd((rows, n_in), 11)))).astype(np.float32),
             corr=rnd((n_in, n_out), 15, 0.01), corr_b=rnd(n_out, 19, 0.01))
    d["P"] = slab_sums(d["Es"]).astype(np.float32)
    for a in d.values():
        a.setflags(write=False)
    return d


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", VIEW_SHAPES)
def test_affine_fwd_views(rows, n_in, n_out, layout, affine_cfg):
    d = affine_case(rows, n_in, n_out)
    z, mag = gemm_ref("N", "N", d["X"], d["W"])
    z = z + d["b"]
    sig = 1.0 / (1.0 + np.exp(-z))
    for act in (0, 1, 2, 3):
        f = Frame(layout, f"affine_fwd act {act}")
        vX, vW, vb = f.inp(d["X"]), f.inp(d["W"]), f.inp(d["b"])
        vY = f.out(rows, n_out)
        st = lib().tnet_affine_fwd(vX.ptr, vX.dim, vW.ptr, vW.dim, vb.ptr, vY.ptr, vY.dim, act, S())
        got, = f.done(st)
        if act in (1, 3):  # test_affine_fwd's sigmoid bound; act 3 stores the negated sigmoid
            within(got, sig if act == 1 else -sig, 2e-5 * mag * sig * (1 - sig) + 2e-6, f.what)
        else:
            within(got, z if act == 0 else -z, 2e-5 * mag + 1e-6, f.what)


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", VIEW_SHAPES)
def test_affine_fwd_t_views(rows, n_in, n_out, layout, affine_cfg):
    """Y [rows x n_in] = act(X [rows x n_out] W^T + b [n_in]) (the RBM reconstruction)"""
    d = affine_case(rows, n_in, n_out)
    z, mag = gemm_ref("N", "T", d["E"], d["W"])
    z = z + d["b_in"]
    sig = 1.0 / (1.0 + np.exp(-z))
    for act in (0, 1):
        f = Frame(layout, f"affine_fwd_t act {act}")
        vX, vW, vb = f.inp(d["E"]), f.inp(d["W"]), f.inp(d["b_in"])
        vY = f.out(rows, n_in)
        st = lib().tnet_affine_fwd_t(vX.ptr, vX.dim, vW.ptr, vW.dim, vb.ptr, vY.ptr, vY.dim, act, S())
        got, = f.done(st)
        if act:
            within(got, sig, 2e-5 * mag * sig * (1 - sig) + 2e-6, f.what)
        else:
            within(got, z, 2e-5 * mag + 1e-6, f.what)


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", VIEW_SHAPES)
def test_affine_bwd_views(rows, n_in, n_out, layout, affine_cfg):
    d = affine_case(rows, n_in, n_out)
    z, mag = gemm_ref("N", "T", d["E"], d["W"])
    s = d["Yb"].astype(np.float64) * (1 - d["Yb"])
    for dsig in (0, 1):
        f = Frame(layout, f"affine_bwd dsig {dsig}")
        vE, vW, vY = f.inp(d["E"]), f.inp(d["W"]), f.inp(d["Yb"])
        vO = f.out(rows, n_in)
        st = lib().tnet_affine_bwd(vE.ptr, vE.dim, vW.ptr, vW.dim, vY.ptr, vY.stride, vO.ptr, vO.dim, dsig, S())
        got, = f.done(st)
        if dsig:
            within(got, z * s, 2e-5 * mag * s + 1e-7, f.what)  # test_affine_bwd_dsig
        else:
            within(got, z, 2e-5 * mag + 1e-6, f.what)


def check_bwd_colsum(d, got, P, what):
    """test_affine_bwd_colsum's bounds: Eo against the fp64 product, the slab sums against it and against the fp32
    sums of the kernel's own outputs"""
    z, mag = gemm_ref("N", "T", d["E"], d["W"])
    s = d["Yb"].astype(np.float64) * (1 - d["Yb"])
    within(got, z * s, 2e-5 * mag * s + 1e-7, what + " Eo")
    within(P, slab_sums(z * s), slab_sums(2e-5 * mag * s + 1e-7) + 32 * 6e-8 * slab_sums(np.abs(got)), what + " slabs")
    within(P, slab_sums(got), 32 * 1.2e-7 * slab_sums(np.abs(got)) + 1e-7, what + " slabs of its own Eo")


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", VIEW_SHAPES)
def test_affine_bwd_colsum_views(rows, n_in, n_out, layout, affine_cfg):
    """the slab sums are where a clamped or past-the-edge row would leak: the last slab of 33, 70 and 130 rows is
    partial, and the rows below it are poison"""
    d = affine_case(rows, n_in, n_out)
    slabs = lib().tnet_colsum_slabs(rows)
    assert slabs == -(-rows // 32)
    f = Frame(layout, "affine_bwd_colsum")
    vE, vW, vY = f.inp(d["E"]), f.inp(d["W"]), f.inp(d["Yb"])
    vO, vP = f.out(rows, n_in), f.out(slabs, n_in)
    st = lib().tnet_affine_bwd_colsum(vE.ptr, vE.dim, vW.ptr, vW.dim, vY.ptr, vY.stride, vO.ptr, vO.dim, vP.ptr,
                                      vP.stride, S())
    got, P = f.done(st)
    check_bwd_colsum(d, got, P, f.what)


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("rows,cols", [(33, 65), (70, 135), (130, 72), (128, 256), (64, 64), (1, 129)])
def test_transpose_views(rows, cols, layout):
    """tnet_transpose (any stride): T = A^T bit for bit, T's frame untouched"""
    A = rnd((rows, cols), 70)
    f = Frame(layout, "transpose")
    vA, vT = f.inp(A), f.out(cols, rows)
    got, = f.done(lib().tnet_transpose(vA.ptr, vA.dim, vT.ptr, vT.stride, S()))
    np.testing.assert_array_equal(got.view(np.uint32), np.ascontiguousarray(A.T).view(np.uint32))


def check_bwd_colsum_both_forms(rows, n_in, n_out, layout):
    """Wt = tnet_transpose(W) on views (exact), then tnet_affine_bwd_colsum_t from Wt and tnet_affine_bwd_colsum from
    W: each within test_affine_bwd_colsum's bounds, Eo bit-identical between the two (the header's promise)"""
    d = affine_case(rows, n_in, n_out)
    slabs = lib().tnet_colsum_slabs(rows)
    ft = Frame(layout, "transpose of W")
    vW = ft.inp(d["W"])
    vWt = ft.out(n_out, n_in)
    Wt, = ft.done(lib().tnet_transpose(vW.ptr, vW.dim, vWt.ptr, vWt.stride, S()))
    np.testing.assert_array_equal(Wt, d["W"].T)
    res = []
    for form in ("t", "w"):
        f = Frame(layout, f"affine_bwd_colsum ({form})")
        vE, vY = f.inp(d["E"]), f.inp(d["Yb"])
        vB = f.inp(Wt) if form == "t" else f.inp(d["W"])
        vO, vP = f.out(rows, n_in), f.out(slabs, n_in)
        fn = lib().tnet_affine_bwd_colsum_t if form == "t" else lib().tnet_affine_bwd_colsum
        st = fn(vE.ptr, vE.dim, vB.ptr, vB.dim, vY.ptr, vY.stride, vO.ptr, vO.dim, vP.ptr, vP.stride, S())
        got, P = f.done(st)
        check_bwd_colsum(d, got, P, f.what)
        res.append(got)
    np.testing.assert_array_equal(res[0].view(np.uint32), res[1].view(np.uint32))


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", VIEW_SHAPES)
def test_affine_bwd_colsum_t_views(rows, n_in, n_out, layout):
    """the backward from the transposed shadow, on views.  The planner's configuration only: a forced one makes the
    _t form decline (gemm_f32.hip launch_colsum_bwd_t)."""
    check_bwd_colsum_both_forms(rows, n_in, n_out, layout)


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", [(1000, 1664, 130), (1024, 1664, 128)])
def test_affine_bwd_colsum_views_one_tile_per_cu(rows, n_in, n_out, layout):
    """the planner's own choice for the training step's backward: at 200 or more 64x128 tiles (16 x 13 here) it runs
    the 64x128 kernel in its direct forms (m64x128c8 from W, m64x128a8 from the transposed shadow) -- which no
    forced configuration reaches, launch_colsum_bwd maps those to the 64x64 ring -- with the slab sums fused.
    1000 rows: the M edge clamps inside the last tile and a partial last slab next to poisoned rows, and a k tail
    of 2; 1024 x 1664 x 128: px_exact() holds, the exact-prefetch instantiation"""
    check_bwd_colsum_both_forms(rows, n_in, n_out, layout)


def sgd_ref(d, mmt, scale, l2):
    g, mag = gemm_ref("T", "N", d["X"], d["Es"])
    c = g + mmt * d["corr"]
    w = d["W"] + scale * c
    w = w + l2 * w
    return c, w, mag


UPDATE_VARIANTS = [(0.0, False, -1e-4), (0.5, True, 0.0), (0.5, True, -1e-4), (0.0, True, 0.0)]


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", VIEW_SHAPES)
def test_affine_update_views(rows, n_in, n_out, layout, affine_cfg):
    """mmt 0 with corrW = NULL, mmt 0.5, l2 != 0, and mmt 0 with a momentum buffer (written with the raw gradient);
    bounds of test_affine_update"""
    d = affine_case(rows, n_in, n_out)
    scale = -0.3 / rows
    for mmt, with_corr, l2 in UPDATE_VARIANTS:
        f = Frame(layout, f"affine_update mmt {mmt} corr {with_corr} l2 {l2}")
        vX, vE = f.inp(d["X"]), f.inp(d["Es"])
        vW = f.io(d["W"])
        vC = f.io(d["corr"]) if with_corr else None
        st = lib().tnet_affine_update(vX.ptr, vX.dim, vE.ptr, vE.dim, vW.ptr, vW.dim, vC.ptr if vC else None,
                                      vC.stride if vC else 0, scale, mmt, l2, S())
        got = f.done(st)
        c, w, mag = sgd_ref(d, mmt, scale, l2)
        within(got[0], w, 2e-5 * abs(scale) * mag + 2e-7 * np.abs(d["W"]) + 1e-7, f.what + " W")
        if with_corr:
            within(got[1], c, 2e-5 * mag + 1e-6, f.what + " corrW")


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", VIEW_SHAPES)
def test_affine_update_bias_views(rows, n_in, n_out, layout, affine_cfg):
    """weight SGD + bias SGD from the slab sums (colpart, b, corr_b on views too); bounds of test_affine_update_bias"""
    d = affine_case(rows, n_in, n_out)
    scale, l2 = -0.3 / rows, -1e-4
    for mmt in (0.0, 0.5):
        f = Frame(layout, f"affine_update_bias mmt {mmt}")
        vX, vE, vP = f.inp(d["X"]), f.inp(d["Es"]), f.inp(d["P"])
        vW, vb = f.io(d["W"]), f.io(d["b"])
        vC, vCb = (f.io(d["corr"]), f.io(d["corr_b"])) if mmt else (None, None)
        st = lib().tnet_affine_update_bias(vX.ptr, vX.dim, vE.ptr, vE.dim, vW.ptr, vW.dim, vC.ptr if vC else None,
                                           vC.stride if vC else 0, scale, mmt, l2, vP.ptr, vP.stride, vb.ptr,
                                           vCb.ptr if vCb else None, S())
        got = f.done(st)
        c, w, mag = sgd_ref(d, mmt, scale, l2)
        within(got[0], w, 2e-5 * abs(scale) * mag + 2e-7 * np.abs(d["W"]) + 1e-7, f.what + " W")
        gb = d["P"].astype(np.float64).sum(0).astype(np.float32).astype(np.float64)
        cb = gb + mmt * d["corr_b"]
        np.testing.assert_allclose(got[1].ravel(), d["b"] + scale * cb, rtol=1e-6, atol=1e-7, err_msg=f.what)
        if mmt:
            within(got[2], c, 2e-5 * mag + 1e-6, f.what + " corrW")
            np.testing.assert_allclose(got[3].ravel(), cb, rtol=1e-6, atol=1e-9, err_msg=f.what)


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", [(1000, 130, 1664), (1024, 128, 1664)])
def test_affine_fwd_views_one_tile_per_cu(rows, n_in, n_out, layout):
    """the planner's own choice for the step's hidden forward: 208 tiles of 64x128 run m64x128a4, the direct form
    (1024 rows: px_exact() holds; 1000 rows and K = 130: the M edge clamps and a k tail of 2)"""
    d = affine_case(rows, n_in, n_out)
    z, mag = gemm_ref("N", "N", d["X"], d["W"])
    sig = 1.0 / (1.0 + np.exp(-(z + d["b"])))
    f = Frame(layout, "affine_fwd act 1")
    vX, vW, vb = f.inp(d["X"]), f.inp(d["W"]), f.inp(d["b"])
    vY = f.out(rows, n_out)
    got, = f.done(lib().tnet_affine_fwd(vX.ptr, vX.dim, vW.ptr, vW.dim, vb.ptr, vY.ptr, vY.dim, 1, S()))
    within(got, sig, 2e-5 * mag * sig * (1 - sig) + 2e-6, f.what)


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", [(130, 2040, 1924), (128, 2048, 1920)])
def test_affine_update_bias_views_one_tile_per_cu(rows, n_in, n_out, layout):
    """the planner's own choice for the step's update: 240 or more 128x128 tiles run m128x128a4, the direct form,
    with the bias SGD in the prologue (2048 x 1920: px_exact() holds including the bias-slab condition of 16 tile
    rows; 2040 x 1924 over K = 130: both edges clamp, a k tail of 2)"""
    d = affine_case(rows, n_in, n_out)
    scale, l2, mmt = -0.3 / rows, -1e-4, 0.5
    f = Frame(layout, "affine_update_bias")
    vX, vE, vP = f.inp(d["X"]), f.inp(d["Es"]), f.inp(d["P"])
    vW, vb, vC, vCb = f.io(d["W"]), f.io(d["b"]), f.io(d["corr"]), f.io(d["corr_b"])
    st = lib().tnet_affine_update_bias(vX.ptr, vX.dim, vE.ptr, vE.dim, vW.ptr, vW.dim, vC.ptr, vC.stride, scale, mmt, l2,
                                       vP.ptr, vP.stride, vb.ptr, vCb.ptr, S())
    W, b, corr, corr_b = f.done(st)
    c, w, mag = sgd_ref(d, mmt, scale, l2)
    within(W, w, 2e-5 * abs(scale) * mag + 2e-7 * np.abs(d["W"]) + 1e-7, f.what + " W")
    within(corr, c, 2e-5 * mag + 1e-6, f.what + " corrW")
    cb = d["P"].astype(np.float64).sum(0).astype(np.float32).astype(np.float64) + mmt * d["corr_b"]
    np.testing.assert_allclose(b.ravel(), d["b"] + scale * cb, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(corr_b.ravel(), cb, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", VIEW_SHAPES)
def test_affine_grad_views(rows, n_in, n_out, layout, affine_cfg):
    """G = X^T E into a poisoned buffer, alone and with gradB from the slab sums (test_affine_grad_bias's bounds)"""
    d = affine_case(rows, n_in, n_out)
    g, mag = gemm_ref("T", "N", d["X"], d["Es"])
    f = Frame(layout, "affine_grad")
    vX, vE = f.inp(d["X"]), f.inp(d["Es"])
    vG = f.out(n_in, n_out)
    got, = f.done(lib().tnet_affine_grad(vX.ptr, vX.dim, vE.ptr, vE.dim, vG.ptr, vG.dim, S()))
    within(got, g, 2e-5 * mag + 1e-7, f.what)
    f = Frame(layout, "affine_grad_bias")
    vX, vE, vP = f.inp(d["X"]), f.inp(d["Es"]), f.inp(d["P"])
    vG, vgb = f.out(n_in, n_out), f.out(1, n_out)
    got, gb = f.done(lib().tnet_affine_grad_bias(vX.ptr, vX.dim, vE.ptr, vE.dim, vG.ptr, vG.dim, vP.ptr, vP.stride,
                                                 vgb.ptr, S()))
    within(got, g, 2e-5 * mag + 1e-7, f.what)
    np.testing.assert_array_equal(gb.ravel(), d["P"].astype(np.float64).sum(0).astype(np.float32))


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", VIEW_SHAPES)
def test_rbm_update_views(rows, n_in, n_out, layout, affine_cfg):
    """corr = mmt*corr + scale*(V^T H) + l2*W ; W += corr.  Bound: test_affine_update's GEMM term, plus one fp32
    rounding for each of the three sums of corr (3 U of the terms' magnitudes) and, for W, of W + corr (2e-7 |W|)"""
    d = affine_case(rows, n_in, n_out)
    scale, mmt, l2 = 0.1 / rows, 0.5, -2e-4
    f = Frame(layout, "rbm_update")
    vV, vH = f.inp(d["X"]), f.inp(d["E"])
    vW, vC = f.io(d["W"]), f.io(d["corr"])
    st = lib().tnet_rbm_update(vV.ptr, vV.dim, vH.ptr, vH.dim, vW.ptr, vW.dim, vC.ptr, vC.stride, scale, mmt, l2, S())
    W, corr = f.done(st)
    g, mag = gemm_ref("T", "N", d["X"], d["E"])
    c = mmt * d["corr"] + scale * g + l2 * d["W"]
    terms = np.abs(mmt * d["corr"]) + np.abs(scale * g) + np.abs(l2 * d["W"])
    tol = 2e-5 * abs(scale) * mag + 3 * U * terms + 1e-9
    within(corr, c, tol, f.what + " corrW")
    within(W, d["W"] + c, tol + 2e-7 * np.abs(d["W"]) + 1e-7, f.what + " W")


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("rows,n_in,n_out", VIEW_SHAPES)
def test_colsum_slab_sums_views(rows, n_in, n_out, layout):
    """E [rows x n_out]; test_colsum_slab_sums's contract: tnet_colsum_slabs(rows) disjoint row ranges whose sum is
    the column sum, 32 rows each where rows % 32 == 0 (`odd` takes the scalar form)"""
    E = affine_case(rows, n_in, n_out)["E"]
    slabs = lib().tnet_colsum_slabs(rows)
    f = Frame(layout, "colsum_slab_sums")
    vE, vP = f.inp(E), f.out(slabs, n_out)
    P, = f.done(lib().tnet_colsum_slab_sums(vE.ptr, vE.dim, vP.ptr, vP.stride, S()))
    tot = np.abs(E).astype(np.float64).sum(0)
    within(P.astype(np.float64).sum(0), E.astype(np.float64).sum(0), 32 * 1.2e-7 * tot + 1e-7, f.what)
    if rows % 32 == 0:
        within(P, slab_sums(E), 32 * 1.2e-7 * slab_sums(np.abs(E)) + 1e-7, f.what)


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("n_out", [7, 135, 256])
@pytest.mark.parametrize("rows,n_in", [(37, 70), (64, 512)])
def test_affine_softmax_xent_views(rows, n_in, n_out, layout, affine_cfg):
    """the fused top layer with Z, Y, E and colpart all on views (64 x 512 is a shape the K-slice kernel of
    top_rows.hip takes under "auto" where W's stride allows it); bounds of test_affine_softmax_xent"""
    X, W, b = rnd((rows, n_in), 60), rnd((n_in, n_out), 61, 0.1), rnd(n_out, 62)
    lab = np.random.default_rng(63).integers(0, n_out, size=rows).astype(np.int32)
    lab[::7] = -1
    lab[3::11] = n_out - 1
    slabs = lib().tnet_colsum_slabs(rows)
    f = Frame(layout, "affine_softmax_xent")
    vX, vW, vb, vL = f.inp(X), f.inp(W), f.inp(b), f.inp(lab)
    vZ, vY, vE, vP = f.out(rows, n_out), f.out(rows, n_out), f.out(rows, n_out), f.out(slabs, n_out)
    stats = DeviceArray(1, 1024, np.float64, stride=1024)
    st = lib().tnet_affine_softmax_xent(vX.ptr, vX.dim, vW.ptr, vW.dim, vb.ptr, vL.ptr, vZ.ptr, vZ.stride, vY.ptr,
                                        vY.stride, vE.ptr, vE.stride, stats.ptr, vP.ptr, vP.stride, S())
    Z, Y, E, P = f.done(st)
    z, mag = gemm_ref("N", "N", X, W)
    within(Z, z + b, 2e-5 * mag + 1e-6, f.what + " Z")
    Yref = orc.softmax(Z)
    Eref, xent, correct = orc.xent_eval(Yref, lab)
    np.testing.assert_allclose(Y, Yref, rtol=2e-5, atol=1e-9)
    np.testing.assert_allclose(E, Eref, rtol=2e-5, atol=1e-7)
    s = stats.numpy()[0]
    np.testing.assert_allclose(s[0::2].sum(), xent, rtol=1e-5, atol=1e-5)
    assert int(round(s[1::2].sum())) == correct
    within(P, slab_sums(E), 32 * 1.2e-7 * slab_sums(np.abs(E)) + 1e-7, f.what + " slabs")


@pytest.mark.parametrize("rows,n_in,n_out", [(33, 65, 31), (128, 256, 128)])
def test_affine_side_operands_on_odd_views(rows, n_in, n_out, affine_cfg):
    """what the GEMM family does not ask to be 16-B aligned, on `odd` views (a 4-B aligned base, any stride): the
    bias of the forward, the slab-sum rows written by the backward and read by the update / gradient, b, corr_b and
    gradB, and Z, Y, E and colpart of the fused top layer.  The GEMM matrices stay on `offset`."""
    d = affine_case(rows, n_in, n_out)
    L = lib()
    f = Frame("offset", "affine_fwd, bias odd")
    vX, vW, vb, vY = f.inp(d["X"]), f.inp(d["W"]), f.inp(d["b"], "odd"), f.out(rows, n_out)
    got, = f.done(L.tnet_affine_fwd(vX.ptr, vX.dim, vW.ptr, vW.dim, vb.ptr, vY.ptr, vY.dim, 1, S()))
    z, mag = gemm_ref("N", "N", d["X"], d["W"])
    sig = 1.0 / (1.0 + np.exp(-(z + d["b"])))
    within(got, sig, 2e-5 * mag * sig * (1 - sig) + 2e-6, f.what)

    slabs = L.tnet_colsum_slabs(rows)
    f = Frame("offset", "affine_bwd_colsum, colpart odd")
    vE, vW, vYb = f.inp(d["E"]), f.inp(d["W"]), f.inp(d["Yb"])
    vO, vP = f.out(rows, n_in), f.out(slabs, n_in, "odd")
    got, P = f.done(L.tnet_affine_bwd_colsum(vE.ptr, vE.dim, vW.ptr, vW.dim, vYb.ptr, vYb.stride, vO.ptr, vO.dim,
                                             vP.ptr, vP.stride, S()))
    check_bwd_colsum(d, got, P, f.what)

    scale, l2, mmt = -0.3 / rows, -1e-4, 0.5
    f = Frame("offset", "affine_update_bias, colpart / b / corr_b odd")
    vX, vE, vP = f.inp(d["X"]), f.inp(d["Es"]), f.inp(d["P"], "odd")
    vW, vC, vb, vCb = f.io(d["W"]), f.io(d["corr"]), f.io(d["b"], "odd"), f.io(d["corr_b"], "odd")
    W, corr, b, corr_b = f.done(L.tnet_affine_update_bias(vX.ptr, vX.dim, vE.ptr, vE.dim, vW.ptr, vW.dim, vC.ptr,
                                                          vC.stride, scale, mmt, l2, vP.ptr, vP.stride, vb.ptr, vCb.ptr,
                                                          S()))
    c, w, mag = sgd_ref(d, mmt, scale, l2)
    within(W, w, 2e-5 * abs(scale) * mag + 2e-7 * np.abs(d["W"]) + 1e-7, f.what + " W")
    within(corr, c, 2e-5 * mag + 1e-6, f.what + " corrW")
    gb = d["P"].astype(np.float64).sum(0).astype(np.float32)
    cb = gb.astype(np.float64) + mmt * d["corr_b"]
    np.testing.assert_allclose(b.ravel(), d["b"] + scale * cb, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(corr_b.ravel(), cb, rtol=1e-6, atol=1e-9)

    f = Frame("offset", "affine_grad_bias, colpart / gradB odd")
    vX, vE, vP = f.inp(d["X"]), f.inp(d["Es"]), f.inp(d["P"], "odd")
    vG, vgb = f.out(n_in, n_out), f.out(1, n_out, "odd")
    G, gradB = f.done(L.tnet_affine_grad_bias(vX.ptr, vX.dim, vE.ptr, vE.dim, vG.ptr, vG.dim, vP.ptr, vP.stride,
                                              vgb.ptr, S()))
    g, mag = gemm_ref("T", "N", d["X"], d["Es"])
    within(G, g, 2e-5 * mag + 1e-7, f.what)
    np.testing.assert_array_equal(gradB.ravel(), gb)

    lab = np.random.default_rng(63).integers(0, n_out, size=rows).astype(np.int32)
    lab[::7] = -1
    f = Frame("offset", "affine_softmax_xent, Z / Y / E / colpart odd")
    vX, vW, vb, vL = f.inp(d["X"]), f.inp(d["W"]), f.inp(d["b"], "odd"), f.inp(lab, "odd")
    vZ, vY, vE = f.out(rows, n_out, "odd"), f.out(rows, n_out, "odd"), f.out(rows, n_out, "odd")
    vP = f.out(slabs, n_out, "odd")
    stats = DeviceArray(1, 1024, np.float64, stride=1024)
    Z, Y, E, P = f.done(L.tnet_affine_softmax_xent(vX.ptr, vX.dim, vW.ptr, vW.dim, vb.ptr, vL.ptr, vZ.ptr, vZ.stride,
                                                   vY.ptr, vY.stride, vE.ptr, vE.stride, stats.ptr, vP.ptr, vP.stride,
                                                   S()))
    z, mag = gemm_ref("N", "N", d["X"], d["W"])
    within(Z, z + d["b"], 2e-5 * mag + 1e-6, f.what + " Z")
    Yref = orc.softmax(Z)
    Eref, xent, correct = orc.xent_eval(Yref, lab)
    np.testing.assert_allclose(Y, Yref, rtol=2e-5, atol=1e-9)
    np.testing.assert_allclose(E, Eref, rtol=2e-5, atol=1e-7)
    st = stats.numpy()[0]
    np.testing.assert_allclose(st[0::2].sum(), xent, rtol=1e-5, atol=1e-5)
    assert int(round(st[1::2].sum())) == correct
    within(P, slab_sums(E), 32 * 1.2e-7 * slab_sums(np.abs(E)) + 1e-7, f.what + " slabs")


# ---- rejection: a base one float off 16-B alignment, a stride that is no multiple of 4 -> TNET_ERR_ARG, nothing run
def _reject_calls():
    """name -> (operands to perturb ("K:stride": its stride only), call(P, D, ST)); P / D / ST give an operand's pointer / MatrixDim / stride with
    the test's perturbation applied.  rows 16, n_in 24, n_out 32 in the `offset` layout: even a perturbed view lies
    inside its backing buffer (one float, or 2 floats a row over 16 rows, against 3 guard rows of >= 36)"""
    L = lib()
    r, ni, no = 16, 24, 32
    mats = dict(X=(r, ni), W=(ni, no), E=(r, no), Yb=(r, ni), Eo=(r, ni), Y=(r, no), Yt=(r, ni), C=(ni, no),
                P=(1, no), Pi=(1, ni), Wt=(no, ni), Xt=(r, no))
    vecs = dict(b=no, bi=ni, cb=no, gb=no)
    calls = {
        "sgemm": (("X", "W", "Y"), lambda P, D, ST: L.tnet_sgemm(b"N", b"N", r, no, ni, 1.0, P("X"), ST("X"), P("W"),
                                                                  ST("W"), 0.0, P("Y"), ST("Y"), S())),
        "affine_fwd": (("X", "W", "Y"), lambda P, D, ST: L.tnet_affine_fwd(P("X"), D("X"), P("W"), D("W"), P("b"), P("Y"),
                                                                           D("Y"), 1, S())),
        "affine_fwd_t": (("Xt", "W", "Yt"), lambda P, D, ST: L.tnet_affine_fwd_t(P("Xt"), D("Xt"), P("W"), D("W"), P("bi"),
                                                                                 P("Yt"), D("Yt"), 1, S())),
        "affine_bwd": (("E", "W", "Eo", "Yb"), lambda P, D, ST: L.tnet_affine_bwd(P("E"), D("E"), P("W"), D("W"), P("Yb"),
                                                                                  ST("Yb"), P("Eo"), D("Eo"), 1, S())),
        "affine_bwd_colsum": (("E", "W", "Eo", "Yb"), lambda P, D, ST: L.tnet_affine_bwd_colsum(
            P("E"), D("E"), P("W"), D("W"), P("Yb"), ST("Yb"), P("Eo"), D("Eo"), P("Pi"), ST("Pi"), S())),
        "affine_bwd_colsum_t": (("E", "Wt", "Eo", "Yb"), lambda P, D, ST: L.tnet_affine_bwd_colsum_t(
            P("E"), D("E"), P("Wt"), D("Wt"), P("Yb"), ST("Yb"), P("Eo"), D("Eo"), P("Pi"), ST("Pi"), S())),
        "affine_update": (("X", "E", "W", "C:stride"), lambda P, D, ST: L.tnet_affine_update(
            P("X"), D("X"), P("E"), D("E"), P("W"), D("W"), P("C"), ST("C"), -0.01, 0.5, 0.0, S())),
        "affine_update_bias": (("X", "E", "W", "C:stride"), lambda P, D, ST: L.tnet_affine_update_bias(
            P("X"), D("X"), P("E"), D("E"), P("W"), D("W"), P("C"), ST("C"), -0.01, 0.5, 0.0, P("P"), ST("P"), P("b"),
            P("cb"), S())),
        "affine_grad": (("X", "E", "C"), lambda P, D, ST: L.tnet_affine_grad(P("X"), D("X"), P("E"), D("E"), P("C"),
                                                                             D("C"), S())),
        "affine_grad_bias": (("X", "E", "C"), lambda P, D, ST: L.tnet_affine_grad_bias(
            P("X"), D("X"), P("E"), D("E"), P("C"), D("C"), P("P"), ST("P"), P("gb"), S())),
        "rbm_update": (("X", "E", "W", "C:stride"), lambda P, D, ST: L.tnet_rbm_update(
            P("X"), D("X"), P("E"), D("E"), P("W"), D("W"), P("C"), ST("C"), 0.01, 0.5, 0.0, S())),
        "affine_softmax_xent": (("X", "W"), lambda P, D, ST: L.tnet_affine_softmax_xent(
            P("X"), D("X"), P("W"), D("W"), P("b"), P("lab"), P("Y"), ST("Y"), None, 0, P("E"), ST("E"), None, P("P"),
            ST("P"), S())),
    }
    return mats, vecs, calls


REJECT_NAMES = ["sgemm", "affine_fwd", "affine_fwd_t", "affine_bwd", "affine_bwd_colsum", "affine_bwd_colsum_t",
                "affine_update", "affine_update_bias", "affine_grad", "affine_grad_bias", "rbm_update",
                "affine_softmax_xent"]


@pytest.mark.parametrize("name", REJECT_NAMES)
def test_gemm_family_rejects_misaligned_views(name):
    """each 16-B / multiple-of-4 operand of each entry point, perturbed one at a time: TNET_ERR_ARG before any launch
    (every operand's whole buffer bit-identical afterwards).  These are the operands the entry points check: the
    three GEMM matrices, Ybelow, and the momentum matrix's stride.  The side operands -- bias and momentum vectors,
    slab-sum rows, Z / Y / E of the fused top layer -- are taken at any 4-B alignment and any stride
    (test_affine_side_operands_on_odd_views runs them so); tnet_colsum_slab_sums takes any stride too
    (test_colsum_slab_sums_views `odd`)."""
    mats, vecs, calls = _reject_calls()
    operands, call = calls[name]
    for op in operands:
        op, _, only = op.partition(":")
        for fault in ("base + 4 B", "stride + 2"):
            if only == "stride" and fault != "stride + 2":
                continue
            f = Frame("offset", f"{name}: {op} {fault}")
            v = {k: f.io(rnd(shape, 200 + i)) for i, (k, shape) in enumerate(mats.items())}
            v.update({k: f.io(rnd(n, 300 + i)) for i, (k, n) in enumerate(vecs.items())})
            v["lab"] = f.io(np.arange(16, dtype=np.int32))

            def P(k):
                return v[k].ptr + (4 if (k == op and fault == "base + 4 B") else 0)

            def ST(k):
                return v[k].stride + (2 if (k == op and fault == "stride + 2") else 0)

            def D(k):
                return MatrixDim(v[k].rows, v[k].cols, ST(k))

            f.rejected(call(P, D, ST))
    # and the unperturbed call is accepted: the rejections above are about the perturbation alone
    f = Frame("offset", f"{name}: unperturbed")
    v = {k: f.io(rnd(shape, 200 + i)) for i, (k, shape) in enumerate(mats.items())}
    v.update({k: f.io(rnd(n, 300 + i)) for i, (k, n) in enumerate(vecs.items())})
    v["lab"] = f.io(np.arange(16, dtype=np.int32))
    st = call(lambda k: v[k].ptr, lambda k: v[k].dim, lambda k: v[k].stride)
    assert st == TNET_OK, f"{name}: status {st}"
    for k, x in v.items():
        assert_frame_untouched(x, f"{name}: {k}")


# ------------------------------------------------------------------------------------------------------------------
# Part B: element-wise maps, reductions, gathers
# ------------------------------------------------------------------------------------------------------------------
EW_SHAPES = [(37, 131), (36, 132)]  # 36 x 132 on tight / offset: every f32x4 path; 37 x 131 and `odd`: the scalar ones


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def other_layout(layout):
    """a second operand on another stride than the matrix's (the three strides differ at every width: roundup4(c),
    roundup4(c) + 12, c + 3 -- except tight and odd at c % 4 == 1, which this map never pairs)"""
    return {"tight": "offset", "offset": "odd", "odd": "offset"}[layout]


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("rows,cols", EW_SHAPES)
def test_map_ops_exact_views(rows, cols, layout):
    """set_const, apply_mask, apply_l1, scale_cols, scale_rows, mul_elem: one fp32 rounding each, bit for bit
    against the same op in float32 numpy"""
    X = rnd((rows, cols), 22)
    L = lib()
    f = Frame(layout, "set_const")
    v = f.out(rows, cols)
    got, = f.done(L.tnetF_set_const(v.ptr, 3.5, v.dim, S()))
    assert (got == np.float32(3.5)).all()

    # a mask on another stride than the matrix; exact zeros, negative zeros and tiny values in it
    mask = (np.random.default_rng(30).random((rows, cols)) < 0.5).astype(np.float32)
    mask[0, :4] = [0.0, -0.0, 1e-45, -3.0]
    f = Frame(layout, "apply_mask")
    v, vm = f.io(X), f.inp(mask, other_layout(layout))
    assert vm.stride != v.stride
    got, = f.done(L.tnetF_apply_mask(v.ptr, vm.ptr, v.dim, vm.dim, S()))
    np.testing.assert_array_equal(bits(got), bits(np.where(mask == 0, np.float32(0), X)))

    # soft threshold: exactly at +-l1, just inside, just outside, +-0
    l1 = np.float32(0.3)
    Xl = X.copy()
    edge = [l1, -l1, np.nextafter(l1, np.float32(0)), -np.nextafter(l1, np.float32(0)),
            np.nextafter(l1, np.float32(1)), -np.nextafter(l1, np.float32(1)), 0.0, -0.0]
    Xl[0, :8] = edge
    Xl[-1, -8:] = edge
    f = Frame(layout, "apply_l1")
    v = f.io(Xl)
    got, = f.done(L.tnetF_apply_l1(v.ptr, l1, v.dim, S()))
    ref = np.where(np.abs(Xl) < l1, np.float32(0), np.where(Xl > 0, Xl - l1, Xl + l1)).astype(np.float32)
    np.testing.assert_array_equal(bits(got), bits(ref))
    assert got[0, 0] == 0 and got[0, 1] == 0 and got[0, 2] == 0 and got[0, 4] > 0 and got[0, 5] < 0

    sc, sr = rnd(cols, 31), rnd(rows, 32)
    f = Frame(layout, "scale_cols")
    v, vs = f.io(X), f.inp(sc)
    got, = f.done(L.tnetF_scale_cols(v.ptr, vs.ptr, v.dim, S()))
    np.testing.assert_array_equal(bits(got), bits(X * sc[None, :]))
    f = Frame(layout, "scale_rows")
    v, vs = f.io(X), f.inp(sr)
    got, = f.done(L.tnetF_scale_rows(v.ptr, vs.ptr, v.dim, S()))
    np.testing.assert_array_equal(bits(got), bits(X * sr[:, None]))

    A = rnd((rows, cols), 33)
    f = Frame(layout, "mul_elem")
    v, va = f.io(X), f.inp(A, other_layout(layout))
    assert va.stride != v.stride
    got, = f.done(L.tnetF_mul_elem(v.ptr, va.ptr, va.stride, v.dim, S()))
    np.testing.assert_array_equal(bits(got), bits(X * A))


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("rows,cols", EW_SHAPES)
def test_map_ops_rounded_views(rows, cols, layout):
    """add_scaled, add_scaled_row (rtol 1e-6 atol 1e-6: the compiler may contract to FMA), apply_log, log_elem
    (rtol 2e-6)"""
    X, A = rnd((rows, cols), 22), rnd((rows, cols), 34)
    L = lib()
    f = Frame(layout, "add_scaled")
    v, va = f.io(X), f.inp(A, other_layout(layout))
    assert va.stride != v.stride
    got, = f.done(L.tnetF_add_scaled(2.0, va.ptr, va.stride, 0.5, v.ptr, v.dim, S()))
    np.testing.assert_allclose(got, 2.0 * A.astype(np.float64) + 0.5 * X, rtol=1e-6, atol=1e-6)

    r = rnd(cols, 24)
    f = Frame(layout, "add_scaled_row")
    v, vr = f.io(X), f.inp(r)
    got, = f.done(L.tnetF_add_scaled_row(2.0, vr.ptr, 0.5, v.ptr, v.dim, S()))
    np.testing.assert_allclose(got, 2.0 * r.astype(np.float64) + 0.5 * X, rtol=1e-6, atol=1e-6)
    # beta == 0 over a poisoned destination: the destination is not read
    f = Frame(layout, "add_scaled_row beta 0")
    v, vr = f.out(rows, cols), f.inp(r)
    got, = f.done(L.tnetF_add_scaled_row(2.0, vr.ptr, 0.0, v.ptr, v.dim, S()))
    np.testing.assert_array_equal(bits(got), bits(np.broadcast_to(np.float32(2.0) * r, (rows, cols))))

    P = np.abs(rnd((rows, cols), 25)) + np.float32(1e-3)
    f = Frame(layout, "apply_log")
    v = f.io(P)
    got, = f.done(L.tnetF_apply_log(v.ptr, v.dim, S()))
    np.testing.assert_allclose(got, np.log(P.astype(np.float64)), rtol=2e-6, atol=0)

    # log_elem clamps at FLT_MIN: 0, a denormal and FLT_MIN itself all give log(FLT_MIN)
    Pc = P.copy()
    Pc[0, :3] = [0.0, 1e-45, FLT_MIN]
    Pc[-1, -3:] = [0.0, 1e-45, FLT_MIN]
    f = Frame(layout, "log_elem")
    v = f.io(Pc)
    got, = f.done(L.tnetF_log_elem(v.ptr, v.dim, S()))
    np.testing.assert_allclose(got, np.log(np.maximum(Pc, FLT_MIN).astype(np.float64)), rtol=2e-6, atol=0)
    assert (got[0, :3] == got[0, 2]).all() and abs(got[0, 2] + 87.33654) < 1e-3


def sigmoid_inputs(rows, cols, seed):
    X = rnd((rows, cols), seed, 3.0)
    X[0, :4] = [90.0, -90.0, 0.0, -0.0]
    X[-1, -4:] = [90.0, -90.0, 0.0, -0.0]
    return X


def check_sigmoid_pair(rows, cols, layout):
    """tnetF_sigmoid and tnetF_diff_sigmoid at one shape.  rtol 2e-6 of the module's element-wise bound with the
    atol 1e-7 of test_elementwise_ops: sigmoid(-90) is 8e-40, below the smallest normal float, where a relative bound
    on a flushed result means nothing"""
    X = sigmoid_inputs(rows, cols, 22)
    f = Frame(layout, f"sigmoid {rows}x{cols}")
    vx, vy = f.inp(X), f.out(rows, cols)
    got, = f.done(lib().tnetF_sigmoid(vy.ptr, vx.ptr, vx.dim, S()))
    ref = 1.0 / (1.0 + np.exp(-X.astype(np.float64)))
    np.testing.assert_allclose(got, ref, rtol=2e-6, atol=1e-7)
    assert got[0, 0] == 1.0 and got[0, 1] == 0.0  # exp overflow / underflow give exactly 0 / 1 (kcommon.h)
    Y = ref.astype(np.float32)
    E = rnd((rows, cols), 23)
    f = Frame(layout, f"diff_sigmoid {rows}x{cols}")
    ve, vy, vo = f.inp(E), f.inp(Y), f.out(rows, cols)
    got, = f.done(lib().tnetF_diff_sigmoid(vo.ptr, ve.ptr, vy.ptr, ve.dim, S()))
    Yd = Y.astype(np.float64)
    np.testing.assert_allclose(got, Yd * (1 - Yd) * E, rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("rows,cols", EW_SHAPES)
def test_sigmoid_views(rows, cols, layout):
    check_sigmoid_pair(rows, cols, layout)


@pytest.mark.parametrize("rows,cols,layout", [(1100, 2000, "odd"), (2112, 4000, "tight")])
def test_sigmoid_views_past_the_grid_cap(rows, cols, layout):
    """more elements than ew_grid's 8192 blocks x 256 threads cover in one pass: 1100 x 2000 scalar elements on
    `odd`, 2112 x 4000 / 4 float4 on `tight` -- the grid-stride loops' second pass"""
    assert rows * cols // (4 if layout == "tight" else 1) > 8192 * 256
    check_sigmoid_pair(rows, cols, layout)


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("n", [1, 1023, 8192 * 256 + 5])
def test_sgd_update_views(n, layout):
    """c = g + mmt*corr; p += scale*c; p += l2*p; corr = c on flat arrays (the last size is past the grid cap)"""
    p, g, c0 = rnd(n, 30), rnd(n, 50), rnd(n, 70, 0.1)
    scale, l2 = -0.01, -1e-4
    for mmt in (0.0, 0.9):
        f = Frame(layout, f"sgd_update n {n} mmt {mmt}")
        vp, vg = f.io(p), f.inp(g)
        vc = f.io(c0) if mmt else None
        got = f.done(lib().tnet_sgd_update(vp.ptr, vg.ptr, vc.ptr if vc else None, n, scale, mmt, l2, S()))
        cc = g.astype(np.float64) + mmt * c0
        w = p + scale * cc
        w = w + l2 * w
        np.testing.assert_allclose(got[0].ravel(), w, rtol=1e-6, atol=1e-6)
        if mmt:
            np.testing.assert_allclose(got[1].ravel(), cc, rtol=1e-6, atol=1e-6)
    # momentum without its buffer: TNET_ERR_ARG, nothing written
    f = Frame(layout, "sgd_update mmt 0.9 without corr")
    vp, vg = f.io(p), f.inp(g)
    f.rejected(lib().tnet_sgd_update(vp.ptr, vg.ptr, None, n, scale, 0.9, l2, S()))


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("rows,cols,src_rows", [(256, 440, 500), (256, 441, 500), (256, 8, 300), (16500, 8, 20000)])
def test_gathers_views(rows, cols, src_rows, layout):
    """tnetF_randomize, tnet_gather_i32, tnet_gather_bunch: rows and class ids exact; repeated and reversed indices;
    16,500 rows are more than the row gather's 4096 blocks x 4 waves take in one pass.  Neither randomize nor
    gather_bunch has a licence to write y's padding: the frame check is strict."""
    X = rnd((src_rows, cols), 26)
    lab = (np.arange(src_rows, dtype=np.int32) * 3) % 4001
    idx = np.random.default_rng(27).integers(0, src_rows, rows).astype(np.int32)
    idx[:8] = [5, 5, 5, src_rows - 1, 0, src_rows - 1, 0, 5]   # repeats, both ends
    idx[rows // 2:] = idx[rows // 2:][::-1].copy()
    idx[-16:] = np.arange(src_rows - 1, src_rows - 17, -1)       # a reversed run
    L = lib()
    f = Frame(layout, "randomize")
    vx, vi, vy = f.inp(X), f.inp(idx), f.out(rows, cols)
    got, = f.done(L.tnetF_randomize(vy.ptr, vx.ptr, vi.ptr, vy.dim, vx.dim, S()))
    np.testing.assert_array_equal(bits(got), bits(X[idx]))
    f = Frame(layout, "gather_i32")
    vl, vi, vo = f.inp(lab), f.inp(idx), f.out(1, rows, dtype=np.int32)
    got, = f.done(L.tnet_gather_i32(vo.ptr, vl.ptr, vi.ptr, rows, S()))
    np.testing.assert_array_equal(got.ravel(), lab[idx])
    f = Frame(layout, "gather_bunch")
    vx, vl, vi = f.inp(X), f.inp(lab), f.inp(idx)
    vy, vo = f.out(rows, cols), f.out(1, rows, dtype=np.int32)
    got, glab = f.done(L.tnet_gather_bunch(vy.ptr, vx.ptr, vo.ptr, vl.ptr, vi.ptr, vy.dim, vx.dim, S()))
    np.testing.assert_array_equal(bits(got), bits(X[idx]))
    np.testing.assert_array_equal(glab.ravel(), lab[idx])


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
def test_expand_rearrange_views(layout):
    L = lib()
    # expand: y[i, j] = x[clamp(i + off[j / cols]), j % cols]; offsets -5 .. +5 on 7 rows clamp at both ends
    X = rnd((7, 13), 80)
    off = np.arange(-5, 6, dtype=np.int32)
    f = Frame(layout, "expand")
    vx, vo, vy = f.inp(X), f.inp(off), f.out(7, 13 * len(off))
    got, = f.done(L.tnetF_expand(vy.ptr, vx.ptr, vo.ptr, vy.dim, vx.dim, S()))
    ref = np.concatenate([X[np.clip(np.arange(7) + o, 0, 6)] for o in off], axis=1)
    np.testing.assert_array_equal(bits(got), bits(ref))
    # rearrange: y[i, j] = x[i, copy_from[j]], out of range and negative sources give +inf
    X = rnd((9, 21), 81)
    cf = np.array([20, 0, -1, 21, 7, 7, 1000, -2147483648, 3, 19, 2147483647], np.int32)
    f = Frame(layout, "rearrange")
    vx, vc, vy = f.inp(X), f.inp(cf), f.out(9, len(cf))
    got, = f.done(L.tnetF_rearrange(vy.ptr, vx.ptr, vc.ptr, vy.dim, vx.dim, S()))
    ok = (cf >= 0) & (cf < 21)
    ref = np.where(ok[None, :], X[:, np.where(ok, cf, 0)], np.float32(np.inf))
    np.testing.assert_array_equal(bits(got), bits(ref))
    assert np.isposinf(got[:, ~ok]).all()


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("blocks,bi,bo,rows", [(3, 5, 7, 19), (4, 16, 8, 33)])
def test_block_linearity_views(blocks, bi, bo, rows, layout):
    """y[:, b*bo:(b+1)*bo] = x[:, b*bi:(b+1)*bi] . t, "any strides/offsets".  One fma per term in i order (frontend.hip):
    error <= bi * U * sum_i |x_i t_i|"""
    X, T = rnd((rows, blocks * bi), 82), rnd((bi, bo), 83)
    f = Frame(layout, "block_linearity")
    vx, vt, vy = f.inp(X), f.inp(T, other_layout(layout)), f.out(rows, blocks * bo)
    got, = f.done(lib().tnet_block_linearity(vy.ptr, vy.dim, vx.ptr, vx.dim, vt.ptr, vt.dim, S()))
    Xb = X.astype(np.float64).reshape(rows, blocks, bi)
    ref = np.einsum("rbi,io->rbo", Xb, T.astype(np.float64)).reshape(rows, blocks * bo)
    mag = np.einsum("rbi,io->rbo", np.abs(Xb), np.abs(T).astype(np.float64)).reshape(rows, blocks * bo)
    within(got, ref, bi * U * mag + 1e-30, f.what)


def nan_workspace(d):
    """a column-sum workspace whose contents are NaN: the kernels must write what they read of it"""
    n = max(1, lib().tnet_col_sum_workspace(d) // 4 + 64)
    return DeviceArray.from_numpy(np.full((1, n), np.nan, np.float32), stride=n)


def colsum_tol(M, rows_per_slab):
    """The column-sum bound of this module.  It deliberately departs from tests/test_gpu_kernels.py's "reductions:
    rtol 1e-5" (test_col_sum_and_bias_update: rtol 1e-5, atol 1e-5 on the same entry points): a column sum of
    signed values cancels, so a bound relative to |sum| is arbitrarily tight where the sum happens to be small and
    8200 rows of unit normals leave |sum| ~ 90 against sum|x| ~ 6500.  This one is relative to sum|x| instead, from
    the precision of the format and the reduction's depth -- tighter than rtol 1e-5 at 33 rows, 3-6 times looser
    relative to |sum| at 2049 and 8200 -- and a leaked, dropped or doubled row still misses it by orders of
    magnitude (one row is 1 / rows of sum|x|, the bound 7e-7 of it).  The depth is that of reduce.hip's
    colsum_partial_block as it stands; a reduction that reorders the additions within a slab keeps it, one that adds
    more of them in sequence would have to restate it.
    fp32 sums inside a slab (each element passes through at most ceil(rows_per_slab / 4) + 3 additions: its row
    sub-group's chain, then the 4 sub-group sums), fp64 across slabs: |error| <= that depth * U * colsum(|M|)"""
    return (-(-rows_per_slab // 4) + 3) * U * np.abs(M).astype(np.float64).sum(0)


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("rows,cols", [(33, 7), (64, 132), (2049, 77), (8200, 12), (8200, 7)])
def test_colsum_family_views(rows, cols, layout):
    """tnetF_add_col_sum, tnet_bias_update (momentum-free, momentum, grad_out) and tnet_rbm_bias_update; 8200 rows
    are past cs_slabs' cap of 256 slabs: a slab is 33 rows there.  Bounds: colsum_tol for the sum, plus one rounding
    (U) of each term of the update that follows it"""
    E = rnd((rows, cols), 18)
    slabs = min(256, -(-rows // 32))
    rps = -(-rows // slabs)
    assert (rows == 8200) == (rps > 32)
    cs = E.astype(np.float64).sum(0)
    tol = colsum_tol(E, rps)
    L = lib()

    for beta, v0 in ((2.0, rnd(cols, 19)), (0.0, None)):
        f = Frame(layout, f"add_col_sum beta {beta}")
        vE = f.inp(E)
        vv = f.io(v0) if beta else f.out(1, cols)  # beta == 0 over a poisoned vector: not read
        ws = nan_workspace(vE.dim)
        got, = f.done(L.tnetF_add_col_sum(0.5, vE.ptr, beta, vv.ptr, vE.dim, ws.ptr, S()))
        ref = 0.5 * cs + (beta * v0 if beta else 0.0)
        within(got.ravel(), ref, 0.5 * tol + 2 * U * (np.abs(0.5 * cs) + np.abs(ref)) + 1e-30, f.what)

    b0, cb0 = rnd(cols, 20), rnd(cols, 21)
    scale = -0.01
    for mmt in (0.0, 0.9):
        f = Frame(layout, f"bias_update mmt {mmt}")
        vE, vb = f.inp(E), f.io(b0)
        vcb = f.io(cb0) if mmt else None
        ws = nan_workspace(vE.dim)
        got = f.done(L.tnet_bias_update(vE.ptr, vE.dim, vb.ptr, vcb.ptr if vcb else None, None, scale, mmt, ws.ptr, S()))
        c = cs + mmt * cb0
        ctol = tol + 3 * U * (np.abs(cs) + np.abs(mmt * cb0)) + 1e-30
        within(got[0].ravel(), b0 + scale * c, abs(scale) * ctol + 2 * U * (np.abs(b0) + np.abs(scale * c)), f.what + " b")
        if mmt:
            within(got[1].ravel(), c, ctol, f.what + " corr_b")
    # grad_out: the raw column sum; b is not touched
    f = Frame(layout, "bias_update grad_out")
    vE, vb, vg = f.inp(E), f.inp(b0), f.out(1, cols)
    ws = nan_workspace(vE.dim)
    got, = f.done(L.tnet_bias_update(vE.ptr, vE.dim, vb.ptr, None, vg.ptr, scale, 0.0, ws.ptr, S()))
    within(got.ravel(), cs, tol + U * np.abs(cs) + 1e-30, f.what)

    # RBM form: rows from neg_from on enter negated; neg_from inside a slab
    neg_from = (rows // 2) | 5
    assert neg_from % rps != 0 and 0 < neg_from < rows
    sg = np.where(np.arange(rows) < neg_from, 1.0, -1.0)[:, None]
    scs = (E.astype(np.float64) * sg).sum(0)
    mmt, scale = 0.5, 0.1 / rows
    f = Frame(layout, "rbm_bias_update")
    vE, vb, vcb = f.inp(E), f.io(b0), f.io(cb0)
    ws = nan_workspace(vE.dim)
    b, cb = f.done(L.tnet_rbm_bias_update(vE.ptr, vE.dim, neg_from, vb.ptr, vcb.ptr, scale, mmt, ws.ptr, S()))
    c = mmt * cb0 + scale * scs
    ctol = abs(scale) * (tol + U * np.abs(scs)) + 3 * U * (np.abs(mmt * cb0) + np.abs(scale * scs)) + 1e-30
    within(cb.ravel(), c, ctol, f.what + " corr_b")
    within(b.ravel(), b0 + c, ctol + 2 * U * (np.abs(b0) + np.abs(c)), f.what + " b")


SOFTMAX_COLS = [1, 7, 256, 1024, 1028, 4096, 4100]


def logits(rows, cols, seed):
    """logits scaled by 3, one row with a +200 spike (every other probability of that row underflows)"""
    Z = rnd((rows, cols), seed, 3.0)
    Z[2, cols // 2] += 200.0
    return Z


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_views(cols, layout):
    """tnetF_softmax, 5 rows (a partial last workgroup of 4 rows).  Out of place only: no host caller aliases y and
    x -- CuSoftmax::PropagateFnc (culayers.cpp) passes the component's own output matrix and its predecessor's, and
    CuMath::Softmax has no other caller."""
    rows = 5
    Z = logits(rows, cols, 16)
    f = Frame(layout, "softmax")
    vx, vy = f.inp(Z), f.out(rows, cols)
    assert vx.stride == vy.stride
    got, = f.done(lib().tnetF_softmax(vy.ptr, vx.ptr, vx.dim, S()))
    z = Z.astype(np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    np.testing.assert_allclose(got, e / e.sum(1, keepdims=True), rtol=2e-5, atol=1e-9)
    assert np.all(np.abs(got.astype(np.float64).sum(1) - 1.0) <= 1e-6)


def xent_labels(rows, cols, seed):
    lab = np.random.default_rng(seed).integers(0, cols, size=rows).astype(np.int32)
    lab[0] = -1            # unlabeled
    lab[1] = cols          # out of range: treated as unlabeled
    lab[3] = cols + 1000
    lab[4] = cols - 1
    return lab


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_xent_views(cols, layout):
    """tnet_softmax_xent from logits (the one-wave-per-row kernel and, from 1028 columns on 16-B layouts, the
    four-waves-per-row one) and with Z == NULL -- the only way CuCrossEntropy::EvaluateLabels calls it: Y holds the
    probabilities on another stride than E, and must be bit-identical afterwards"""
    rows = 6
    Z = logits(rows, cols, 16)
    lab = xent_labels(rows, cols, 17)
    ref_lab = np.where(lab >= cols, -1, lab).astype(np.int32)
    f = Frame(layout, "softmax_xent from Z")
    vZ, vL = f.inp(Z), f.inp(lab)
    vY, vE = f.out(rows, cols), f.out(rows, cols)
    stats = DeviceArray(1, 1024, np.float64, stride=1024)
    Y, E = f.done(lib().tnet_softmax_xent(vZ.ptr, vZ.dim, vL.ptr, vY.ptr, vY.stride, vE.ptr, vE.stride, stats.ptr, S()))
    Yref = orc.softmax(Z)
    Eref, xent, correct = orc.xent_eval(Yref, ref_lab)
    np.testing.assert_allclose(Y, Yref, rtol=2e-5, atol=1e-9)
    np.testing.assert_allclose(E, Eref, rtol=2e-5, atol=1e-8)
    s = stats.numpy()[0]
    np.testing.assert_allclose(s[0::2].sum(), xent, rtol=1e-5, atol=1e-5)
    assert int(round(s[1::2].sum())) == correct

    f = Frame(layout, "softmax_xent Z == NULL")
    vY, vL = f.inp(Yref), f.inp(lab)   # Y is a pure input here
    vE = f.out(rows, cols, other_layout(layout))
    assert vY.stride != vE.stride
    stats = DeviceArray(1, 1024, np.float64, stride=1024)
    E, = f.done(lib().tnet_softmax_xent(None, vY.dim, vL.ptr, vY.ptr, vY.stride, vE.ptr, vE.stride, stats.ptr, S()))
    np.testing.assert_allclose(E, Eref, rtol=2e-5, atol=1e-8)
    s = stats.numpy()[0]
    np.testing.assert_allclose(s[0::2].sum(), xent, rtol=1e-5, atol=1e-5)
    assert int(round(s[1::2].sum())) == correct


DENSE_ROWS = 7
DENSE_MATCH = [1, 1, 1, 1, 1, 0, 1]  # what each row of dense_case adds to `correct` (cols >= 4)


def dense_case(cols):
    """logits Z and dense targets D of DENSE_ROWS rows.  For cols >= 4 each row's contribution to `correct` is fixed by
    construction, and rows 2, 3, 4 and 6 match ONLY under the reference's rules (first maximum wins, on either side;
    an all-zero target row's argmax is column 0):
      0  one-hot target, the output's maximum on the same column                                      match
      1  soft target (a Dirichlet draw), the output's maximum on the target's                         match
      2  all-zero target, the output's maximum on column 0                                            match
      3  target tie at columns 1 and cols-1, output tie at columns 1 and cols-2                       match
         (last-wins on either side, or on both, gives cols-1 / cols-2: no match)
      4  one-hot target at column 2, output tie at columns 2 and cols-1 (the output's rule alone)     match
      5  a +200 spike at cols // 2, the whole target on column 0, whose probability underflows:
         -log(FLT_MIN) in the cross-entropy                                                           no match
      6  target tie at columns 0 and cols-2, the output's maximum on column 0 (the target's rule)     match
    Below 4 columns the rows are plain one-hot / soft targets on random logits."""
    rng = np.random.default_rng(18)
    Z = logits(DENSE_ROWS, cols, 16)
    D = np.zeros((DENSE_ROWS, cols), np.float32)
    for r in range(DENSE_ROWS):
        if r % 2 == 0:
            D[r, rng.integers(0, cols)] = 1.0
        else:
            D[r] = rng.dirichlet(np.ones(cols)).astype(np.float32)
    if cols < 4:
        return Z, D, None
    top = np.float32(40.0)
    Z[5] = Z[2]                                   # the spike row
    D[5] = 0.0
    D[5, 0] = 1.0
    Z[2] = rnd((1, cols), 17, 3.0)[0]
    Z[0, D[0].argmax()] = top
    Z[1, D[1].argmax()] = top
    D[2] = 0.0
    Z[2, 0] = top
    D[3] = 0.0
    D[3, [1, cols - 1]] = 0.5
    Z[3, [1, cols - 2]] = top
    D[4] = 0.0
    D[4, 2] = 1.0
    Z[4, [2, cols - 1]] = top
    D[6] = 0.0
    D[6, [0, cols - 2]] = 0.5
    Z[6, 0] = top
    return Z, D, DENSE_MATCH


def dense_ref(Y, D):
    """E, xent, correct of CuCrossEntropy::Evaluate for probabilities Y (fp64; first maximum wins)"""
    Yd, Dd = Y.astype(np.float64), D.astype(np.float64)
    xent = -(Dd * np.log(np.maximum(Y, FLT_MIN).astype(np.float64))).sum()
    per_row = (Y.argmax(1) == D.argmax(1)).astype(int)
    return Yd - Dd, xent, int(per_row.sum()), per_row


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_xent_dense_views(cols, layout):
    """tnet_softmax_xent_dense with logits and with Z == NULL; D on its own stride.  One-hot, soft and all-zero
    target rows, tied maxima in the target and in the output, a probability at the FLT_MIN clamp (dense_case).  The
    asserted `correct` is 6 of 7 by construction: a kernel with another tie rule on either side, or another argmax
    for the all-zero row, counts fewer"""
    rows = DENSE_ROWS
    Z, D, match = dense_case(cols)
    f = Frame(layout, "softmax_xent_dense from Z")
    vZ, vD = f.inp(Z), f.inp(D, other_layout(layout))
    vY, vE = f.out(rows, cols), f.out(rows, cols)
    assert vD.stride != vY.stride
    stats = DeviceArray(1, 1024, np.float64, stride=1024)
    Y, E = f.done(lib().tnet_softmax_xent_dense(vZ.ptr, vZ.dim, vD.ptr, vD.stride, vY.ptr, vY.stride, vE.ptr, vE.stride,
                                                stats.ptr, S()))
    Yref = orc.softmax(Z)
    np.testing.assert_allclose(Y, Yref, rtol=2e-5, atol=1e-9)
    Eref, xent, correct, per_row = dense_ref(Y, D)   # the statistics of the kernel's own probabilities
    if match:  # the rows' matches are what dense_case constructs, not merely what numpy's argmax gives here
        assert list(per_row) == match and correct == sum(match)
    np.testing.assert_allclose(E, Eref, rtol=2e-5, atol=1e-8)
    s = stats.numpy()[0]
    np.testing.assert_allclose(s[0::2].sum(), xent, rtol=1e-5, atol=1e-5)
    assert int(round(s[1::2].sum())) == correct
    if cols >= 4:
        assert Y[5, 0] == 0.0 and xent >= -np.log(np.float64(FLT_MIN))  # the clamp was reached

    f = Frame(layout, "softmax_xent_dense Z == NULL")
    vY, vD = f.inp(Yref), f.inp(D, other_layout(layout))
    vE = f.out(rows, cols)
    stats = DeviceArray(1, 1024, np.float64, stride=1024)
    E, = f.done(lib().tnet_softmax_xent_dense(None, vY.dim, vD.ptr, vD.stride, vY.ptr, vY.stride, vE.ptr, vE.stride,
                                              stats.ptr, S()))
    Eref, xent, correct, per_row = dense_ref(Yref, D)
    if match:
        assert list(per_row) == match and correct == sum(match)
    np.testing.assert_allclose(E, Eref, rtol=2e-5, atol=1e-8)
    s = stats.numpy()[0]
    np.testing.assert_allclose(s[0::2].sum(), xent, rtol=1e-5, atol=1e-5)
    assert int(round(s[1::2].sum())) == correct


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("rows,cols", [(5, 7), (37, 131), (36, 132)])
def test_mse_views(rows, cols, layout):
    """E = Y - D (one rounding: bit for bit), error += sum E^2; with E and with E == NULL; D on its own stride"""
    Y, D = rnd((rows, cols), 90), rnd((rows, cols), 91)
    e = Y - D
    ref = (e.astype(np.float64) ** 2).sum()
    for with_e in (True, False):
        f = Frame(layout, f"mse E {with_e}")
        vY, vD = f.inp(Y), f.inp(D, other_layout(layout))
        vE = f.out(rows, cols) if with_e else None
        stats = DeviceArray(1, 1024, np.float64, stride=1024)
        got = f.done(lib().tnet_mse(vY.ptr, vY.dim, vD.ptr, vD.stride, vE.ptr if vE else None, vE.stride if vE else 0,
                                    stats.ptr, S()))
        if with_e:
            np.testing.assert_array_equal(bits(got[0]), bits(e))
        s = stats.numpy()[0]
        np.testing.assert_allclose(s[0::2].sum(), ref, rtol=1e-5)  # e*e is rounded to fp32 before the fp64 sum
        assert s[1::2].sum() == 0


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("cols", [300, 4100])
def test_check_class_views(cols, layout):
    """match[i] = argmax(out[i]) == argmax(des[i]), first maximum wins -- also when the tied maxima sit on different
    lanes and in different passes of a lane's column loop"""
    rows = 9
    out, des = rnd((rows, cols), 92), np.zeros((rows, cols), np.float32)
    des[np.arange(rows), np.random.default_rng(93).integers(0, cols, rows)] = 1.0
    top = np.float32(50.0)
    out[0, [3, 67]] = top                 # a tie across lanes 3 and 3 + 64 (the same lane, next pass): column 3
    des[0] = 0
    des[0, 3] = 1.0
    out[1, [10, 11]] = top                # a tie across neighbouring lanes: column 10
    des[1] = 0
    des[1, 11] = 1.0                      # -> no match
    out[2, [cols - 1, 64]] = top          # the last column ties with an earlier one: column 64
    des[2] = 0
    des[2, 64] = 1.0
    des[3] = 0                            # all-zero target: its argmax is column 0
    out[3, 0] = top
    des[4] = 0
    des[4, [5, 200]] = 0.5                # a tie in the target: column 5
    out[4, 200] = top                     # -> no match
    f = Frame(layout, "check_class")
    vo, vd = f.inp(out), f.inp(des)
    vm = f.out(1, rows, dtype=np.int32)
    got, = f.done(lib().tnetF_check_class(vo.ptr, vd.ptr, vm.ptr, vo.dim, S()))
    ref = (out.argmax(1) == des.argmax(1)).astype(np.int32)
    np.testing.assert_array_equal(got.ravel(), ref)
    assert list(ref[:5]) == [1, 0, 1, 1, 0]
