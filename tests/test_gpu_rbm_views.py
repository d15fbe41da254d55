"""The RBM step kernels (rand.hip, rbm_stats_kernel / rbm_stats.h, tnet_affine_fwd_sample, tnet_rbm_update_stats and
its gather form) on caller-owned views: the method of tests/test_gpu_rnn_views.py (Ops: poisoned frames, pure inputs
bit-identical, no NaN in an output, values against what tests/test_gpu_rbm.py compares with, at its bounds).

Layouts, as read in the code.  rand.hip's kernels and rbm_stats_block make scalar accesses only and no header comment
asks for an alignment or a stride: tight, offset and odd.  tnet_affine_fwd_sample and tnet_rbm_update_stats[_gather]
are GEMM entry points: check_common (gemm_f32.hip) answers a stride off 4 or a base off 16 bytes with TNET_ERR_ARG, as
tests/test_gpu_views.py shows for the family, so they run in tight and offset; the gather form's own requirement
(y and x 16-byte aligned with strides that are multiples of 4, else TNET_ERR_UNSUPPORTED) is asserted with y in `odd`.

The four HybridTaus state arrays are uint32 views with the target's geometry (index = col + row * stride): the
interior must equal the host generator's state after the same draws (advanced by exactly the reference's number of
draws), and every state word of the frame -- column padding, the band before column 0, guard rows -- is unchanged.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as orc  # noqa: E402
from kernel_views import GUARD, POISON, PoisonView, frame_violation  # noqa: E402
from test_gpu_rnn_views import LAYOUTS, Ops, P, S, TNET_ERR_ARG, U, close, rnd, within  # noqa: E402
from tnet_amd._lib import MatrixDim, lib  # noqa: E402

GEMM_LAYOUTS = ["tight", "offset"]
OTHER = {"tight": "offset", "offset": "odd", "odd": "tight"}  # a second operand on another stride


def states(f, rs, rows, cols):
    return [f.io(z.reshape(rows, cols), np.uint32) for z in rs.z]


def assert_states(zs, rs, what):
    for k, (v, z) in enumerate(zip(zs, rs.z)):
        np.testing.assert_array_equal(v.numpy().reshape(-1), z, err_msg=f"{what}: generator state z{k + 1}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,cols", [(3, 70), (17, 300)])
def test_rand_entry_points_views(rows, cols, layout):
    """(3, 70): one 256-column block with a tail; (17, 300): two.  Uniforms and binarised states bit-exact against the
    host generator, Gaussians within test_gauss_rand_and_noise's 2e-5; tnet_rand_binarize writes states of another
    stride than the probabilities'"""
    L = lib()
    rs = orc.RandState(1234 + cols, rows, cols)
    f = Ops(layout, f"tnetF_rand ({rows}, {cols})")
    zs, out = states(f, rs, rows, cols), f.out(rows, cols)
    assert all(z.stride == out.stride for z in zs)
    for _ in range(2):
        f.check(L.tnetF_rand(out.ptr, out.dim, *[z.ptr for z in zs], S()))
        np.testing.assert_array_equal(out.numpy(), rs.uniform(), err_msg=f.what)
        assert_states(zs, rs, f.what)

    f = Ops(layout, f"tnetF_gauss_rand ({rows}, {cols})")
    zs, out = states(f, rs, rows, cols), f.out(rows, cols)
    f.check(L.tnetF_gauss_rand(out.ptr, out.dim, *[z.ptr for z in zs], S()))
    close(out.numpy(), rs.gauss(), 0.0, 2e-5, f.what)
    assert_states(zs, rs, f.what)

    f = Ops(layout, f"tnet_add_gauss_noise ({rows}, {cols})")
    base = rnd((rows, cols), 5)
    zs, tgt = states(f, rs, rows, cols), f.io(base)
    f.check(L.tnet_add_gauss_noise(tgt.ptr, tgt.dim, 0.5, *[z.ptr for z in zs], S()))
    close(tgt.numpy(), base + 0.5 * rs.gauss(), 0.0, 2e-5, f.what)
    assert_states(zs, rs, f.what)

    Pm = np.random.default_rng(3).random((rows, cols)).astype(np.float32)
    f = Ops(layout, f"tnet_rand_binarize ({rows}, {cols})")
    zs, vP = states(f, rs, rows, cols), f.inp(Pm)
    g = Ops(OTHER[layout], f.what + ": the states")
    st = g.out(rows, cols)
    assert st.stride != vP.stride
    rc = L.tnet_rand_binarize(st.ptr, st.stride, vP.ptr, vP.dim, *[z.ptr for z in zs], S())
    f.check(rc)
    g.check(rc)
    u = rs.uniform()
    np.testing.assert_array_equal(st.numpy(), (Pm > u).astype(np.float32), err_msg=f.what)
    assert_states(zs, rs, f.what)

    f = Ops(layout, f"tnetF_binarize_probs ({rows}, {cols})")
    vP, vU, st = f.inp(Pm), f.inp(u), f.out(rows, cols)
    f.check(L.tnetF_binarize_probs(st.ptr, vP.ptr, vU.ptr, vP.dim, S()))
    np.testing.assert_array_equal(st.numpy(), (Pm > u).astype(np.float32), err_msg=f.what)


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("rows,V,H", [(1, 5, 3), (33, 37, 70), (64, 64, 128)])
def test_affine_fwd_sample_views(rows, V, H, layout):
    """Y, the states and the advanced generator states bit-identical (whole buffers) to tnet_affine_fwd(act 1) +
    tnet_rand_binarize on views of the same layout; the states are the host generator's draws; Y at test_affine_fwd's
    sigmoid bound"""
    X, W, b = rnd((rows, V), 40 + V), rnd((V, H), 41 + H, 0.05), rnd(H, 42)
    L, raws = lib(), []
    for fused in (True, False):
        rs = orc.RandState(31, rows, H)
        f = Ops(layout, f"{'affine_fwd_sample' if fused else 'affine_fwd + rand_binarize'} ({rows}, {V}, {H})")
        vX, vW, vb = f.inp(X), f.inp(W), f.inp(b)
        vY, st, zs = f.out(rows, H), f.out(rows, H), states(f, rs, rows, H)
        if fused:
            f.check(L.tnet_affine_fwd_sample(vX.ptr, vX.dim, vW.ptr, vW.dim, vb.ptr, vY.ptr, vY.dim, st.ptr, st.stride,
                                             *[z.ptr for z in zs], S()))
        else:
            f.check(L.tnet_affine_fwd(vX.ptr, vX.dim, vW.ptr, vW.dim, vb.ptr, vY.ptr, vY.dim, 1, S()), partial=(st,))
            f.check(L.tnet_rand_binarize(st.ptr, st.stride, vY.ptr, vY.dim, *[z.ptr for z in zs], S()))
        Y = vY.numpy()
        np.testing.assert_array_equal(st.numpy(), (Y > rs.uniform()).astype(np.float32), err_msg=f.what)
        assert_states(zs, rs, f.what)
        a = X.astype(np.float64) @ W + b
        sig = 1 / (1 + np.exp(-a))
        within(Y, sig, 2e-5 * (np.abs(X).astype(np.float64) @ np.abs(W)) * sig * (1 - sig) + 2e-6, f.what + " Y")
        raws.append([v.raw() for v in [vY, st] + zs])
    for x, y, name in zip(raws[0], raws[1], ("Y", "states", "z1", "z2", "z3", "z4")):
        np.testing.assert_array_equal(x, y, err_msg=f"fused vs two launches: {name} (whole buffers)")


# ------------------------------------------------------------------------------------------------------------------
# the CD-1 statistics
# ------------------------------------------------------------------------------------------------------------------
def cd1_case(V, H, B):
    rng = np.random.default_rng([V, H, B])
    Vs = rng.standard_normal((2 * B, V)).astype(np.float32)
    Hs = rng.random((2 * B, H)).astype(np.float32)
    Hs[B:] *= -1  # the negative phase stored negated
    return dict(Vs=Vs, Hs=Hs, W=rnd((V, H), 50, 0.05), cW=rnd((V, H), 51, 0.01), vb=rnd(V, 52), hb=rnd(H, 53),
                cvb=rnd(V, 54, 0.01), chb=rnd(H, 55, 0.01), B=B)


def stats_reference(d, scale, mmt):
    """fp64: c_v = mmt c_v + scale (sum pos_vis - sum neg_vis), c_h = mmt c_h + scale (sum of all rows of Hs), the
    biases plus those, the reconstruction error sum (neg_vis - pos_vis)^2; with each momentum's tolerance.  The sums'
    bound is the column-sum bound of tests/test_gpu_views.py (colsum_tol: fp32 inside a slab, each element through at
    most ceil(rows_per_slab / 4) + 3 additions, fp64 across slabs) and test_colsum_family_views's terms for the
    update that follows: one rounding of the sum, three of the momentum form's terms"""
    B, Vs, Hs = d["B"], d["Vs"].astype(np.float64), d["Hs"].astype(np.float64)
    rows = 2 * B
    slabs = min(256, -(-rows // 32))
    depth = -(-(-(-rows // slabs)) // 4) + 3
    out = {}
    for name, s, sa, c0, b0 in (("v", Vs[:B].sum(0) - Vs[B:].sum(0), np.abs(Vs).sum(0), d["cvb"], d["vb"]),
                                ("h", Hs.sum(0), np.abs(Hs).sum(0), d["chb"], d["hb"])):
        c = mmt * c0 + scale * s
        ctol = abs(scale) * (depth * U * sa + U * np.abs(s)) + 3 * U * (np.abs(mmt * c0) + np.abs(scale * s)) + 1e-30
        out[name] = (c, ctol, b0 + c, ctol + 2 * U * (np.abs(b0) + np.abs(c)))
    e = Vs[B:] - Vs[:B]
    out["mse"] = float((e * e).sum())
    return out


def check_stats(d, ref, vvb, vcvb, vhb, vchb, vst, what):
    for name, vb, vc in (("v", vvb, vcvb), ("h", vhb, vchb)):
        c, ctol, b, btol = ref[name]
        within(vc.numpy()[0], c, ctol, f"{what}: momentum of the {name} bias")
        within(vb.numpy()[0], b, btol, f"{what}: {name} bias")
    if vst is not None:
        st = vst.numpy()[0]
        np.testing.assert_allclose(st[0::2].sum(), ref["mse"], rtol=1e-6, err_msg=what + " MSE")
        assert not st[1::2].any(), what + ": a `correct` slot was written"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("V,H,B", [(5, 3, 1), (33, 70, 17), (64, 130, 600)])
def test_rbm_stats_update_views(V, H, B, layout):
    """(5, 3, 1): one slab of two rows; (33, 70, 17): two slabs, column blocks with a tail; (64, 130, 600): 38 slabs (a
    second group of 32 for the waves), 75 MSE blocks.  mse_stats NULL and an 8-byte view; the biases and their momenta
    bit-identical to two tnet_rbm_bias_update calls on views of the same layout, and inside the column-sum bound"""
    d = cd1_case(V, H, B)
    scale, mmt = 0.1 / B, 0.5
    ref = stats_reference(d, scale, mmt)
    L = lib()
    got = {}
    for mode in ("fused", "fused without mse", "bias_update"):
        f = Ops(layout, f"rbm_stats_update ({V}, {H}, {B}) {mode}")
        vV, vH = f.inp(d["Vs"]), f.inp(d["Hs"])
        vvb, vcvb, vhb, vchb = f.io(d["vb"]), f.io(d["cvb"]), f.io(d["hb"]), f.io(d["chb"])
        vst = f.io(np.zeros(1024), np.float64) if mode == "fused" else None
        if mode == "bias_update":
            f.check(L.tnet_rbm_bias_update(vV.ptr, vV.dim, B, vvb.ptr, vcvb.ptr, scale, mmt, None, S()))
            f.check(L.tnet_rbm_bias_update(vH.ptr, vH.dim, 2 * B, vhb.ptr, vchb.ptr, scale, mmt, None, S()))
        else:
            f.check(L.tnet_rbm_stats_update(vV.ptr, vV.dim, vH.ptr, vH.dim, B, vvb.ptr, vcvb.ptr, vhb.ptr, vchb.ptr,
                                            scale, mmt, P(vst), S()))
        check_stats(d, ref, vvb, vcvb, vhb, vchb, vst, f.what)
        got[mode] = [v.raw() for v in (vvb, vcvb, vhb, vchb)]
    for mode in ("fused without mse", "bias_update"):
        for x, y, name in zip(got["fused"], got[mode], ("vb", "cvb", "hb", "chb")):
            np.testing.assert_array_equal(x, y, err_msg=f"fused vs {mode}: {name} (whole buffers)")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rbm_stats_update_refusal_views(layout):
    """B = 4097: 8194 rows are more than 256 slabs of 32: TNET_ERR_UNSUPPORTED, nothing written"""
    d = cd1_case(5, 3, 4097)
    f = Ops(layout, "rbm_stats_update B 4097")
    vV, vH = f.inp(d["Vs"]), f.inp(d["Hs"])
    vvb, vcvb, vhb, vchb = f.io(d["vb"]), f.io(d["cvb"]), f.io(d["hb"]), f.io(d["chb"])
    vst = f.io(np.zeros(1024), np.float64)
    f.refused(lib().tnet_rbm_stats_update(vV.ptr, vV.dim, vH.ptr, vH.dim, 4097, vvb.ptr, vcvb.ptr, vhb.ptr, vchb.ptr,
                                          0.1, 0.5, vst.ptr, S()))


# ------------------------------------------------------------------------------------------------------------------
# tnet_rbm_update_stats, tnet_rbm_update_stats_gather
# ------------------------------------------------------------------------------------------------------------------
class Cd1Views:
    """the operands of one CD-1 update + statistics on views of one layout"""

    def __init__(self, f, d):
        self.V, self.H = f.inp(d["Vs"]), f.inp(d["Hs"])
        self.W, self.cW = f.io(d["W"]), f.io(d["cW"])
        self.vb, self.cvb, self.hb, self.chb = f.io(d["vb"]), f.io(d["cvb"]), f.io(d["hb"]), f.io(d["chb"])
        self.st = f.io(np.zeros(1024), np.float64)

    def head(self, scale, mmt, l2, B):
        return [self.V.ptr, self.V.dim, self.H.ptr, self.H.dim, self.W.ptr, self.W.dim, self.cW.ptr, self.cW.stride,
                scale, mmt, l2, B, self.vb.ptr, self.cvb.ptr, self.hb.ptr, self.chb.ptr, self.st.ptr]

    def raws(self):
        return [v.raw() for v in (self.W, self.cW, self.vb, self.cvb, self.hb, self.chb)]


def check_update(d, o, scale, mmt, l2, what):
    """test_rbm_update_views's bound (tests/test_gpu_views.py): the GEMM term, one rounding for each of the three sums
    of corr, and for W that of W + corr"""
    Vs, Hs = d["Vs"].astype(np.float64), d["Hs"].astype(np.float64)
    g, mag = Vs.T @ Hs, np.abs(Vs).T @ np.abs(Hs)
    c = mmt * d["cW"] + scale * g + l2 * d["W"]
    terms = np.abs(mmt * d["cW"]) + np.abs(scale * g) + np.abs(l2 * d["W"])
    tol = 2e-5 * abs(scale) * mag + 3 * U * terms + 1e-9
    within(o.cW.numpy(), c, tol, what + " corrW")
    within(o.W.numpy(), d["W"] + c, tol + 2e-7 * np.abs(d["W"]) + 1e-7, what + " W")


# The fused form is accepted where, in rbm_update_stats_run (gemm_f32.hip): B > 0 and 2 B <= 8192 (CS_ROWS *
# RS_MAX_SLABS), no forced GEMM configuration, pairing on, and plan_gemm<false> gives the 64x64 configuration unsplit --
# for a small V x H that is its last `else` (fewer than 200 64x64 tiles, A not k-contiguous) with ks = 1 because
# K = 2 B < 1024.  (5, 3, 1) is the smallest shape there is; (33, 70, 17) has two column tiles and every edge.
@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("V,H,B", [(5, 3, 1), (33, 70, 17)])
def test_rbm_update_stats_views(V, H, B, layout):
    """one launch == tnet_rbm_update + tnet_rbm_stats_update on views of the same layout: W, its momentum, the biases
    and their momenta bit for bit (whole buffers), the MSE sums equal; against fp64 at the separate calls' bounds"""
    d = cd1_case(V, H, B)
    lr, mmt, wc = 0.1, 0.5, 2e-4
    scale, l2 = lr / B, -lr * wc
    ref = stats_reference(d, scale, mmt)
    L, got = lib(), {}
    for one in (True, False):
        f = Ops(layout, f"{'rbm_update_stats' if one else 'rbm_update + rbm_stats_update'} ({V}, {H}, {B})")
        o = Cd1Views(f, d)
        if one:
            f.check(L.tnet_rbm_update_stats(*o.head(scale, mmt, l2, B), S()))
        else:
            f.check(L.tnet_rbm_update(o.V.ptr, o.V.dim, o.H.ptr, o.H.dim, o.W.ptr, o.W.dim, o.cW.ptr, o.cW.stride, scale,
                                      mmt, l2, S()))
            f.check(L.tnet_rbm_stats_update(o.V.ptr, o.V.dim, o.H.ptr, o.H.dim, B, o.vb.ptr, o.cvb.ptr, o.hb.ptr,
                                            o.chb.ptr, scale, mmt, o.st.ptr, S()))
        check_update(d, o, scale, mmt, l2, f.what)
        check_stats(d, ref, o.vb, o.cvb, o.hb, o.chb, o.st, f.what)
        got[one] = (o.raws(), o.st.numpy()[0][0::2].sum())
    for x, y, name in zip(got[True][0], got[False][0], ("W", "corrW", "vb", "cvb", "hb", "chb")):
        np.testing.assert_array_equal(x, y, err_msg=f"one launch vs two: {name} (whole buffers)")
    np.testing.assert_allclose(got[True][1], got[False][1], rtol=1e-12)


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
def test_rbm_update_stats_declines_views(layout):
    """B = 4097 (2 B > 8192 rows: the statistics blocks decline): TNET_ERR_UNSUPPORTED, every buffer bit-identical"""
    d = cd1_case(5, 3, 4097)
    f = Ops(layout, "rbm_update_stats B 4097")
    o = Cd1Views(f, d)
    f.refused(lib().tnet_rbm_update_stats(*o.head(0.1 / 4097, 0.5, -2e-5, 4097), S()))


def y_frame_violation(vy, c4):
    """the frame check of the gathered bunch: columns cols .. c4 - 1 of each row (the row padding up to the next
    multiple of 4 columns, which the header lets the gather fill) are exempt; every other frame word is checked"""
    raw = vy.raw()
    assert c4 <= vy.stride
    for r in range(vy.rows):
        w0 = (GUARD + r) * vy.stride + vy.c0
        raw[w0 + vy.cols: w0 + c4] = POISON
    return frame_violation(raw, vy.rows, vy.cols, vy.layout)


def assert_y_untouched(vy):
    assert (vy.raw() == POISON).all(), "the gather's destination was written by a refused call"


@pytest.mark.parametrize("layout", GEMM_LAYOUTS)
@pytest.mark.parametrize("V,H,B", [(5, 3, 1), (33, 70, 17)])
def test_rbm_update_stats_gather_views(V, H, B, layout):
    """accepted where tnet_rbm_update_stats is (above) and, in tnet_rbm_update_stats_gather, y and x are 16-byte
    aligned with strides that are multiples of 4 holding roundup4(cols), and 16 CUs are left beside the update's
    tiles.  One launch == tnet_rbm_update_stats + tnet_gather_bunch on views of the same layout; the gather may fill
    y's row padding up to roundup4(V) columns and writes nothing beyond; y overlapping V: TNET_ERR_ARG; y in `odd`:
    TNET_ERR_UNSUPPORTED; both with every buffer bit-identical"""
    d = cd1_case(V, H, B)
    lr, mmt, wc = 0.1, 0.5, 2e-4
    scale, l2 = lr / B, -lr * wc
    ref = stats_reference(d, scale, mmt)
    rng = np.random.default_rng(V + B)
    cache = rng.standard_normal((3 * B + 5, V)).astype(np.float32)
    perm = rng.permutation(cache.shape[0]).astype(np.int32)[:B]
    lab = rng.integers(0, 40, cache.shape[0]).astype(np.int32)
    c4 = (V + 3) & ~3
    L, got = lib(), {}
    for one in (True, False):
        f = Ops(layout, f"{'rbm_update_stats_gather' if one else 'rbm_update_stats + gather_bunch'} ({V}, {H}, {B})")
        o = Cd1Views(f, d)
        vC, vL, vP = f.inp(cache), f.inp(lab, np.int32), f.inp(perm, np.int32)
        vy = PoisonView.empty(B, V, layout)  # (not among f's outputs: its frame check is y_frame_violation)
        vlo = f.out(1, B, np.int32)
        gargs = [vy.ptr, vC.ptr, vlo.ptr, vL.ptr, vP.ptr, vy.dim, vC.dim]
        if one:
            # the destination inside V: refused before anything runs
            inside = MatrixDim(B, V, o.V.stride)
            f.refused(L.tnet_rbm_update_stats_gather(*o.head(scale, mmt, l2, B), o.V.ptr, vC.ptr, vlo.ptr, vL.ptr, vP.ptr,
                                                     inside, vC.dim, S()), TNET_ERR_ARG)
            assert_y_untouched(vy)
            # a destination whose stride holds no 16-byte pieces: declined
            g = Ops("odd", f.what + ": y in odd")
            vodd = g.out(B, V)
            rc = L.tnet_rbm_update_stats_gather(*o.head(scale, mmt, l2, B), vodd.ptr, vC.ptr, vlo.ptr, vL.ptr, vP.ptr,
                                                vodd.dim, vC.dim, S())
            f.refused(rc)
            g.refused(rc)
            assert_y_untouched(vy)
            f.check(L.tnet_rbm_update_stats_gather(*o.head(scale, mmt, l2, B), *gargs, S()))
            msg = y_frame_violation(vy, c4)
            assert msg is None, f"{f.what}: y beyond its row padding up to {c4} columns: {msg}"
        else:
            f.check(L.tnet_rbm_update_stats(*o.head(scale, mmt, l2, B), S()), partial=(vlo,))
            f.check(L.tnet_gather_bunch(*gargs, S()))
            msg = frame_violation(vy.raw(), vy.rows, vy.cols, vy.layout)
            assert msg is None, f"{f.what}: y: {msg}"  # tnet_gather_bunch has no licence for the padding
        check_update(d, o, scale, mmt, l2, f.what)
        check_stats(d, ref, o.vb, o.cvb, o.hb, o.chb, o.st, f.what)
        np.testing.assert_array_equal(vy.numpy(), cache[perm], err_msg=f.what + " gathered rows")
        np.testing.assert_array_equal(vlo.numpy()[0], lab[perm], err_msg=f.what + " gathered ids")
        got[one] = (o.raws(), o.st.numpy()[0][0::2].sum())
    for x, y, name in zip(got[True][0], got[False][0], ("W", "corrW", "vb", "cvb", "hb", "chb")):
        np.testing.assert_array_equal(x, y, err_msg=f"one launch vs separate calls: {name} (whole buffers)")
    np.testing.assert_allclose(got[True][1], got[False][1], rtol=1e-12)
