"""The recurrent trainer's look-ahead launches (tnet_rnn_out_bwd_update_ahead, tnet_rnn_out_full_ahead; gemv.hip
RnnAhead / RnnCorr, CuRecurrentTrainer::TrainFrameFused) at kernel level, on one frame boundary built from a seed.

Frame t has finished its forward (h, z, the softmax pairs).  The trainer's next two launches are
  1. tnet_rnn_out_bwd_update_ahead: the output layer's backprop + SGD, the recurrent bias copy, and the look-ahead
     of frame t+1 -- the split-K partials of [x_{t+1}, h_t] W_t, the dots [x_{t+1}, h_t] . h_i with the ring rows the
     pending update reads, and the push of [x_{t+1}, h_t] into the ring;
  2. (after the BPTT steps, here a given D) tnet_rnn_out_full_ahead: h_{t+1} from the look-ahead partials corrected
     to the updated weights, z and the softmax pairs, and the pending update of W itself.

What the kernel comments claim bit for bit ("the arithmetic and k order of ...") is asserted with
assert_array_equal against the existing entry points on copies of the same inputs; what they claim "up to fp32
reassociation" is asserted against numpy in fp64, with test_rnn_out_full's tolerances and with the forward error
bound of the sums (see _h_bound).  Every matrix with a leading dimension is allocated wider than its logical width
and the padding columns, filled with a sentinel, must come back untouched.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tnet_amd import DeviceArray, synchronize  # noqa: E402
from tnet_amd._lib import check, lib  # noqa: E402

SENT = -12345.678  # padding / "must not be written" filler: far outside every operand's range
UNSUPPORTED = -4   # TNET_ERR_UNSUPPORTED
U = 2.0 ** -24     # fp32 unit roundoff
LR, SCALE, L2 = float(np.float32(0.02)), -0.03, -1e-5


def S():
    return lib().tnet_stream()


def _dev(a, ld=None, dtype=np.float32):
    """a [rows x cols] on the device with leading dimension ld (default cols), the padding columns = SENT"""
    a = np.atleast_2d(np.asarray(a, dtype))
    ld = a.shape[1] if ld is None else ld
    d = DeviceArray(a.shape[0], a.shape[1], dtype, stride=ld, zero=False)
    host = np.full((a.shape[0], ld), SENT, dtype)
    host[:, : a.shape[1]] = a
    check(lib().tnet_memcpy_h2d(d.ptr, host.ctypes.data, host.nbytes), "h2d")
    return d


def _raw(d):
    """the whole allocation [rows x stride], padding included"""
    host = np.empty((d.rows, d.stride), d.dtype)
    check(lib().tnet_memcpy_d2h(host.ctypes.data, d.ptr, host.nbytes), "d2h")
    return host


def _from_raw(d):
    """a copy of the whole allocation, padding included"""
    c = DeviceArray(d.rows, d.cols, d.dtype, stride=d.stride, zero=False)
    host = _raw(d)
    check(lib().tnet_memcpy_h2d(c.ptr, host.ctypes.data, host.nbytes), "h2d")
    return c


def _ptr(d):
    return d.ptr if d is not None else None


class Boundary:
    """The state between frame t's forward and its second launch.  Leading dimensions: W and D H + 4 (multiples of
    4, as the update blocks' 16-byte accesses need), the ring K + 3, Wo and its momentum N + 4."""

    def __init__(self, nIn, H, N, steps, R, head, mmt, wc, seed=0, ldw=None, ldd=None):
        rng = np.random.default_rng([nIn, H, N, steps, R, head, seed])
        self.nIn, self.H, self.N, self.K = nIn, H, N, nIn + H
        self.steps, self.R, self.head, self.mmt, self.wc = steps, R, head, mmt, wc
        self.push = (head + R - 1) % R
        K = self.K
        self.hs, self.G = -(-K // 64), -(-N // 64)
        f = np.float32
        ldw = H + 4 if ldw is None else ldw
        ldd = H + 4 if ldd is None else ldd
        self.W = _dev((rng.standard_normal((K, H)) / np.sqrt(K)).astype(f), ldw)
        self.b = _dev((0.5 * rng.standard_normal(H)).astype(f))
        self.cb = _dev((0.01 * rng.standard_normal(H)).astype(f))
        hist = rng.standard_normal((R, K)).astype(f)
        hist[:, nIn:] = rng.random((R, H)).astype(f)  # history-like: the y part in (0, 1)
        self.hist = _dev(hist, K + 3)
        self.D = _dev((0.1 * rng.standard_normal((steps, H))).astype(f), ldd)
        self.Wo = _dev((0.05 * rng.standard_normal((H, N))).astype(f), N + 4)
        self.bo = _dev(rng.standard_normal(N).astype(f))
        self.corrWo = _dev((0.01 * rng.standard_normal((H, N))).astype(f), N + 4) if mmt else None
        self.corr_bo = _dev((0.01 * rng.standard_normal(N)).astype(f)) if mmt else None
        self.x_next = _dev(rng.standard_normal(nIn).astype(f))
        self.bnext = _dev((0.5 * rng.standard_normal(H)).astype(f))
        self.cbnext = _dev((0.01 * rng.standard_normal(H)).astype(f))
        t = -1 if N == 300 else (7 * H + 3) % N  # one unlabeled frame among the shapes
        self.label = DeviceArray.vector(np.array([t], np.int32))
        # frame t's forward on the existing kernels: h, z, the softmax pairs (ring row `head` = [x_t, y_{t-1}])
        self.h, self.z = DeviceArray(1, H, stride=H), DeviceArray(1, N, stride=N)
        self.smx = DeviceArray(1, 2 * self.G, np.float64, stride=2 * self.G)
        row = self.hist.ptr + head * self.hist.stride * 4
        part = DeviceArray(self.hs, H, stride=H)
        if H <= 2048:  # (past tnet_rnn_out_full's limit only the refusals are tested: h, z and the pairs stay zero)
            check(lib().tnet_gemv_rowvec_partial(row, nIn, row + 4 * nIn, H, None, self.W.ptr, self.W.stride, H,
                                                 part.ptr, S()))
            check(lib().tnet_rnn_out_full(part.ptr, self.hs, self.b.ptr, self.h.ptr, H, self.Wo.ptr, self.Wo.stride, N,
                                          self.bo.ptr, self.z.ptr, self.smx.ptr, S()))
        # outputs of the two launches, prefilled with the sentinel
        self.partial = _dev(np.full((self.hs, H), SENT, f))
        self.dpart = _dev(np.full((self.hs, 16), SENT, f))
        self.e, self.eo = _dev(np.full(N, SENT, f)), _dev(np.full(H, SENT, f))
        self.stats = DeviceArray(1, 1024, np.float64, stride=1024)
        self.key = DeviceArray.vector(np.zeros(2, np.int32))  # one 64-bit key
        synchronize()

    def bwd_update_ahead(self, bias_copy=True, look=True, steps=None, R=None, pairs=None, N=None):
        """launch 1, the trainer's argument order (curecurrent.cpp TrainFrameFused); d goes to D's row 0"""
        return lib().tnet_rnn_out_bwd_update_ahead(
            self.z.ptr, self.smx.ptr, self.G if pairs is None else pairs, self.N if N is None else N, self.label.ptr,
            self.h.ptr, self.H, self.Wo.ptr, self.Wo.stride, _ptr(self.corrWo), self.N + 4, self.bo.ptr,
            _ptr(self.corr_bo), SCALE, self.mmt, L2, self.e.ptr, self.eo.ptr, self.D.ptr, self.stats.ptr, self.key.ptr,
            self.bnext.ptr if bias_copy else None, self.cbnext.ptr if bias_copy else None, self.b.ptr, self.cb.ptr,
            self.x_next.ptr if look else None, self.nIn, self.W.ptr, self.W.stride, self.partial.ptr, self.dpart.ptr,
            self.hist.ptr + self.push * self.hist.stride * 4, self.hist.ptr, self.hist.stride, self.head,
            self.R if R is None else R, self.steps if steps is None else steps, S())

    def full_ahead(self, out, H=None, N=None, steps=None, R=None, hslices=None, ldw=None, ldd=None):
        """launch 2 with pend = head; out = (h, z, smx, bnext, cbnext)"""
        h, z, smx, bnext, cbnext = out
        return lib().tnet_rnn_out_full_ahead(
            self.partial.ptr, self.hs if hslices is None else hslices, self.b.ptr, h.ptr, self.H if H is None else H,
            self.Wo.ptr, self.Wo.stride, self.N if N is None else N, self.bo.ptr, z.ptr, smx.ptr, self.dpart.ptr,
            self.D.ptr, self.D.stride if ldd is None else ldd, self.steps if steps is None else steps, LR, self.mmt,
            self.wc, self.cb.ptr, bnext.ptr, cbnext.ptr, self.W.ptr, self.W.stride if ldw is None else ldw, self.K,
            self.hist.ptr, self.hist.stride, self.head, self.R if R is None else R, S())

    def full_outputs(self):
        f = np.float32
        return (_dev(np.full(self.H, SENT, f)), _dev(np.full(self.N, SENT, f)),
                _dev(np.full(2 * self.G, SENT, np.float64), dtype=np.float64), _dev(np.full(self.H, SENT, f)),
                _dev(np.full(self.H, SENT, f)))


def _h_bound(st, v, W0, b1, dots, D, hslices):
    """|h_gpu - h_fp64| allowed by the forward error bound of the pre-activation's sums.

    a_c = b'_c + (1 - lr wc) sum_k v_k W_kc + sum_i (-lr dot_i) d_ic.  A sum evaluated in fp32 in any order with an
    add chain of at most n operations is off by at most n 2^-24 times the sum of the operands' magnitudes (Higham,
    Accuracy and Stability, 4.2), so |da| <= n 2^-24 (sum_k |v_k W_kc| + sum_i |lr dot_i d_ic| + |b'_c|) with
    n = 16 (a wave's k rows) + 4 (waves) + hslices + steps + 4 (weight cost, bias chain, final adds): the longest
    chain of either path.  The sigmoid is v_exp_f32 of the scaled argument and v_rcp_f32: the scaling's two roundings
    move the argument by <= 2 2^-24 |a| (added to da), the slope is <= 1/4, and exp + add + rcp cost <= 2 ulp of a
    value below 1 (2 2^-23)."""
    n = 16 + 4 + hslices + st.steps + 4
    mag = np.abs(v) @ np.abs(W0) + np.abs(LR * dots[:, None] * D).sum(0) + np.abs(b1)
    a = b1 + (1 - LR * st.wc) * (v @ W0) + ((-LR * dots)[:, None] * D).sum(0)
    da = n * U * mag + 2 * U * np.abs(a)
    return da / 4 + 2 * 2.0 ** -23


def _z_bound(h, dh, Wo, bo):
    """the same bound for z_c = bo_c + sum_k h_k Wo_kc: a lane's chain of ceil(H/16) rows, 16 wave sums, the bias;
    plus what the allowed error of h carries over"""
    n = -(-len(h) // 16) + 16 + 2
    return n * U * (h @ np.abs(Wo) + np.abs(bo)) + dh @ np.abs(Wo)


# (nIn, H, N): the smallest shapes that reach each branch of rnn_out_full_kernel / rnn_ahead_block
#   8, 64, 5        2 k-slices, one partial column block, N < 64
#   30, 68, 300     H % 64 != 0 with H % 4 = 0, K % 64 != 0, an unlabeled frame
#   600, 512, 135   18 slices: the second round of 16 partial slices, the dots' tail loop (q0 >= 16)
#   40, 516, 1025   the Wo reload loop (H > 512), rnn_out_bwd_kernel<4> (N > 1024) in its scalar form
#   8, 1028, 135    KPT = 2 with a 4-element second unit, 17 slices
#   40, 2048, 4096  both limits: 33 slices (third round), 64 softmax pairs, the register form of <4>
# (steps, R, head): R = steps + 1 as the trainer has it, once larger; head + i wraps in every one but (1, 2, 1)
CASES = [
    (8, 64, 5, 1, 2, 1, 0.0, 0.0),
    (8, 64, 5, 9, 10, 7, 0.5, 1e-4),
    (30, 68, 300, 5, 6, 4, 0.5, 1e-4),
    (30, 68, 300, 9, 10, 7, 0.0, 0.0),
    (30, 68, 300, 3, 7, 6, 0.5, 1e-4),
    (600, 512, 135, 9, 10, 7, 0.0, 0.0),
    (600, 512, 135, 5, 6, 4, 0.5, 1e-4),
    (40, 516, 1025, 9, 10, 7, 0.5, 1e-4),
    (40, 516, 1025, 3, 7, 6, 0.0, 0.0),
    (8, 1028, 135, 9, 10, 7, 0.0, 0.0),
    (8, 1028, 135, 1, 2, 1, 0.5, 1e-4),
    (40, 2048, 4096, 9, 10, 7, 0.5, 1e-4),
    (40, 2048, 4096, 5, 6, 4, 0.0, 0.0),
]


@pytest.mark.parametrize("nIn,H,N,steps,R,head,mmt,wc", CASES)
def test_rnn_ahead_frame_boundary(nIn, H, N, steps, R, head, mmt, wc):
    """Both look-ahead launches in the trainer's order on one frame boundary.

    Bit-identical (assert_array_equal): the output-layer side of launch 1 == tnet_rnn_out_bwd_update(train=1); the
    look-ahead partials == tnet_gemv_rowvec_partial([x_next, h], W_t); the pushed ring row == [x_next, h]; the
    bias copy; launch 2's W, bnext, cbnext == tnet_rnn_update's W, b, cb; every padding column, every other ring row,
    and the buffers a launch must not write.

    Against fp64: the dots within 8 2^-24 sum|v_k h_ik| (a product and a 6-step butterfly per slice; the slices are
    summed in fp64 here); h, z, and the softmax at test_rnn_out_full's tolerances (h rtol 1e-5 / atol 1e-6, z rtol
    1e-5 / atol 1e-5, y rtol 2e-5 / atol 1e-9) AND inside the forward bounds of _h_bound / _z_bound, for the
    look-ahead path and for the materialised chain (tnet_rnn_update -> tnet_gemv_rowvec_partial ->
    tnet_rnn_out_full) on the same inputs, so a failure says which path is off.

    Observed on MI355X, max over the cases of this table (error / allowance, look-ahead | materialised):
      h vs fixed tolerance   0.039 | 0.040     h vs forward bound   0.045 | 0.045
      z vs fixed tolerance   0.095 | 0.093     z vs forward bound   0.013 | 0.015
      dots vs their bound    0.12
    (every shape meets the fixed tolerances, so both are asserted)
    (per case: profiles/rnn_ahead_error_ratios.json)"""
    st = Boundary(nIn, H, N, steps, R, head, mmt, wc)
    K, hs, G = st.K, st.hs, st.G
    x_next, h_t = st.x_next.numpy().ravel(), st.h.numpy().ravel()
    row = np.concatenate([x_next, h_t])
    W0, hist0, b0, cb0 = _raw(st.W), _raw(st.hist), st.b.numpy(), st.cb.numpy()

    # ---- the existing output-layer launch on copies
    ref = dict(Wo=_from_raw(st.Wo), bo=_from_raw(st.bo), corrWo=_from_raw(st.corrWo) if mmt else None,
               corr_bo=_from_raw(st.corr_bo) if mmt else None, e=_from_raw(st.e), eo=_from_raw(st.eo),
               d=_dev(np.full(H, SENT, np.float32)), stats=DeviceArray(1, 1024, np.float64, stride=1024),
               key=DeviceArray.vector(np.zeros(2, np.int32)))
    check(lib().tnet_rnn_out_bwd_update(st.z.ptr, st.smx.ptr, G, N, st.label.ptr, st.h.ptr, H, ref["Wo"].ptr,
                                        ref["Wo"].stride, _ptr(ref["corrWo"]), N + 4, ref["bo"].ptr,
                                        _ptr(ref["corr_bo"]), SCALE, mmt, L2, None, ref["e"].ptr, ref["eo"].ptr,
                                        ref["d"].ptr, ref["stats"].ptr, ref["key"].ptr, 1, S()))
    part_ref = _dev(np.full((hs, H), SENT, np.float32))
    check(lib().tnet_gemv_rowvec_partial(st.x_next.ptr, nIn, st.h.ptr, H, None, st.W.ptr, st.W.stride, H,
                                         part_ref.ptr, S()))
    # ---- launch 1
    check(st.bwd_update_ahead())
    synchronize()
    for name in ("e", "eo", "Wo", "bo", "stats", "key") + (("corrWo", "corr_bo") if mmt else ()):
        np.testing.assert_array_equal(_raw(getattr(st, name)), _raw(ref[name]), err_msg=name)
    D = _raw(st.D)
    np.testing.assert_array_equal(D[0, :H], ref["d"].numpy().ravel(), err_msg="d")
    assert (D[:, H:] == np.float32(SENT)).all() and (_raw(st.Wo)[:, N:] == np.float32(SENT)).all()
    np.testing.assert_array_equal(_raw(st.partial), _raw(part_ref), err_msg="look-ahead partials")
    hist1 = _raw(st.hist)
    np.testing.assert_array_equal(hist1[st.push, :K], row, err_msg="pushed ring row")
    keep = np.ones_like(hist1, bool)
    keep[st.push, :K] = False
    np.testing.assert_array_equal(hist1[keep], hist0[keep], err_msg="ring rows / padding besides the push")
    np.testing.assert_array_equal(_raw(st.W), W0, err_msg="launch 1 must not write W")
    np.testing.assert_array_equal(st.b.numpy(), st.bnext.numpy(), err_msg="bias copy")
    np.testing.assert_array_equal(st.cb.numpy(), st.cbnext.numpy(), err_msg="bias momentum copy")
    dpart = _raw(st.dpart)
    assert (dpart[:, steps:] == np.float32(SENT)).all(), "dpart columns past `steps` written"
    v = row.astype(np.float64)
    ring = hist0[:, :K].astype(np.float64)
    hrows = np.stack([ring[(head + i) % R] for i in range(steps)])
    dots_ref = hrows @ v
    dots_err = np.abs(dpart[:, :steps].astype(np.float64).sum(0) - dots_ref)
    dots_bound = 8 * U * (np.abs(hrows) @ np.abs(v))
    r_dots = float((dots_err / dots_bound).max())

    # ---- the materialised chain on copies of the state launch 2 sees
    mW, mb, mcb = _from_raw(st.W), _from_raw(st.b), _from_raw(st.cb)
    b1_in, cb1_in = st.b.numpy(), st.cb.numpy()
    check(lib().tnet_rnn_update(mW.ptr, mW.stride, K, H, st.hist.ptr, st.hist.stride, head, R, st.D.ptr, st.D.stride,
                                steps, mb.ptr, mcb.ptr, LR, mmt, wc, S()))
    mpart = DeviceArray(hs, H, stride=H)
    check(lib().tnet_gemv_rowvec_partial(st.x_next.ptr, nIn, st.h.ptr, H, None, mW.ptr, mW.stride, H, mpart.ptr, S()))
    mh, mz, msmx = DeviceArray(1, H, stride=H), DeviceArray(1, N, stride=N), DeviceArray(1, 2 * G, np.float64,
                                                                                           stride=2 * G)
    check(lib().tnet_rnn_out_full(mpart.ptr, hs, mb.ptr, mh.ptr, H, st.Wo.ptr, st.Wo.stride, N, st.bo.ptr, mz.ptr,
                                  msmx.ptr, S()))
    # ---- launch 2
    out = st.full_outputs()
    Wo1, D1 = _raw(st.Wo), _raw(st.D)
    check(st.full_ahead(out))
    synchronize()
    h2, z2, smx2, bnext2, cbnext2 = (a.numpy().ravel() for a in out)
    np.testing.assert_array_equal(_raw(st.W), _raw(mW), err_msg="pending update of W (padding included)")
    assert (_raw(st.W)[:, H:] == np.float32(SENT)).all()
    np.testing.assert_array_equal(bnext2, mb.numpy().ravel(), err_msg="bnext")
    np.testing.assert_array_equal(cbnext2, mcb.numpy().ravel(), err_msg="cbnext")
    np.testing.assert_array_equal(st.b.numpy(), b1_in, err_msg="launch 2 must not write hb")
    np.testing.assert_array_equal(st.cb.numpy(), cb1_in, err_msg="launch 2 must not write cb")
    for name, before in (("hist", hist1), ("Wo", Wo1), ("D", D1), ("dpart", dpart)):
        np.testing.assert_array_equal(_raw(getattr(st, name)), before, err_msg=f"launch 2 must not write {name}")

    # ---- fp64: W_{t+1}, b' from the update formula (cuRecurrent.cc:88-153), h, z, softmax
    Dd = D1[:, :H].astype(np.float64)
    W64 = W0[:, :H].astype(np.float64)
    g = mmt * cb1_in.ravel().astype(np.float64) - LR * Dd.sum(0)
    b1 = b1_in.ravel().astype(np.float64) + g
    acc = -LR * (hrows.T @ Dd)
    W1 = W64 + (-LR * wc) * W64 + acc
    a = b1 + v @ W1
    hr = 1 / (1 + np.exp(-a))
    bo1 = st.bo.numpy().ravel().astype(np.float64)
    Wo64 = Wo1[:, :N].astype(np.float64)
    zr = bo1 + hr @ Wo64
    yr = np.exp(zr - zr.max())
    yr /= yr.sum()
    hb = _h_bound(st, v, W64, b1, dots_ref, Dd, hs)
    zb = _z_bound(hr, hb, Wo64, bo1)
    ratios = {"dots": r_dots}
    for path, hg, zg in (("ahead", h2, z2), ("materialised", mh.numpy().ravel(), mz.numpy().ravel())):
        eh, ez = np.abs(hg - hr), np.abs(zg - zr)
        ratios[path] = dict(h_fixed=float((eh / (1e-6 + 1e-5 * np.abs(hr))).max()), h_bound=float((eh / hb).max()),
                            z_fixed=float((ez / (1e-5 + 1e-5 * np.abs(zr))).max()), z_bound=float((ez / zb).max()))
    print("rnn_ahead ratios", (nIn, H, N, steps, R, head, mmt, wc), ratios)
    assert r_dots <= 1.0, f"dots off their bound: {r_dots}"
    for path in ("ahead", "materialised"):
        assert ratios[path]["h_bound"] <= 1.0 and ratios[path]["z_bound"] <= 1.0, (path, ratios[path])
    for path, hg, zg in (("ahead", h2, z2), ("materialised", mh.numpy().ravel(), mz.numpy().ravel())):
        np.testing.assert_allclose(hg, hr, rtol=1e-5, atol=1e-6, err_msg=path)
        np.testing.assert_allclose(zg, zr, rtol=1e-5, atol=1e-5, err_msg=path)
    # the softmax pairs of launch 2: the exact maximum of its z per 64 columns, the sum of exp(z - max) (fast_exp:
    # relative error <= 1e-6, kcommon.h), and through tnet_rnn_out_bwd_update (train = 0) the softmax itself
    for gidx in range(G):
        zc = z2[64 * gidx: 64 * gidx + 64]
        assert smx2[2 * gidx] == float(zc.max())
        np.testing.assert_allclose(smx2[2 * gidx + 1], np.exp(zc.astype(np.float64) - float(zc.max())).sum(),
                                   rtol=1e-5)
    y = DeviceArray(1, N, stride=N)
    check(lib().tnet_rnn_out_bwd_update(out[1].ptr, out[2].ptr, G, N, st.label.ptr, out[0].ptr, H, None, 0, None, 0,
                                        None, None, SCALE, 0.0, L2, y.ptr, None, None, None, None, None, 0, S()))
    np.testing.assert_allclose(y.numpy().ravel(), yr, rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize("nIn,H,N,steps,R,head", [(8, 64, 5, 1, 2, 1), (30, 68, 300, 5, 6, 4),
                                                   (8, 1028, 135, 9, 10, 7)])
def test_rnn_ahead_optional_parts(nIn, H, N, steps, R, head):
    """bnext = NULL: b and cb are untouched (the frame after a materialised forward has nothing to copy);
    x_next = NULL: partial, dpart and the ring are untouched (an utterance's last frame looks nowhere); in both the
    output-layer side is still tnet_rnn_out_bwd_update's, bit for bit"""
    for bias_copy, look in ((False, True), (True, False), (False, False)):
        st = Boundary(nIn, H, N, steps, R, head, 0.5, 1e-4, seed=1)
        ref = dict(Wo=_from_raw(st.Wo), bo=_from_raw(st.bo), corrWo=_from_raw(st.corrWo),
                   corr_bo=_from_raw(st.corr_bo), e=_from_raw(st.e), eo=_from_raw(st.eo))
        d = _dev(np.full(H, SENT, np.float32))
        stats, key = DeviceArray(1, 1024, np.float64, stride=1024), DeviceArray.vector(np.zeros(2, np.int32))
        check(lib().tnet_rnn_out_bwd_update(st.z.ptr, st.smx.ptr, st.G, N, st.label.ptr, st.h.ptr, H, ref["Wo"].ptr,
                                            ref["Wo"].stride, ref["corrWo"].ptr, N + 4, ref["bo"].ptr,
                                            ref["corr_bo"].ptr, SCALE, 0.5, L2, None, ref["e"].ptr, ref["eo"].ptr, d.ptr,
                                            stats.ptr, key.ptr, 1, S()))
        b0, cb0, hist0, part0, dpart0 = (_raw(a) for a in (st.b, st.cb, st.hist, st.partial, st.dpart))
        check(st.bwd_update_ahead(bias_copy=bias_copy, look=look))
        synchronize()
        for name in ref:
            np.testing.assert_array_equal(_raw(getattr(st, name)), _raw(ref[name]), err_msg=name)
        np.testing.assert_array_equal(_raw(st.D)[0, :H], d.numpy().ravel())
        np.testing.assert_array_equal(_raw(st.key), _raw(key))
        np.testing.assert_array_equal(_raw(st.stats), _raw(stats))
        if bias_copy:
            np.testing.assert_array_equal(_raw(st.b), _raw(st.bnext))
            np.testing.assert_array_equal(_raw(st.cb), _raw(st.cbnext))
        else:
            np.testing.assert_array_equal(_raw(st.b), b0)
            np.testing.assert_array_equal(_raw(st.cb), cb0)
        if look:
            np.testing.assert_array_equal(_raw(st.hist)[st.push, : st.K],
                                          np.concatenate([st.x_next.numpy().ravel(), st.h.numpy().ravel()]))
            assert not (_raw(st.partial) == np.float32(SENT)).any()
        else:
            np.testing.assert_array_equal(_raw(st.hist), hist0)
            np.testing.assert_array_equal(_raw(st.partial), part0)
            np.testing.assert_array_equal(_raw(st.dpart), dpart0)


def test_rnn_ahead_refusals():
    """TNET_ERR_UNSUPPORTED (-4), nothing launched, every output as it was: H > 2048, N > 4096 (65 pairs), steps
    > 9, steps >= R, H % 4 != 0, ldd or ldw no multiple of 4, hslices != ceil(rows / 64)"""
    def snapshot(st, out):
        return [_raw(a) for a in (st.W, st.b, st.cb, st.hist, st.D, st.Wo, st.bo, st.partial, st.dpart, st.e, st.eo,
                                  st.stats, st.key) + tuple(out)]

    def refused(st, out, rc, what):
        synchronize()
        assert rc == UNSUPPORTED, (what, rc)
        for before, after in zip(st.snap, snapshot(st, out)):
            np.testing.assert_array_equal(after, before, err_msg=what)

    def make(nIn, H, N, steps, R, head, **kw):
        st = Boundary(nIn, H, N, steps, R, head, 0.0, 0.0, seed=2, **kw)
        out = st.full_outputs()
        st.snap = snapshot(st, out)
        return st, out

    st, out = make(8, 64, 5, 3, 4, 1)
    refused(st, out, st.full_ahead(out, steps=4), "full_ahead steps = R")
    refused(st, out, st.full_ahead(out, hslices=st.hs + 1), "full_ahead hslices + 1")
    refused(st, out, st.full_ahead(out, hslices=st.hs - 1), "full_ahead hslices - 1")
    refused(st, out, st.bwd_update_ahead(steps=4), "bwd_update_ahead steps = R")
    refused(st, out, st.bwd_update_ahead(steps=10, R=12), "bwd_update_ahead steps = 10")
    # (65 pairs stand for N = 4097: the pair count is what the launch is refused on, before anything is read)
    refused(st, out, st.bwd_update_ahead(pairs=65), "bwd_update_ahead 65 pairs")
    st, out = make(8, 64, 5, 10, 12, 1)
    refused(st, out, st.full_ahead(out), "full_ahead steps = 10")
    st, out = make(8, 64, 5, 3, 4, 1, ldw=66)
    refused(st, out, st.full_ahead(out), "full_ahead ldw % 4")
    st, out = make(8, 64, 5, 3, 4, 1, ldd=70)
    refused(st, out, st.full_ahead(out), "full_ahead ldd % 4")
    st, out = make(6, 70, 5, 3, 4, 1, ldw=72, ldd=72)
    refused(st, out, st.full_ahead(out), "full_ahead H = 70")
    st, out = make(8, 2052, 5, 3, 4, 1)
    refused(st, out, st.full_ahead(out), "full_ahead H = 2052")
    # N = 4097 on a state built at N = 4096 (the forward kernels refuse 4097 too): Wo's leading dimension, 4100,
    # covers it, and nothing may be read or written before the refusal
    st, out = make(8, 64, 4096, 3, 4, 1)
    refused(st, out, st.full_ahead(out, N=4097), "full_ahead N = 4097")
    refused(st, out, st.bwd_update_ahead(N=4097, pairs=65), "bwd_update_ahead N = 4097")
