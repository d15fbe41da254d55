"""The TRecurrentCu single-frame chain (gemv.hip, 19 entry points) on caller-owned views.

tests/test_gpu_rnn.py and tests/test_gpu_rnn_ahead.py hand these kernels DeviceArrays: an allocation base, a stride
of 64k floats, zero padding.  Here every matrix operand (W, Wo, corrWo, the history ring, D) is a PoisonView
(tests/kernel_views.py), every flat operand a 1 x n view of exactly the element count include/tnet_kernels.h states
(partial ceil(K/64) x N, opart ceil(H/64) x N, dpart ceil(K/64) x 16, smx 2 ceil(N/256) or 2 ceil(N/64) doubles,
vout K0 + K1, one 64-bit key per frame), and every word around them a quiet-NaN pattern.  After every call
  * every operand's frame is intact (Ops.check: guard rows, the band before column 0, the padding, as uint32),
  * every pure input's buffer is bit-identical to what was uploaded (they carry POISON_INPUT),
  * no output interior holds a NaN (outputs start as poison: every element must have been written),
  * the values match a float64 numpy restatement written here, at the bounds the existing tests give each quantity
    (test_gpu_rnn.py: h 1e-5 / 1e-6, z 1e-5 / 1e-5, y 2e-5 / 1e-9, e 2e-5 / 1e-8, e_out and d 1e-4 / 1e-6, Wo and bo
    1e-5 / 1e-7, xent 1e-5 / 1e-6 as rtol / atol, the key exact; test_affine_bwd_update_row: e_out, d 1e-5 / 1e-6, W,
    b and the momentum 1e-6 / 1e-7; test_gemv_rowvec 1e-5 / 1e-5, _cat 1e-5 / 1e-6, test_gemv_rows 1e-5 / 1e-5;
    test_gpu_rnn_ahead.py: h, z as above and inside _h_bound / _z_bound, the dots within 8 2^-24 sum |v h|), and a
    plain dot product without a bound of its own (the split-K partials) at test_gpu_kernels.py's
    |got - ref| <= 2e-5 (|a| . |b|) + 1e-6.

Layouts.  tight and offset: every entry point.  odd (a 4-byte aligned base, a stride that is no multiple of 4): every
entry point but tnet_rnn_out_full_ahead, because, as read in gemv.hip, every other kernel either makes scalar
accesses only (gemv_rowvec_partial_k, gemv_rowvec_final, gemv_softmax_xent_final, rnn_update_kernel,
affine_update_row_kernel, rnn_out_partial_kernel, rnn_out_stats_kernel, rnn_out_full_kernel without RnnCorr,
rnn_ahead_block, argmax_correct_kernel) or guards its 16-byte path on n % 4, ld % 4 and the pointers' alignment
(gemv_rows_kernel, affine_bwd_update_row_kernel, rnn_out_bwd_kernel's `vec`), and no header comment asks for more.
tnet_rnn_out_full_ahead's update blocks load W and D as 16-byte vectors; its host code answers a misaligned W or D,
or an ldw / ldd off 4, with TNET_ERR_UNSUPPORTED before any launch: the odd case asserts that status and that every
buffer is bit-identical.  mixed (matrices in `offset`, vectors in `odd`), for the three guarded kernels: n % 4 == 0 and
ld % 4 == 0 with a misaligned e / x / z -- the guard's pointer term alone decides.  The 8-byte operands (smx, stats,
keys) are 8-byte aligned in every layout (`offset` where the floats are odd): they are targets of 64-bit atomics.

Paths reached, by the host code's conditions (gemv.hip):
  rnn_out_bwd_kernel<4> for N > 1024 (tnet_rnn_out_bwd_update: wide = N > 1024); there vec && n_out <= NP * STEP
  = 4096 is the register form (N = 1028, tight / offset), N = 4100 with vec the `c += STEP` loop, N = 1025 / 5001
  (N % 4 != 0) and every odd / mixed layout the scalar loop; N = 16384 is pairs = 64.
  gemv_rows_kernel: n = 1024 the register form, 1028 the loop, 13 and every odd / mixed layout the scalar loop.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from kernel_views import POISON, POISON_INPUT, PoisonView, assert_frame_untouched, assert_unchanged  # noqa: E402
from test_gpu_rnn_ahead import _h_bound, _z_bound  # noqa: E402
from tnet_amd._lib import lib  # noqa: E402

TNET_OK, TNET_ERR_ARG, TNET_ERR_UNSUPPORTED = 0, -1, -4  # include/tnet_kernels.h
U = 2.0 ** -24
FLT_MIN = 1.1754944e-38
LAYOUTS = ["tight", "offset", "odd"]
GUARDED_LAYOUTS = LAYOUTS + ["mixed"]  # for gemv_rows, affine_bwd_update_row, rnn_out_bwd


def S():
    return lib().tnet_stream()


def cdiv(a, b):
    return -(-a // b)


def P(v):
    return v.ptr if v is not None else None


class Ops:
    """the operands of one call or one chain of calls.  inp: a pure input (POISON_INPUT around, bit-identical
    afterwards); out: an output (poison inside too: must come out without NaN); io: in place; keep: handed to the call
    but to be left wholly unchanged.  Matrices take the layout, vectors the vector layout (they differ in `mixed`),
    8-byte operands `offset` where that would be odd."""

    def __init__(self, layout, what):
        self.what = what
        self.mat, self.vec_layout = ("offset", "odd") if layout == "mixed" else (layout, layout)
        self.ins, self.outs, self.kept = [], [], []

    def _layout(self, rows, dtype):
        lay = self.vec_layout if rows == 1 else self.mat
        return "offset" if np.dtype(dtype).itemsize == 8 and lay == "odd" else lay

    def inp(self, a, dtype=np.float32):
        a = np.atleast_2d(np.asarray(a))
        v = PoisonView(a, self._layout(a.shape[0], dtype), dtype=dtype, poison=POISON_INPUT)
        self.ins.append(v)
        return v

    def out(self, rows, cols, dtype=np.float32):
        v = PoisonView.empty(rows, cols, self._layout(rows, dtype), dtype)
        self.outs.append(v)
        return v

    def io(self, a, dtype=np.float32):
        a = np.atleast_2d(np.asarray(a))
        v = PoisonView(a, self._layout(a.shape[0], dtype), dtype=dtype)
        self.outs.append(v)
        return v

    def keep(self, a=None, rows=1, cols=None, dtype=np.float32):
        if a is not None:
            a = np.atleast_2d(np.asarray(a))
            rows, cols = a.shape
        v = PoisonView(a, self._layout(rows, dtype), rows, cols, dtype)
        self.kept.append(v)
        return v

    def check(self, status, expect=TNET_OK, partial=()):
        """after a call: status; frames of outputs / in-place operands intact and (but for those in `partial`, which
        the caller inspects) no NaN inside; pure inputs and kept operands bit-identical"""
        assert status == expect, f"{self.what}: status {status}, expected {expect}"
        for k, v in enumerate(self.outs):
            raw = v.raw()
            assert_frame_untouched(v, f"{self.what}: output {k} ({v.rows} x {v.cols})", raw=raw)
            if v.dtype.kind == "f" and not any(v is p for p in partial):
                a = raw[v._index].view(v.dtype)
                assert not np.isnan(a).any(), f"{self.what}: output {k} ({v.rows} x {v.cols}): " \
                                              f"{int(np.isnan(a).sum())} NaN, first at {np.flatnonzero(np.isnan(a))[0]}"
        for k, v in enumerate(self.ins + self.kept):
            assert_unchanged(v, v.initial, f"{self.what}: input / kept operand {k} ({v.rows} x {v.cols})")

    def refused(self, status, expect=TNET_ERR_UNSUPPORTED, before=None):
        """nothing launched: every operand's whole buffer as it was (`before`: raws taken before the call, for
        operands an earlier call of the chain has written)"""
        assert status == expect, f"{self.what}: status {status}, expected {expect}"
        for k, v in enumerate(self.ins + self.kept + self.outs):
            ref = v.initial if before is None or id(v) not in before else before[id(v)]
            assert_unchanged(v, ref, f"{self.what}: operand {k} ({v.rows} x {v.cols}) after a refusal")

    def snapshot(self):
        return {id(v): v.raw() for v in self.ins + self.kept + self.outs}


def close(got, ref, rtol, atol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, tol = np.abs(got - ref), atol + rtol * np.abs(ref)
    bad = ~(err <= tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} element(s) off, worst {err[bad].max():.3e} at " \
                          f"{np.argwhere(bad)[0]} (tolerance there {tol[bad][0]:.3e})"


def within(got, ref, tol, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    tol = np.broadcast_to(tol, err.shape)
    bad = ~(err <= tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} element(s) off, worst {err[bad].max():.3e} at " \
                          f"{np.argwhere(bad)[0]} (tolerance there {tol[bad][0]:.3e})"


def rnd(shape, seed, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def slice_partials(v, W):
    """fp64 split-K partials of v W over 64-row slices and their magnitudes |v| . |W|"""
    K = len(v)
    v, W = v.astype(np.float64), W.astype(np.float64)
    idx = [slice(k, min(K, k + 64)) for k in range(0, K, 64)]
    return (np.stack([v[s] @ W[s] for s in idx]), np.stack([np.abs(v[s]) @ np.abs(W[s]) for s in idx]))


def frozen(**d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return SimpleNamespace(**d)


# ------------------------------------------------------------------------------------------------------------------
# tnet_gemv_rowvec, _cat, _partial
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rowvec_case(K, N):
    v, W, b = rnd(K, 100 + K), rnd((K, N), 200 + N, 0.05), rnd(N, 300 + N)
    part, mag = slice_partials(v, W)
    return frozen(v=v, W=W, b=b, part=part, mag=mag, a=b + v.astype(np.float64) @ W)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("K,N", [(1, 1), (64, 64), (65, 63), (130, 68)])
def test_gemv_rowvec_family_views(K, N, layout):
    """one slice, one full slice and column block, a slice tail with N off 64, three slices and two column blocks.
    K split as K0 = 0, K1 = 0 and both non-zero (the empty half's pointer NULL); vout NULL and an exact K-word
    vector; the workspace exactly tnet_gemv_workspace(K, N) bytes, poison beyond"""
    d = rowvec_case(K, N)
    L, slices = lib(), cdiv(K, 64)
    assert L.tnet_gemv_workspace(K, N) == 4 * slices * N
    for act in (0, 1):
        f = Ops(layout, f"gemv_rowvec act {act}")
        v, W, b, y, ws = f.inp(d.v), f.inp(d.W), f.inp(d.b), f.out(1, N), f.out(1, slices * N)
        f.check(L.tnet_gemv_rowvec(v.ptr, K, W.ptr, W.stride, b.ptr, y.ptr, N, act, ws.ptr, S()))
        close(y.numpy()[0], sigmoid(d.a) if act else d.a, 1e-5, 1e-5, f.what)
        within(ws.numpy().reshape(slices, N), d.part, 2e-5 * d.mag + 1e-6, f.what + " workspace partials")
    splits = sorted({0, K, K // 2} - ({K // 2} if K < 2 else set()))
    for K0 in splits:
        K1 = K - K0
        for with_vout in (False, True):
            f = Ops(layout, f"gemv_rowvec_cat K0 {K0} K1 {K1} vout {with_vout}")
            v0 = f.inp(d.v[:K0]) if K0 else None
            v1 = f.inp(d.v[K0:]) if K1 else None
            W, b, y, ws = f.inp(d.W), f.inp(d.b), f.out(1, N), f.out(1, slices * N)
            vout = f.out(1, K) if with_vout else None
            f.check(L.tnet_gemv_rowvec_cat(P(v0), K0, P(v1), K1, P(vout), W.ptr, W.stride, b.ptr, y.ptr, N, 1, ws.ptr,
                                           S()))
            close(y.numpy()[0], sigmoid(d.a), 1e-5, 1e-6, f.what)
            if vout:
                np.testing.assert_array_equal(vout.numpy()[0], d.v, err_msg=f.what + " vout")
            f = Ops(layout, f"gemv_rowvec_partial K0 {K0} K1 {K1} vout {with_vout}")
            v0 = f.inp(d.v[:K0]) if K0 else None
            v1 = f.inp(d.v[K0:]) if K1 else None
            W, part = f.inp(d.W), f.out(1, slices * N)
            vout = f.out(1, K) if with_vout else None
            f.check(L.tnet_gemv_rowvec_partial(P(v0), K0, P(v1), K1, P(vout), W.ptr, W.stride, N, part.ptr, S()))
            within(part.numpy().reshape(slices, N), d.part, 2e-5 * d.mag + 1e-6, f.what)
            if vout:
                np.testing.assert_array_equal(vout.numpy()[0], d.v, err_msg=f.what + " vout")


# ------------------------------------------------------------------------------------------------------------------
# tnet_gemv_rows
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", GUARDED_LAYOUTS)
@pytest.mark.parametrize("nrows", [1, 7])
@pytest.mark.parametrize("n", [0, 13, 68, 1024, 1028])
def test_gemv_rows_views(n, nrows, layout):
    """r0 = 2 and one more row below: the rows around [r0, r0 + nrows) are live data (1e30: one of them in a sum
    shows) that is neither read into y nor written.  n = 13 scalar, 68 / 1024 the register form, 1028 the loop (tight,
    offset); in odd (ld % 4 != 0) and mixed (W aligned with ld % 4 == 0, x misaligned) n % 4 == 0 takes the scalar
    loop.  n = 0: y = beta y, nothing read (the register form's clamp n - 4 would lie before the row)."""
    r0 = 2
    W = rnd((r0 + nrows + 1, n), 400 + n)
    W[:r0], W[r0 + nrows:] = 1e30, 1e30
    x, y0, s = rnd(n, 401 + n), rnd(nrows, 402), np.random.default_rng(403).random(nrows).astype(np.float32)
    dot = W[r0:r0 + nrows].astype(np.float64) @ x
    for beta, with_s in ((0.0, False), (0.0, True), (0.5, True), (0.5, False)):
        f = Ops(layout, f"gemv_rows n {n} nrows {nrows} beta {beta} s {with_s}")
        if n:
            vW, vx = f.inp(W), f.inp(x)
        else:  # no columns: a 1-column view whose column is not part of the operand
            vW, vx = f.keep(rows=r0 + nrows + 1, cols=1), f.keep(rows=1, cols=1)
        vy = f.io(y0) if beta else f.out(1, nrows)
        vs = f.inp(s) if with_s else None
        if layout == "mixed" and n and n % 4 == 0:
            assert vW.ptr % 16 == 0 and vW.stride % 4 == 0 and vx.ptr % 16 != 0
        f.check(lib().tnet_gemv_rows(vW.ptr, vW.stride, r0, nrows, n, vx.ptr, vy.ptr, beta, P(vs), S()))
        ref = beta * y0 + dot
        close(vy.numpy()[0], ref * s * (1 - s) if with_s else ref, 1e-5, 1e-5, f.what)


# ------------------------------------------------------------------------------------------------------------------
# tnet_rnn_update, tnet_gemv_rowvec_partial_update
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mmt,wc", [(0.0, 0.0), (0.5, 1e-4)])
@pytest.mark.parametrize("steps", [1, 8, 9])
@pytest.mark.parametrize("nIn,H", [(8, 64), (30, 68)])
def test_rnn_update_views(nIn, H, steps, mmt, wc, layout):
    """steps 1, 8 (one full batch of rnn_update_kernel), 9 (a second batch; GV_UPD_MAX of the folded form);
    R = steps + 1 and head = R - 1, so every step but the first wraps the ring.  hist and D are pure inputs of
    tnet_rnn_update; the folded form pushes [x, y] into the ring row the update does not read: an output of exactly K
    words, every other ring word unchanged.  Folded == tnet_rnn_update then tnet_gemv_rowvec_partial bit for bit on
    views of the same layout; W, b, cb against fp64 at the output chain's parameter bound (rtol 1e-5, atol 1e-7)."""
    K, R = nIn + H, steps + 1
    head = R - 1
    push = (head + R - 1) % R
    lr = float(np.float32(0.02))
    W, b, cb = rnd((K, H), 500 + H, 0.05), rnd(H, 501), rnd(H, 502, 0.01)
    hist, D = rnd((R, K), 503 + steps), rnd((steps, H), 504 + steps, 0.1)
    x, yp = rnd(nIn, 505), np.random.default_rng(506).random(H).astype(np.float32)
    L, slices = lib(), cdiv(K, 64)
    hrows = np.stack([hist[(head + i) % R] for i in range(steps)]).astype(np.float64)
    W64, D64 = W.astype(np.float64), D.astype(np.float64)
    Wr = W64 + (-lr * wc) * W64 + (-lr) * (hrows.T @ D64)
    cbr = mmt * cb.astype(np.float64) - lr * D64.sum(0)
    got = {}
    for fused in (False, True):
        f = Ops(layout, f"{'gemv_rowvec_partial_update' if fused else 'rnn_update + gemv_rowvec_partial'}")
        vW, vb, vcb, vD = f.io(W), f.io(b), f.io(cb), f.inp(D)
        vh = f.io(hist)
        vx, vy, part = f.inp(x), f.inp(yp), f.out(1, slices * H)
        row = vh.ptr + 4 * push * vh.stride
        if fused:
            f.check(L.tnet_gemv_rowvec_partial_update(vx.ptr, nIn, vy.ptr, H, row, vW.ptr, vW.stride, H, part.ptr, vh.ptr,
                                                      vh.stride, head, R, vD.ptr, vD.stride, steps, vb.ptr, vcb.ptr, lr,
                                                      mmt, wc, S()))
        else:
            f.check(L.tnet_rnn_update(vW.ptr, vW.stride, K, H, vh.ptr, vh.stride, head, R, vD.ptr, vD.stride, steps,
                                      vb.ptr, vcb.ptr, lr, mmt, wc, S()), partial=(part,))
            assert_unchanged(vh, vh.initial, f.what + ": the ring is a pure input of tnet_rnn_update")
            f.check(L.tnet_gemv_rowvec_partial(vx.ptr, nIn, vy.ptr, H, row, vW.ptr, vW.stride, H, part.ptr, S()))
        got[fused] = [v.raw() for v in (vW, vb, vcb, part, vh)]
        ring = vh.numpy()
        np.testing.assert_array_equal(ring[push], np.concatenate([x, yp]), err_msg=f.what + " pushed row")
        keep = np.arange(R) != push
        np.testing.assert_array_equal(ring[keep], hist[keep], err_msg=f.what + " ring rows besides the push")
        close(vW.numpy(), Wr, 1e-5, 1e-7, f.what + " W")
        close(vcb.numpy()[0], cbr, 1e-5, 1e-7, f.what + " corr_b")
        close(vb.numpy()[0], b + cbr, 1e-5, 1e-7, f.what + " b")
        pr, mag = slice_partials(np.concatenate([x, yp]), vW.numpy())
        within(part.numpy().reshape(slices, H), pr, 2e-5 * mag + 1e-6, f.what + " partials")
    for a, c, name in zip(got[False], got[True], ("W", "b", "corr_b", "partial", "ring")):
        np.testing.assert_array_equal(a, c, err_msg=f"folded vs separate: {name} (whole buffers)")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rowvec_partial_update_refusals_views(layout):
    """steps = 10 (> GV_UPD_MAX) and steps >= R: TNET_ERR_UNSUPPORTED, nothing written"""
    nIn, H = 8, 64
    K = nIn + H
    for steps, R in ((10, 12), (4, 4), (5, 4)):
        f = Ops(layout, f"gemv_rowvec_partial_update steps {steps} R {R}")
        vW, vb, vcb = f.io(rnd((K, H), 1)), f.io(rnd(H, 2)), f.io(rnd(H, 3))
        vh, vD = f.io(rnd((R, K), 4)), f.inp(rnd((max(steps, 1), H), 5))
        vx, vy, part = f.inp(rnd(nIn, 6)), f.inp(rnd(H, 7)), f.out(1, cdiv(K, 64) * H)
        f.refused(lib().tnet_gemv_rowvec_partial_update(vx.ptr, nIn, vy.ptr, H, vh.ptr, vW.ptr, vW.stride, H, part.ptr,
                                                        vh.ptr, vh.stride, 0, R, vD.ptr, vD.stride, steps, vb.ptr,
                                                        vcb.ptr, 0.02, 0.5, 1e-4, S()))


# ------------------------------------------------------------------------------------------------------------------
# tnet_affine_update_row, tnet_affine_bwd_update_row
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", GUARDED_LAYOUTS)
@pytest.mark.parametrize("mmt", [0.0, 0.9])
@pytest.mark.parametrize("n_in,n_out", [(1, 1), (13, 7), (5, 68), (5, 260)])
def test_affine_update_row_views(n_in, n_out, mmt, layout):
    """(5, 68): one 16-byte pass of a wave; (5, 260): a second pass (c += 256) and a second bias block.  mmt = 0:
    corrW / corr_b are handed over as wholly poisoned views and are neither read (W and b come out finite) nor written;
    e_out / d_out / s NULL and non-NULL.  In odd and mixed n_out % 4 == 0 takes the scalar loop (mixed: W aligned,
    ld % 4 == 0, e misaligned)."""
    rng = np.random.default_rng(600 + n_out)
    x, s = rng.random(n_in).astype(np.float32), rng.random(n_in).astype(np.float32)
    e = (0.1 * rng.standard_normal(n_out)).astype(np.float32)
    W, corr = rnd((n_in, n_out), 601, 0.1), rnd((n_in, n_out), 602)
    b, cb = rnd(n_out, 603), rnd(n_out, 604)
    scale, l2 = -0.02, -1e-4
    c = np.outer(x, e).astype(np.float64) + (mmt * corr if mmt else 0)
    w = W + scale * c
    w = w + l2 * w
    gb = e + mmt * cb if mmt else e.astype(np.float64)
    er = W.astype(np.float64) @ e
    L = lib()

    def operands(f):
        vx, ve, vW, vb = f.inp(x), f.inp(e), f.io(W), f.io(b)
        if mmt:
            vC, vcb = f.io(corr), f.io(cb)
        else:
            vC, vcb = f.keep(rows=n_in, cols=n_out), f.keep(rows=1, cols=n_out)
        return vx, ve, vW, vb, vC, vcb

    def updated(f, vW, vb, vC, vcb):
        close(vW.numpy(), w, 1e-6, 1e-7, f.what + " W")
        close(vb.numpy()[0], b + scale * gb, 1e-6, 1e-7, f.what + " b")
        if mmt:
            close(vC.numpy(), c, 1e-6, 1e-7, f.what + " corrW")
            close(vcb.numpy()[0], gb, 1e-6, 1e-7, f.what + " corr_b")

    if layout != "mixed":
        f = Ops(layout, f"affine_update_row mmt {mmt}")
        vx, ve, vW, vb, vC, vcb = operands(f)
        f.check(L.tnet_affine_update_row(vx.ptr, n_in, ve.ptr, n_out, vW.ptr, vW.stride, vC.ptr, vC.stride, vb.ptr,
                                         vcb.ptr, scale, mmt, l2, S()))
        updated(f, vW, vb, vC, vcb)
    for with_eo, with_d in ((True, True), (False, True), (True, False), (False, False)):
        f = Ops(layout, f"affine_bwd_update_row mmt {mmt} e_out {with_eo} d_out {with_d}")
        vx, ve, vW, vb, vC, vcb = operands(f)
        vs = f.inp(s) if with_d else None
        veo = f.out(1, n_in) if with_eo else None
        vd = f.out(1, n_in) if with_d else None
        if layout == "mixed" and n_out % 4 == 0:
            assert vW.ptr % 16 == 0 and vW.stride % 4 == 0 and ve.ptr % 16 != 0
        f.check(L.tnet_affine_bwd_update_row(vx.ptr, n_in, ve.ptr, n_out, vW.ptr, vW.stride, vC.ptr, vC.stride, vb.ptr,
                                             vcb.ptr, scale, mmt, l2, P(veo), P(vs), P(vd), S()))
        updated(f, vW, vb, vC, vcb)
        if with_eo:
            close(veo.numpy()[0], er, 1e-5, 1e-6, f.what + " e_out")
        if with_d:
            close(vd.numpy()[0], er * s * (1 - s), 1e-5, 1e-6, f.what + " d_out")


# ------------------------------------------------------------------------------------------------------------------
# the output side: tnet_rnn_out_partial -> tnet_rnn_out_stats -> tnet_rnn_out_bwd_update, tnet_rnn_out_full
# ------------------------------------------------------------------------------------------------------------------
SCALE, L2 = -0.03, -1e-5


@functools.lru_cache(maxsize=None)
def out_case(nIn, H, N):
    """one frame's output side in fp64.  Two columns of Wo and bo are identical and carry the largest logit: an exact
    tie that the argmax key must resolve to the first (they lie in different 256- and 64-column blocks where N allows)"""
    rng = np.random.default_rng([nIn, H, N])
    hs = cdiv(nIn + H, 64)
    hpart = (rng.standard_normal((hs, H)) / np.sqrt(hs)).astype(np.float32)
    hb = rng.standard_normal(H).astype(np.float32)
    Wo = (0.05 * rng.standard_normal((H, N))).astype(np.float32)
    bo = rng.standard_normal(N).astype(np.float32)
    corrWo = (0.01 * rng.standard_normal((H, N))).astype(np.float32)
    corr_bo = (0.01 * rng.standard_normal(N)).astype(np.float32)
    j1, j2 = (1, N - 2) if N >= 4 else (0, 0)
    Wo[:, j2], bo[j1], bo[j2] = Wo[:, j1], 10.0, 10.0
    h = sigmoid(hb + hpart.astype(np.float64).sum(0))
    z = bo + h @ Wo.astype(np.float64)
    z[j2] = z[j1]  # (the same sum: a blocked matrix product may round the two columns differently)
    y = np.exp(z - z.max())
    y /= y.sum()
    assert int(np.argmax(y)) == j1 and y[j1] == y[j2]
    return frozen(hs=hs, hpart=hpart, hb=hb, Wo=Wo, bo=bo, corrWo=corrWo, corr_bo=corr_bo, h=h, z=z, y=y, j1=j1,
                  label=(7 * H + 3) % N)


def check_pairs(smx, z_gpu, per, what):
    """the softmax pairs: the exact maximum of the stored z per `per` columns and the sum of exp(z - max) (fast_exp:
    relative error <= 1e-6, kcommon.h)"""
    N = len(z_gpu)
    assert smx.shape == (2 * cdiv(N, per),)
    for g in range(cdiv(N, per)):
        zc = z_gpu[per * g: per * g + per]
        assert smx[2 * g] == float(zc.max()), f"{what}: pair {g} max"
        np.testing.assert_allclose(smx[2 * g + 1], np.exp(zc.astype(np.float64) - float(zc.max())).sum(), rtol=1e-5,
                                   err_msg=f"{what}: pair {g} sum")


# (mmt, train, label kind, the optional output passed as NULL)
BWD_VARIANTS = [(0.0, 1, "in", None), (0.5, 1, "in", "y"), (0.5, 0, "in", "e"), (0.0, 0, "none", "e_out"),
                (0.0, 1, "none", "d"), (0.5, 1, "past", None), (0.5, 1, "tie", None)]


def run_bwd_update(layout, c, N, H, z32, smx, pairs, h32, what):
    """tnet_rnn_out_bwd_update in every variant on fresh views of the forward's results (z, the pairs and h are pure
    inputs here), against fp64 from those results' fp64 counterparts"""
    L = lib()
    for mmt, train, lk, null in BWD_VARIANTS:
        t = {"in": c.label, "none": -1, "past": N + 3, "tie": N - 2 if N >= 4 else 0}[lk]
        tt = t if 0 <= t < N else -1
        f = Ops(layout, f"{what} -> rnn_out_bwd_update mmt {mmt} train {train} label {t} without {null}")
        vz, vsmx, vh = f.inp(z32), f.inp(smx, np.float64), f.inp(h32)
        vlab = f.inp(np.array([t], np.int32), np.int32)
        par = f.io if train else f.keep
        vWo, vbo = par(c.Wo), par(c.bo)
        if mmt and train:
            vC, vcb = f.io(c.corrWo), f.io(c.corr_bo)
        elif mmt:
            vC, vcb = f.keep(c.corrWo), f.keep(c.corr_bo)
        else:  # momentum 0: wholly poisoned, neither read nor written
            vC, vcb = f.keep(rows=H, cols=N), f.keep(rows=1, cols=N)
        vy = None if null == "y" else f.out(1, N)
        ve = None if null == "e" else f.out(1, N)
        # e_out / d belong to the `train` part of the header's contract: without it they are left as they were
        side = f.out if train else (lambda r, n: f.keep(rows=r, cols=n))
        veo = None if null == "e_out" else side(1, H)
        vd = None if null == "d" else side(1, H)
        vstats = f.io(np.zeros(1024), np.float64)
        vkey = f.io(np.zeros(1, np.uint64), np.uint64)
        if layout == "mixed" and N % 4 == 0:
            assert vWo.ptr % 16 == 0 and vWo.stride % 4 == 0 and vz.ptr % 16 != 0
        f.check(L.tnet_rnn_out_bwd_update(vz.ptr, vsmx.ptr, pairs, N, vlab.ptr, vh.ptr, H, vWo.ptr, vWo.stride, vC.ptr,
                                          vC.stride, vbo.ptr, vcb.ptr, SCALE, mmt, L2, P(vy), P(ve), P(veo), P(vd),
                                          vstats.ptr, vkey.ptr, train, S()))
        er = c.y - (np.arange(N) == tt)
        if vy:
            close(vy.numpy()[0], c.y, 2e-5, 1e-9, f.what + " y")
        if ve:
            close(ve.numpy()[0], er, 2e-5, 1e-8, f.what + " e")
        if train:
            eor = c.Wo.astype(np.float64) @ er
            if veo:
                close(veo.numpy()[0], eor, 1e-4, 1e-6, f.what + " e_out")
            if vd:
                close(vd.numpy()[0], eor * c.h * (1 - c.h), 1e-4, 1e-6, f.what + " d")
            cr = np.outer(c.h, er) + (mmt * c.corrWo if mmt else 0)
            gb = er + (mmt * c.corr_bo if mmt else 0)
            Wn = c.Wo + SCALE * cr
            close(vWo.numpy(), Wn + L2 * Wn, 1e-5, 1e-7, f.what + " Wo")
            close(vbo.numpy()[0], c.bo + SCALE * gb, 1e-5, 1e-7, f.what + " bo")
            if mmt:
                # the momentum has no kernel-level bound of its own in this chain; this one is what the bounds of its
                # factors allow: h (1e-5 |h| + 1e-6) and e (2e-5 |e| + 1e-8) carried through c = h e + mmt corr, plus
                # two fp32 roundings of the sum's terms
                he = np.abs(np.outer(c.h, er))
                tol = np.outer(1e-5 * c.h + 1e-6, np.abs(er)) + np.outer(c.h, 2e-5 * np.abs(er) + 1e-8) + \
                    2 * U * (he + np.abs(mmt * c.corrWo))
                within(vC.numpy(), cr, tol, f.what + " corrWo")
                within(vcb.numpy()[0], gb, 2e-5 * np.abs(er) + 1e-8 + 2 * U * (np.abs(er) + np.abs(mmt * c.corr_bo)),
                       f.what + " corr_bo")
        stats = vstats.numpy()[0]
        xent = -np.log(max(c.y[tt], FLT_MIN)) if tt >= 0 else 0.0
        close(stats[0], xent, 1e-5, 1e-6, f.what + " xent")
        assert not stats[1:].any(), f.what + ": a statistics word besides slot 0's error was written"
        key = int(vkey.numpy()[0, 0])
        assert 0xFFFFFFFF - (key & 0xFFFFFFFF) == c.j1, f.what + ": the key's column (first of the two equal maxima)"
        ybits = np.array([key >> 32], np.uint32).view(np.float32)[0]
        close(ybits, c.y[c.j1], 2e-5, 1e-9, f.what + " the key's y")
        if vy:
            assert ybits == vy.numpy()[0].max() and int(np.argmax(vy.numpy()[0])) == c.j1


@pytest.mark.parametrize("layout", GUARDED_LAYOUTS)
@pytest.mark.parametrize("nIn,H,N", [(8, 64, 5), (30, 70, 300), (8, 68, 1028), (8, 68, 1025), (8, 8, 4100),
                                     (8, 8, 5001), (8, 4, 16384)])
def test_rnn_out_stats_chain_views(nIn, H, N, layout):
    """(8, 64, 5), (30, 70, 300): rnn_out_bwd_kernel<1>; 1028: <4> in its register form; 1025: <4> scalar; 4100: <4>'s
    `c += STEP` vector loop; 5001: <4> scalar past 4096; 16384: 64 pairs, the documented limit (the last three reached
    by no other test).  z = NULL once for tnet_rnn_out_stats."""
    c = out_case(nIn, H, N)
    L, osl, G = lib(), cdiv(H, 64), cdiv(N, 256)
    f = Ops(layout, f"rnn_out_partial ({nIn}, {H}, {N})")
    vhp, vhb, vWo, vbo = f.inp(c.hpart.reshape(1, -1)), f.inp(c.hb), f.inp(c.Wo), f.inp(c.bo)
    vh, vop, vz, vsmx = f.out(1, H), f.out(1, osl * N), f.out(1, N), f.out(1, 2 * G, np.float64)
    f.check(L.tnet_rnn_out_partial(vhp.ptr, c.hs, vhb.ptr, vh.ptr, H, vWo.ptr, vWo.stride, N, vop.ptr, S()),
            partial=(vz, vsmx))
    h32 = vh.numpy()[0]
    close(h32, c.h, 1e-5, 1e-6, f.what + " h")
    pr, mag = slice_partials(h32, c.Wo)
    within(vop.numpy().reshape(osl, N), pr, 2e-5 * mag + 1e-6, f.what + " opart")
    f.what = f"rnn_out_stats ({nIn}, {H}, {N})"
    f.check(L.tnet_rnn_out_stats(vop.ptr, H, N, vbo.ptr, None, vsmx.ptr, S()), partial=(vz,))  # z = NULL
    assert (vz.raw() == POISON).all()
    smx_without_z = vsmx.raw()
    f.check(L.tnet_rnn_out_stats(vop.ptr, H, N, vbo.ptr, vz.ptr, vsmx.ptr, S()))
    np.testing.assert_array_equal(vsmx.raw(), smx_without_z, err_msg="the pairs do not depend on z being stored")
    z32, smx = vz.numpy()[0], vsmx.numpy()[0]
    close(z32, c.z, 1e-5, 1e-5, f.what + " z")
    check_pairs(smx, z32, 256, f.what)
    run_bwd_update(layout, c, N, H, z32, smx, G, h32, f"stats chain ({nIn}, {H}, {N})")


@pytest.mark.parametrize("layout", ["tight", "offset"])
def test_rnn_out_bwd_update_65_pairs_refused_views(layout):
    """N = 16385 through tnet_rnn_out_stats gives 65 pairs: tnet_rnn_out_bwd_update answers TNET_ERR_UNSUPPORTED and
    writes nothing"""
    H, N = 4, 16385
    rng = np.random.default_rng(65)
    f = Ops(layout, "rnn_out_stats N 16385 -> rnn_out_bwd_update 65 pairs")
    vop, vbo = f.inp(rng.standard_normal(N).astype(np.float32)), f.inp(rng.standard_normal(N).astype(np.float32))
    vz, vsmx = f.out(1, N), f.out(1, 2 * 65, np.float64)
    f.check(lib().tnet_rnn_out_stats(vop.ptr, H, N, vbo.ptr, vz.ptr, vsmx.ptr, S()))
    vh, vlab = f.inp(rng.random(H).astype(np.float32)), f.inp(np.array([3], np.int32), np.int32)
    vWo, vC, vcb = f.io(rnd((H, N), 66)), f.io(rnd((H, N), 67)), f.io(rnd(N, 68))
    vy, ve, veo, vd = f.out(1, N), f.out(1, N), f.out(1, H), f.out(1, H)
    vstats, vkey = f.io(np.zeros(1024), np.float64), f.io(np.zeros(1, np.uint64), np.uint64)
    vbo2 = f.io(rng.standard_normal(N).astype(np.float32))
    before = f.snapshot()
    for train in (1, 0):
        f.refused(lib().tnet_rnn_out_bwd_update(vz.ptr, vsmx.ptr, 65, N, vlab.ptr, vh.ptr, H, vWo.ptr, vWo.stride, vC.ptr,
                                                vC.stride, vbo2.ptr, vcb.ptr, SCALE, 0.5, L2, vy.ptr, ve.ptr, veo.ptr,
                                                vd.ptr, vstats.ptr, vkey.ptr, train, S()), before=before)


@pytest.mark.parametrize("layout", ["tight", "offset"])
@pytest.mark.parametrize("T", [1, 300])
def test_argmax_correct_views(T, layout):
    """the keys as an exact 8-byte view: frame accuracy = #(key != 0 and its column == the label, 0 for an unlabeled
    frame) added to slot 0's `correct`; 300 frames: a second pass of the 256 threads"""
    N = 37
    rng = np.random.default_rng(T)
    cols = rng.integers(0, N, T)
    labels = np.where(rng.random(T) < 0.5, cols, rng.integers(-1, N + 2, T)).astype(np.int32)
    ybits = rng.random(T).astype(np.float32).view(np.uint32).astype(np.uint64)
    keys = (ybits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - cols.astype(np.uint64))
    keys[3::7] = 0  # a frame whose key was never folded counts as wrong
    des = np.where((labels >= 0) & (labels < N), labels, 0)
    ref = float(((keys != 0) & (cols == des)).sum())
    f = Ops(layout, f"argmax_correct T {T}")
    vk, vl = f.inp(keys, np.uint64), f.inp(labels, np.int32)
    base = np.zeros(1024)
    base[1] = 5.0
    vst = f.io(base, np.float64)
    f.check(lib().tnet_argmax_correct(vk.ptr, vl.ptr, T, N, vst.ptr, S()))
    got = vst.numpy()[0]
    assert got[1] == 5.0 + ref and got[0] == 0.0 and not got[2:].any()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nIn,H,N", [(8, 64, 5), (30, 70, 300), (8, 68, 1028), (8, 2048, 64)])
def test_rnn_out_full_views(nIn, H, N, layout):
    """tnet_rnn_out_full (smx exactly 2 ceil(N/64) doubles) and tnet_rnn_out_bwd_update with ceil(N/64) pairs;
    H = 2048: both units of a thread, the Wo reload loop"""
    c = out_case(nIn, H, N)
    L, G = lib(), cdiv(N, 64)
    f = Ops(layout, f"rnn_out_full ({nIn}, {H}, {N})")
    vhp, vhb, vWo, vbo = f.inp(c.hpart.reshape(1, -1)), f.inp(c.hb), f.inp(c.Wo), f.inp(c.bo)
    vh, vz, vsmx = f.out(1, H), f.out(1, N), f.out(1, 2 * G, np.float64)
    f.check(L.tnet_rnn_out_full(vhp.ptr, c.hs, vhb.ptr, vh.ptr, H, vWo.ptr, vWo.stride, N, vbo.ptr, None, vsmx.ptr, S()),
            partial=(vz,))  # z = NULL
    assert (vz.raw() == POISON).all()
    f.check(L.tnet_rnn_out_full(vhp.ptr, c.hs, vhb.ptr, vh.ptr, H, vWo.ptr, vWo.stride, N, vbo.ptr, vz.ptr, vsmx.ptr, S()))
    h32, z32, smx = vh.numpy()[0], vz.numpy()[0], vsmx.numpy()[0]
    close(h32, c.h, 1e-5, 1e-6, f.what + " h")
    close(z32, c.z, 1e-5, 1e-5, f.what + " z")
    check_pairs(smx, z32, 64, f.what)
    if H <= 70:
        run_bwd_update(layout, c, N, H, z32, smx, G, h32, f"rnn_out_full ({nIn}, {H}, {N})")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("H,N", [(2052, 5), (8, 4097)])
def test_rnn_out_full_refusals_views(H, N, layout):
    """H > 2048 and N > 4096 (65 pairs): TNET_ERR_UNSUPPORTED, nothing written"""
    hs = cdiv(8 + H, 64)
    f = Ops(layout, f"rnn_out_full H {H} N {N}")
    vhp, vhb, vWo, vbo = f.inp(rnd((1, hs * H), 70)), f.inp(rnd(H, 71)), f.inp(rnd((H, N), 72)), f.inp(rnd(N, 73))
    vh, vz, vsmx = f.out(1, H), f.out(1, N), f.out(1, 2 * cdiv(N, 64), np.float64)
    f.refused(lib().tnet_rnn_out_full(vhp.ptr, hs, vhb.ptr, vh.ptr, H, vWo.ptr, vWo.stride, N, vbo.ptr, vz.ptr, vsmx.ptr,
                                      S()))


# ------------------------------------------------------------------------------------------------------------------
# the look-ahead pair
# ------------------------------------------------------------------------------------------------------------------
LR = float(np.float32(0.02))
# the three smallest of tests/test_gpu_rnn_ahead.py's CASES and one wide case (rnn_out_bwd_kernel<4>, register form)
AHEAD_CASES = [(8, 64, 5, 1, 2, 1, 0.0, 0.0), (8, 64, 5, 9, 10, 7, 0.5, 1e-4), (30, 68, 300, 5, 6, 4, 0.5, 1e-4),
               (8, 68, 1028, 9, 10, 7, 0.5, 1e-4)]


@functools.lru_cache(maxsize=None)
def ahead_case(nIn, H, N, steps, R):
    rng = np.random.default_rng([nIn, H, N, steps, R])
    K = nIn + H
    f32 = np.float32
    hist = rng.standard_normal((R, K)).astype(f32)
    hist[:, nIn:] = rng.random((R, H)).astype(f32)
    return frozen(W=(rng.standard_normal((K, H)) / np.sqrt(K)).astype(f32), b=(0.5 * rng.standard_normal(H)).astype(f32),
                  cb=(0.01 * rng.standard_normal(H)).astype(f32), hist=hist,
                  D=(0.1 * rng.standard_normal((steps, H))).astype(f32),
                  x_next=rng.standard_normal(nIn).astype(f32), bnext=(0.5 * rng.standard_normal(H)).astype(f32),
                  cbnext=(0.01 * rng.standard_normal(H)).astype(f32))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nIn,H,N,steps,R,head,mmt,wc", AHEAD_CASES)
def test_rnn_ahead_pair_views(nIn, H, N, steps, R, head, mmt, wc, layout):
    """Launch 1 (tnet_rnn_out_bwd_update_ahead), with bnext and x_next each NULL once: the output-layer side ==
    tnet_rnn_out_bwd_update(train = 1), the look-ahead partials == tnet_gemv_rowvec_partial([x_next, h], W), each on
    copies in the same layout, bit for bit (whole buffers); vout is exactly one ring row, the other R - 1 unchanged;
    dpart exactly ceil(K/64) x 16 with the columns past `steps` unwritten; the bias copy exact.  Launch 2
    (tnet_rnn_out_full_ahead): W, bnext, cbnext == tnet_rnn_update's W, b, cb bit for bit; h and z at
    test_gpu_rnn_ahead.py's fixed tolerances and inside its forward bounds.  In `odd` launch 2 is refused
    (TNET_ERR_UNSUPPORTED: W and D misaligned, ldw and ldd off 4) with every buffer bit-identical."""
    c, a = out_case(nIn, H, N), ahead_case(nIn, H, N, steps, R)
    L, K, G, hs = lib(), nIn + H, cdiv(N, 64), cdiv(nIn + H, 64)
    push = (head + R - 1) % R
    # frame t's forward on views: h, z, the pairs
    f0 = Ops(layout, "rnn_out_full before the look-ahead pair")
    vhp, vhb, vWo0, vbo0 = f0.inp(c.hpart.reshape(1, -1)), f0.inp(c.hb), f0.inp(c.Wo), f0.inp(c.bo)
    vh0, vz0, vsmx0 = f0.out(1, H), f0.out(1, N), f0.out(1, 2 * G, np.float64)
    f0.check(L.tnet_rnn_out_full(vhp.ptr, c.hs, vhb.ptr, vh0.ptr, H, vWo0.ptr, vWo0.stride, N, vbo0.ptr, vz0.ptr,
                                 vsmx0.ptr, S()))
    h32, z32, smx = vh0.numpy()[0], vz0.numpy()[0], vsmx0.numpy()[0]
    row = np.concatenate([a.x_next, h32])
    hrows = np.stack([a.hist[(head + i) % R] for i in range(steps)]).astype(np.float64)
    dots_ref = hrows @ row.astype(np.float64)
    look_state = None
    for bias_copy, look in ((True, True), (False, True), (True, False)):
        sides = {}
        for ahead in (False, True):
            f = Ops(layout, f"{'rnn_out_bwd_update_ahead' if ahead else 'rnn_out_bwd_update + gemv_rowvec_partial'} "
                            f"bias copy {bias_copy} look {look}")
            vz, vsmx, vh = f.inp(z32), f.inp(smx, np.float64), f.inp(h32)
            vlab = f.inp(np.array([c.label], np.int32), np.int32)
            vWo, vbo = f.io(c.Wo), f.io(c.bo)
            vC, vcbo = (f.io(c.corrWo), f.io(c.corr_bo)) if mmt else (f.keep(rows=H, cols=N), f.keep(rows=1, cols=N))
            ve, veo, vd = f.out(1, N), f.out(1, H), f.out(1, H)
            vstats, vkey = f.io(np.zeros(1024), np.float64), f.io(np.zeros(1, np.uint64), np.uint64)
            vW, vx = f.inp(a.W), f.inp(a.x_next)
            part = f.out(1, hs * H) if look else f.keep(rows=1, cols=hs * H)
            if not ahead:
                f.check(L.tnet_rnn_out_bwd_update(vz.ptr, vsmx.ptr, G, N, vlab.ptr, vh.ptr, H, vWo.ptr, vWo.stride,
                                                  vC.ptr, vC.stride, vbo.ptr, vcbo.ptr, SCALE, mmt, L2, None, ve.ptr,
                                                  veo.ptr, vd.ptr, vstats.ptr, vkey.ptr, 1, S()), partial=(part,))
                if look:
                    f.check(L.tnet_gemv_rowvec_partial(vx.ptr, nIn, vh.ptr, H, None, vW.ptr, vW.stride, H, part.ptr, S()))
            else:
                vbn, vcbn = f.inp(a.bnext), f.inp(a.cbnext)
                vb, vcb = (f.io(a.b), f.io(a.cb)) if bias_copy else (f.keep(a.b), f.keep(a.cb))
                vhist = f.io(a.hist) if look else f.keep(a.hist)
                dpart = f.out(1, hs * 16) if look else f.keep(rows=1, cols=hs * 16)
                f.check(L.tnet_rnn_out_bwd_update_ahead(
                    vz.ptr, vsmx.ptr, G, N, vlab.ptr, vh.ptr, H, vWo.ptr, vWo.stride, vC.ptr, vC.stride, vbo.ptr,
                    vcbo.ptr, SCALE, mmt, L2, ve.ptr, veo.ptr, vd.ptr, vstats.ptr, vkey.ptr,
                    vbn.ptr if bias_copy else None, vcbn.ptr if bias_copy else None, vb.ptr, vcb.ptr,
                    vx.ptr if look else None, nIn, vW.ptr, vW.stride, part.ptr, dpart.ptr,
                    vhist.ptr + 4 * push * vhist.stride, vhist.ptr, vhist.stride, head, R, steps, S()),
                    partial=(dpart,))
                if bias_copy:
                    np.testing.assert_array_equal(vb.numpy()[0], a.bnext, err_msg=f.what + " bias copy")
                    np.testing.assert_array_equal(vcb.numpy()[0], a.cbnext, err_msg=f.what + " momentum copy")
                if look:
                    ring = vhist.numpy()
                    np.testing.assert_array_equal(ring[push], row, err_msg=f.what + " pushed ring row")
                    keep = np.arange(R) != push
                    np.testing.assert_array_equal(ring[keep], a.hist[keep], err_msg=f.what + " the other ring rows")
                    dp = dpart.numpy().reshape(hs, 16)
                    assert (dp[:, steps:].view(np.uint32) == POISON).all(), f.what + ": dpart past `steps` written"
                    assert not np.isnan(dp[:, :steps]).any()
                    err = np.abs(dp[:, :steps].astype(np.float64).sum(0) - dots_ref)
                    within(err, 0.0, 8 * U * (np.abs(hrows) @ np.abs(row.astype(np.float64))), f.what + " dots")
                    if bias_copy:
                        look_state = (part, dpart, vhist, vb, vcb)
            sides[ahead] = [v.raw() for v in (vWo, vbo, vC, vcbo, ve, veo, vd, vstats, vkey, part)]
        for x, y, name in zip(sides[False], sides[True], ("Wo", "bo", "corrWo", "corr_bo", "e", "e_out", "d", "stats",
                                                          "key", "look-ahead partials")):
            np.testing.assert_array_equal(x, y, err_msg=f"launch 1 vs the named entry points: {name} (whole buffers)")

    # ---- launch 2 on the state launch 1 (bias copy and look-ahead) left
    part, dpart, vhist, vb, vcb = look_state
    b1, cb1 = vb.numpy()[0], vcb.numpy()[0]
    f = Ops(layout, "rnn_out_full_ahead")
    vhp2, vdp = f.inp(part.numpy()), f.keep(dpart.numpy())
    # (dpart's columns past `steps` are poison, as launch 1 left them: read into LDS, never used)
    vhb, vcbi = f.inp(b1), f.inp(cb1)
    vWo, vbo, vD, vring = f.inp(c.Wo), f.inp(c.bo), f.inp(a.D), f.inp(vhist.numpy())
    vW = f.io(a.W)
    vh, vz, vsmx, vbn, vcbn = f.out(1, H), f.out(1, N), f.out(1, 2 * G, np.float64), f.out(1, H), f.out(1, H)
    rc = L.tnet_rnn_out_full_ahead(vhp2.ptr, hs, vhb.ptr, vh.ptr, H, vWo.ptr, vWo.stride, N, vbo.ptr, vz.ptr, vsmx.ptr,
                                   vdp.ptr, vD.ptr, vD.stride, steps, LR, mmt, wc, vcbi.ptr, vbn.ptr, vcbn.ptr, vW.ptr,
                                   vW.stride, K, vring.ptr, vring.stride, head, R, S())
    if layout == "odd":
        assert vW.stride % 4 and vD.stride % 4 and vW.ptr % 16 and vD.ptr % 16
        f.refused(rc)
        return
    f.check(rc)
    g = Ops(layout, "rnn_update on copies")
    mW, mb, mcb, mD, mring = g.io(a.W), g.io(b1), g.io(cb1), g.inp(a.D), g.inp(vhist.numpy())
    g.check(L.tnet_rnn_update(mW.ptr, mW.stride, K, H, mring.ptr, mring.stride, head, R, mD.ptr, mD.stride, steps,
                              mb.ptr, mcb.ptr, LR, mmt, wc, S()))
    for x, y, name in ((vW, mW, "W"), (vbn, mb, "bnext"), (vcbn, mcb, "cbnext")):
        np.testing.assert_array_equal(x.raw(), y.raw(), err_msg=f"launch 2 vs tnet_rnn_update: {name} (whole buffers)")
    # fp64: the update formula (cuRecurrent.cc:88-153), h, z
    Dd, W64, v = a.D.astype(np.float64), a.W.astype(np.float64), row.astype(np.float64)
    bn = b1.astype(np.float64) + mmt * cb1.astype(np.float64) - LR * Dd.sum(0)
    W1 = W64 + (-LR * wc) * W64 - LR * (hrows.T @ Dd)
    hr = sigmoid(bn + v @ W1)
    Wo64, bo64 = c.Wo.astype(np.float64), c.bo.astype(np.float64)
    zr = bo64 + hr @ Wo64
    h2, z2 = vh.numpy()[0], vz.numpy()[0]
    close(h2, hr, 1e-5, 1e-6, f.what + " h")
    close(z2, zr, 1e-5, 1e-5, f.what + " z")
    hb_ = _h_bound(SimpleNamespace(steps=steps, wc=wc), v, W64, bn, dots_ref, Dd, hs)
    within(h2, hr, hb_, f.what + " h inside its forward bound")
    within(z2, zr, _z_bound(hr, hb_, Wo64, bo64), f.what + " z inside its forward bound")
    check_pairs(vsmx.numpy()[0], z2, 64, f.what)


# ------------------------------------------------------------------------------------------------------------------
# tnet_gemv_rowvec_softmax_xent
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("K,N", [(64, 1), (100, 300), (8, 1028), (8, 4096)])
def test_gemv_rowvec_softmax_xent_views(K, N, layout):
    """label in range, -1 and N (out of range: unlabeled); z / y / e each NULL once; N = 4096 is the limit (16 columns
    a thread), N = 4097 TNET_ERR_UNSUPPORTED with nothing written"""
    rng = np.random.default_rng([K, N])
    v, W, b = rnd(K, 800 + K), rnd((K, N), 801 + N, 0.1), rnd(N, 802 + N)
    b[N // 2] += 8.0  # a clear maximum: `correct` does not hang on rounding
    zr = b + v.astype(np.float64) @ W
    yr = np.exp(zr - zr.max())
    yr /= yr.sum()
    slices, L = cdiv(K, 64), lib()
    for t, null in ((int(rng.integers(0, N)), None), (N // 2, "z"), (-1, "y"), (N, "e")):
        tt = t if 0 <= t < N else -1
        f = Ops(layout, f"gemv_rowvec_softmax_xent ({K}, {N}) label {t} without {null}")
        vv, vW, vb, vlab = f.inp(v), f.inp(W), f.inp(b), f.inp(np.array([t], np.int32), np.int32)
        vz, vy, ve = (None if null == n else f.out(1, N) for n in ("z", "y", "e"))
        vstats, ws = f.io(np.zeros(1024), np.float64), f.out(1, slices * N)
        f.check(L.tnet_gemv_rowvec_softmax_xent(vv.ptr, K, vW.ptr, vW.stride, vb.ptr, P(vz), P(vy), P(ve), N, vlab.ptr,
                                                vstats.ptr, ws.ptr, S()))
        if vz:
            close(vz.numpy()[0], zr, 1e-5, 1e-5, f.what + " z")
        if vy:
            close(vy.numpy()[0], yr, 2e-5, 1e-9, f.what + " y")
        if ve:
            close(ve.numpy()[0], yr - (np.arange(N) == tt), 2e-5, 1e-8, f.what + " e")
        stats = vstats.numpy()[0]
        close(stats[0], -np.log(max(yr[tt], FLT_MIN)) if tt >= 0 else 0.0, 1e-5, 1e-6, f.what + " xent")
        assert stats[1] == float(int(np.argmax(yr)) == (tt if tt >= 0 else 0)) and not stats[2:].any()
    if N == 4096:
        f = Ops(layout, "gemv_rowvec_softmax_xent N 4097")
        vv, vW, vb = f.inp(v), f.inp(rnd((K, 4097), 803, 0.1)), f.inp(rnd(4097, 804))
        vlab = f.inp(np.array([5], np.int32), np.int32)
        vz, vy, ve = f.out(1, 4097), f.out(1, 4097), f.out(1, 4097)
        vstats, ws = f.io(np.zeros(1024), np.float64), f.out(1, slices * 4097)
        f.refused(L.tnet_gemv_rowvec_softmax_xent(vv.ptr, K, vW.ptr, vW.stride, vb.ptr, vz.ptr, vy.ptr, ve.ptr, 4097,
                                                  vlab.ptr, vstats.ptr, ws.ptr, S()))
