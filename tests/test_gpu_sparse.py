"""<sparselinearity>: the fused update (tnet_sparse_update, both forms), the bit-mask kernels, the component, its
file format and the C ABI.  The layer has no CPU twin in the reference (src/TNetLib), so parity is restated in
float64 numpy here (cuSparseLinearity.cc:28-97), not pinned to reference output.

Tolerances (tests/test_gpu_shared.py):
  W after the update   |got - ref| <= 2e-5 * |scale| * (|X|^T |E|) + 2e-7 * |W_ref| + 1e-7 -- mask, soft threshold and
                       decay are 1-Lipschitz, so the bound of W + scale*c carries through them
  corrW, accu          the same with scale = 1
  bias                 rtol 1e-5, floors 1e-6 on the bias and 1e-5 on the sum
  mask kernels         exact (fp32 comparisons on given inputs)
  component level      rtol 2e-4 / atol 2e-6 per step, xent rtol 1e-5 (tests/test_gpu_discrete.py)
"""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tnet_amd import DeviceArray, Network, Objective, Trainer, TnetError, formats  # noqa: E402
from tnet_amd._lib import MatrixDim, check, lib  # noqa: E402

ERR_ARG = -1
FORM_AUTO, FORM_SINGLE, FORM_SLICED, TILE128 = 0, 1, 2, 0x20

# (rows, n_in, n_out): one element; the masked scalar path and one partial mask word; a row that crosses a word by
# one bit; several tiles with words straddling a 64-column tile edge; many tiles, still below the threshold of the
# automatic single launch (21 x 21 = 441 tiles of 64x64 against 512); no rows; and past that threshold (21 x 26)
SHAPES = [(1, 1, 1), (33, 39, 10), (16, 24, 33), (130, 72, 136), (70, 1300, 1290), (0, 8, 8), (40, 1290, 1601)]
BIG, PAST = (70, 1300, 1290), (40, 1290, 1601)


def S():
    return lib().tnet_stream()


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def dev_nan_pad(a):
    """`a` on the device with NaN in the padding columns [cols, stride) of every row"""
    a = np.asarray(a, np.float32)
    d = DeviceArray(a.shape[0], a.shape[1])
    host = np.full((d.rows, d.stride), np.nan, np.float32)
    host[:, :d.cols] = a
    check(lib().tnet_memcpy_h2d(d.ptr, host.ctypes.data, host.nbytes), "h2d")
    return d


def raw(d):
    host = np.empty((d.rows, d.stride), d.dtype)
    check(lib().tnet_memcpy_d2h(host.ctypes.data, d.ptr, host.nbytes), "d2h")
    return host


def padding_untouched(d):
    return bool(np.isnan(raw(d)[:, d.cols:]).all())


def pack_host(mask, ldmask, fill=0):
    """the bit matrix of a 0/1 matrix: bit c & 31 of word c >> 5 of row r; words past ceil(cols / 32) hold `fill`"""
    rows, cols = mask.shape
    words = np.full((rows, ldmask), fill, np.uint32)
    words[:, :(cols + 31) // 32] = 0
    r, c = np.nonzero(mask)
    np.bitwise_or.at(words, (r, c >> 5), np.uint32(1) << (c & 31).astype(np.uint32))
    return words


def dev_bits(words):
    d = DeviceArray(words.shape[0], words.shape[1], np.uint32, stride=words.shape[1])
    check(lib().tnet_memcpy_h2d(d.ptr, np.ascontiguousarray(words).ctypes.data, words.nbytes), "h2d")
    return d


def draw_mask(shape, density, seed):
    if density >= 1.0:
        return np.ones(shape, np.float32)
    return (np.random.default_rng(seed).random(shape) < density).astype(np.float32)


# ------------------------------------------------------------------------------ float64 restatement
def update_ref(X, E, W, corr, accu, mask, b, cb, scale, mmt, l1c, l2):
    """CuSparseLinearity::Update (cuSparseLinearity.cc:28-63) without the frame count, in float64"""
    X, E = X.astype(np.float64), E.astype(np.float64)
    g, mag = X.T @ E, np.abs(X).T @ np.abs(E)
    c = g + mmt * corr
    w = W + scale * c
    a = accu + c
    w = np.where(mask != 0, w, 0.0)
    if l1c > 0:
        w = np.where(np.abs(w) < l1c, 0.0, np.where(w > 0, w - l1c, w + l1c))
    if l2 != 0:
        w = w + l2 * w
    cbr = E.sum(axis=0) + mmt * cb
    return dict(W=w, corr=c, accu=a, b=b + scale * cbr, cb=cbr, mag=mag)


def mask_update_ref(W, mask, accu, sparsify, unsparsify, nframes):
    """CuSparseLinearity::UpdateMask (cuSparseLinearity.cc:66-97) with fp32 fabsf in both comparisons"""
    W, accu = np.asarray(W, np.float32), np.asarray(accu, np.float32)
    cut = (mask != 0) & (np.abs(W) < np.float32(sparsify))
    with np.errstate(divide="ignore", invalid="ignore"):
        wake = (mask == 0) & (np.abs(accu) / np.float32(nframes) > np.float32(unsparsify))
    new_mask = np.where(cut, 0.0, np.where(wake, 1.0, mask)).astype(np.float32)
    return np.where(cut, np.float32(0), W), new_mask


# ------------------------------------------------------------------------------------ kernel level
def run_update(form, X, E, W, corr, accu, mask, b, cb, scale, mmt, l1c, l2):
    dX, dE = DeviceArray.from_numpy(X), DeviceArray.from_numpy(E)
    dW, dC, dA = dev_nan_pad(W), dev_nan_pad(corr), dev_nan_pad(accu)
    ldmask = (W.shape[1] + 31) // 32 + 1           # one word of padding per row: never touched
    dM = dev_bits(pack_host(mask, ldmask, fill=0xDEADBEEF))
    db, dcb = DeviceArray.vector(b), DeviceArray.vector(cb)
    was = lib().tnet_sparse_update_form(form)
    try:
        check(lib().tnet_sparse_update(dX.ptr, dX.dim, dE.ptr, dE.dim, dW.ptr, dW.dim, dC.ptr, dC.stride, dA.ptr,
                                       dA.stride, dM.ptr, ldmask, db.ptr, dcb.ptr, scale, mmt, l1c, l2, S()),
              "sparse_update")
    finally:
        lib().tnet_sparse_update_form(was)
    for d in (dW, dC, dA):
        assert padding_untouched(d)
    np.testing.assert_array_equal(raw(dM), pack_host(mask, ldmask, fill=0xDEADBEEF))   # the mask is read only
    return dict(W=dW.numpy(), corr=dC.numpy(), accu=dA.numpy(), b=db.numpy().reshape(-1), cb=dcb.numpy().reshape(-1))


def forms_for(shape):
    # both forms at both tile sizes; the automatic choice as well where it is the single launch (PAST) and where it
    # is the sliced form (a small layer, and BIG just below the threshold)
    forms = [FORM_SINGLE, FORM_SLICED, FORM_SINGLE | TILE128, FORM_SLICED | TILE128]
    return forms + [FORM_AUTO] if shape in (BIG, PAST, (130, 72, 136)) else forms


def inputs(rows, n_in, n_out, density, seed=100):
    X, E = rnd((rows, n_in), seed), rnd((rows, n_out), seed + 1, 0.01)
    mask = draw_mask((n_in, n_out), density, seed + 2)
    W = rnd((n_in, n_out), seed + 3, 0.1) * mask        # the layer's invariant: zeros under the mask
    corr, accu = rnd((n_in, n_out), seed + 4, 0.01), rnd((n_in, n_out), seed + 5, 0.1)
    b, cb = rnd(n_out, seed + 6), rnd(n_out, seed + 7, 0.01)
    return X, E, W, corr, accu, mask, b, cb


@pytest.mark.parametrize("density", [1.0, 0.3], ids=["dense", "density0.3"])
@pytest.mark.parametrize("reg", [False, True], ids=["noreg", "l1+l2"])
@pytest.mark.parametrize("mmt", [0.0, 0.5], ids=["mmt0", "mmt0.5"])
@pytest.mark.parametrize("rows,n_in,n_out", SHAPES)
def test_sparse_update(rows, n_in, n_out, mmt, reg, density):
    X, E, W, corr, accu, mask, b, cb = inputs(rows, n_in, n_out, density)
    scale = -0.3 / max(rows, 1)
    # l1c at the lower tercile of the surviving |W|: about a third of them fall under the soft threshold, the rest
    # shrink towards zero from either side
    alive = np.abs(W[mask != 0])
    l1c = float(np.quantile(alive, 1 / 3)) if reg and alive.size else 0.0
    l2 = -1e-4 if reg else 0.0
    ref = update_ref(X, E, W, corr, accu, mask, b, cb, scale, mmt, l1c, l2)
    if reg and alive.size > 30:
        zeroed = (ref["W"][mask != 0] == 0).mean()
        assert 0.2 < zeroed < 0.5 and (ref["W"] > 0).any() and (ref["W"] < 0).any()
    tol_w = 2e-5 * abs(scale) * ref["mag"] + 2e-7 * np.abs(ref["W"]) + 1e-7
    tol_c = 2e-5 * ref["mag"] + 2e-7 * np.abs(ref["corr"]) + 1e-7
    tol_a = 2e-5 * ref["mag"] + 2e-7 * np.abs(ref["accu"]) + 1e-7
    outs = {}
    for form in forms_for((rows, n_in, n_out)):
        got = outs[form] = run_update(form, X, E, W, corr, accu, mask, b, cb, scale, mmt, l1c, l2)
        ew, ec, ea = (np.abs(got[k] - ref[k]) for k in ("W", "corr", "accu"))
        print(f"form {form:#x}: W err/tol {float((ew / tol_w).max()):.3f} corr {float((ec / tol_c).max()):.3f} "
              f"accu {float((ea / tol_a).max()):.3f}")
        assert np.all(ew <= tol_w), form
        assert np.all(ec <= tol_c), form
        assert np.all(ea <= tol_a), form
        assert np.all(got["W"][mask == 0] == 0.0), form          # exactly 0.0 under the mask
        np.testing.assert_allclose(got["b"], ref["b"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(got["cb"], ref["cb"], rtol=1e-5, atol=1e-5)
    if FORM_AUTO in outs:   # the automatic choice is one of the two forms, bit for bit: which one is the routing
        same = FORM_SINGLE if (rows, n_in, n_out) == PAST else FORM_SLICED
        for k in outs[FORM_AUTO]:
            np.testing.assert_array_equal(outs[FORM_AUTO][k], outs[same][k])


@pytest.mark.parametrize("form", [FORM_SINGLE, FORM_SLICED, FORM_SINGLE | TILE128, FORM_SLICED | TILE128])
@pytest.mark.parametrize("rows,n_in,n_out", [(33, 39, 10), (130, 72, 136), BIG, PAST])
def test_sparse_update_is_deterministic(rows, n_in, n_out, form):
    """no atomics: two runs on the same inputs give the same bits for every output"""
    args = inputs(rows, n_in, n_out, 0.3, seed=200)
    runs = [run_update(form, *args, -0.01, 0.5, 0.02, -1e-4) for _ in range(2)]
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k])


@pytest.mark.parametrize("form", [FORM_SINGLE, FORM_SLICED])
def test_update_with_zero_rows_applies_momentum_mask_l1_and_decay(form):
    X, E, W, corr, accu, mask, b, cb = inputs(0, 8, 8, 0.5, seed=300)
    W = rnd((8, 8), 301, 0.1)                                     # not yet masked: the update masks it
    got = run_update(form, X, E, W, corr, accu, mask, b, cb, -0.1, 0.5, 0.03, -1e-2)
    ref = update_ref(X, E, W, corr, accu, mask, b, cb, -0.1, 0.5, 0.03, -1e-2)
    np.testing.assert_allclose(got["corr"], 0.5 * corr, rtol=1e-6)
    for k in ("W", "accu", "b", "cb"):
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-6, atol=1e-7)
    assert np.all(got["W"][mask == 0] == 0.0) and (got["W"] != 0).any()


@pytest.mark.parametrize("rows,n_out", [(r, c) for _, r, c in SHAPES] + [(5, 64), (3, 257)])
def test_mask_pack_unpack(rows, n_out):
    """pack then unpack is the identity on 0/1 matrices; bits at columns >= n_out are zero; words past
    ceil(n_out / 32) and the float matrix's padding are not written"""
    mask = draw_mask((rows, n_out), 0.5, 400 + n_out)
    nwords, ldmask = (n_out + 31) // 32, (n_out + 31) // 32 + 2
    dF = dev_nan_pad(mask * 2.5)                                  # any nonzero value is a 1
    dM = dev_bits(np.full((rows, ldmask), 0xFFFFFFFF, np.uint32))
    check(lib().tnet_sparse_mask_pack(dF.ptr, dF.dim, dM.ptr, ldmask, S()), "pack")
    words = raw(dM)
    np.testing.assert_array_equal(words, pack_host(mask, ldmask, fill=0xFFFFFFFF))
    if n_out % 32:
        assert np.all(words[:, nwords - 1] >> np.uint32(n_out % 32) == 0)
    dO = dev_nan_pad(np.full((rows, n_out), 7.0, np.float32))
    check(lib().tnet_sparse_mask_unpack(dM.ptr, ldmask, dO.ptr, dO.dim, S()), "unpack")
    np.testing.assert_array_equal(dO.numpy(), mask)
    assert padding_untouched(dO) and padding_untouched(dF)


@pytest.mark.parametrize("nframes", [1, 960])
@pytest.mark.parametrize("n_in,n_out", [(1, 1), (39, 10), (24, 33), (72, 136), (9, 300)])
def test_mask_update_is_exact(n_in, n_out, nframes):
    thr, unsp = np.float32(1e-3), np.float32(0.5)
    rng = np.random.default_rng(500 + n_out)
    mask = draw_mask((n_in, n_out), 0.5, 501 + n_out)
    # weights around the threshold: exactly 1e-3 (stays active), one ulp below (cut), both signs, clearly either side
    pool = np.array([thr, np.nextafter(thr, np.float32(0)), -thr, -np.nextafter(thr, np.float32(0)), 0.0, 5e-4, -5e-4,
                     2e-3, -0.3, np.nextafter(thr, np.float32(1))], np.float32)
    W = pool[rng.integers(0, len(pool), (n_in, n_out))]
    # accu on both sides of unsparsify_accu * nframes, the boundary itself (not above: stays off) and one ulp above
    edge = np.float32(unsp * np.float32(nframes))
    apool = np.array([edge, np.nextafter(edge, np.float32(np.inf)), -np.nextafter(edge, np.float32(np.inf)), -edge,
                      0.0, 0.25 * edge, -4.0 * edge, 3.0 * edge], np.float32)
    accu = apool[rng.integers(0, len(apool), (n_in, n_out))]
    if n_in * n_out > 100:   # every class of element is present
        assert ((mask == 1) & (W == thr)).any() and ((mask == 1) & (W == pool[1])).any()
        assert ((mask == 0) & (accu == edge)).any() and ((mask == 0) & (accu == apool[1])).any()
    Wr, mr = mask_update_ref(W, mask, accu, thr, unsp, nframes)
    ldmask = (n_out + 31) // 32 + 1
    dW, dA = dev_nan_pad(W), dev_nan_pad(accu)
    dM = dev_bits(pack_host(mask, ldmask, fill=0xDEADBEEF))
    check(lib().tnet_sparse_mask_update(dW.ptr, dW.dim, dM.ptr, ldmask, dA.ptr, dA.stride, float(thr), float(unsp),
                                        float(nframes), S()), "mask_update")
    np.testing.assert_array_equal(raw(dM), pack_host(mr, ldmask, fill=0xDEADBEEF))
    np.testing.assert_array_equal(dW.numpy(), Wr)
    np.testing.assert_array_equal(dA.numpy(), accu)
    assert padding_untouched(dW) and padding_untouched(dA)
    if n_in * n_out > 100:
        assert (mr != mask).any() and ((mask == 1) & (W == thr) & (mr == 1)).any()
        assert ((mask == 0) & (mr == 1) & (dW.numpy() == W)).any()      # woken up, W left as it is


def test_argument_errors_return_err_arg():
    """refused before any launch.  Every operand is a real device buffer of one size (8 rows of 64 floats), so a
    check that failed to refuse would still touch only memory this test owns"""
    L, s = lib(), S()
    n = 8
    X, E, W, Cw, A, M = (DeviceArray(n, n) for _ in range(6))
    b, cb = DeviceArray(1, 64), DeviceArray(1, 64)
    good = MatrixDim(n, n, 64)

    def upd(x=X.ptr, dx=good, e=E.ptr, de=good, w=W.ptr, dw=good, c=Cw.ptr, ldc=64, a=A.ptr, lda=64, m=M.ptr, ldm=1,
            bias=b.ptr, cbias=cb.ptr):
        return L.tnet_sparse_update(x, dx, e, de, w, dw, c, ldc, a, lda, m, ldm, bias, cbias, -0.1, 0.5, 0.0, 0.0, s)

    assert upd() == 0
    # a NULL operand
    for k in ("x", "e", "w", "c", "a", "m", "bias", "cbias"):
        assert upd(**{k: None}) == ERR_ARG, k
    # dimension mismatches: dX.cols != dW.rows, dE.cols != dW.cols, dX.rows != dE.rows
    assert upd(dx=MatrixDim(n, n - 1, 64)) == ERR_ARG and upd(dw=MatrixDim(n - 1, n, 64)) == ERR_ARG
    assert upd(de=MatrixDim(n, n + 1, 64)) == ERR_ARG and upd(dw=MatrixDim(n, n - 1, 64)) == ERR_ARG
    assert upd(de=MatrixDim(n - 1, n, 64)) == ERR_ARG and upd(dx=MatrixDim(n + 1, n, 64)) == ERR_ARG
    # a stride that is no multiple of 4, or below the column count
    assert upd(dx=MatrixDim(n, n, 62)) == ERR_ARG and upd(de=MatrixDim(n, n, 10)) == ERR_ARG
    assert upd(dw=MatrixDim(n, n, 62)) == ERR_ARG and upd(ldc=62) == ERR_ARG and upd(lda=10) == ERR_ARG
    assert upd(ldc=4) == ERR_ARG and upd(lda=4) == ERR_ARG and upd(dw=MatrixDim(n, n, 4)) == ERR_ARG
    # ldmask < ceil(n_out / 32)
    assert upd(ldm=0) == ERR_ARG
    wide = MatrixDim(n, 40, 64)
    assert upd(de=wide, dw=wide, ldm=1) == ERR_ARG and upd(de=wide, dw=wide, ldm=2) == 0
    # W, corrW, accu or bits overlapping X or E
    for k in ("w", "c", "a", "m"):
        assert upd(**{k: X.ptr}) == ERR_ARG and upd(**{k: E.ptr + 64}) == ERR_ARG, k
    # ... or each other
    assert upd(c=W.ptr) == ERR_ARG and upd(a=W.ptr + 16) == ERR_ARG and upd(m=W.ptr) == ERR_ARG
    assert upd(a=Cw.ptr) == ERR_ARG and upd(m=Cw.ptr + 4) == ERR_ARG and upd(m=A.ptr) == ERR_ARG
    # misaligned pointers
    assert upd(w=W.ptr + 2) == ERR_ARG and upd(m=M.ptr + 1) == ERR_ARG

    def mupd(w=W.ptr, dw=good, m=M.ptr, ldm=1, a=A.ptr, lda=64):
        return L.tnet_sparse_mask_update(w, dw, m, ldm, a, lda, 1e-3, 1e20, 1.0, s)

    assert mupd() == 0
    assert mupd(w=None) == ERR_ARG and mupd(m=None) == ERR_ARG and mupd(a=None) == ERR_ARG
    assert mupd(ldm=0) == ERR_ARG and mupd(lda=62) == ERR_ARG and mupd(lda=4) == ERR_ARG
    assert mupd(dw=MatrixDim(n, n, 62)) == ERR_ARG
    assert mupd(a=W.ptr) == ERR_ARG and mupd(m=W.ptr) == ERR_ARG and mupd(m=A.ptr) == ERR_ARG
    for fn, first in ((L.tnet_sparse_mask_pack, True), (L.tnet_sparse_mask_unpack, False)):
        def call(f=A.ptr, d=good, m=M.ptr, ldm=1):
            return fn(f, d, m, ldm, s) if first else fn(m, ldm, f, d, s)
        assert call() == 0
        assert call(f=None) == ERR_ARG and call(m=None) == ERR_ARG and call(ldm=0) == ERR_ARG
        assert call(d=MatrixDim(n, n, 62)) == ERR_ARG and call(m=A.ptr) == ERR_ARG
    # the form knob returns the previous setting
    assert L.tnet_sparse_update_form(FORM_SLICED) == FORM_AUTO and L.tnet_sparse_update_form(FORM_AUTO) == FORM_SLICED


# --------------------------------------------------------------------------------- component level
N_IN, N_HID, N_CLS, BUNCH = 40, 24, 7, 33
NET_SEED = 60


def sparse_net(seed=NET_SEED, density=0.5):
    """<sparselinearity> 40 -> 24 (density-0.5 mask in the file), <sigmoid>, <biasedlinearity> 24 -> 7, <softmax>.
    Zero bias in the sparse layer: with the --negbias draw (-4) its sigmoids sit at 0.02 and the gradients reaching
    it would test little."""
    return formats.gen_sparse_init(N_IN, N_HID, seed=seed, density=density, negbias=False) + \
        formats.gen_mlp_init([N_HID, N_CLS], seed=seed + 1)


def net_text(layers, precision=9):
    buf = io.StringIO()
    formats.write_nnet(layers, buf, precision=precision)
    return buf.getvalue()


class SparseOracle:
    """float64 restatement of CuSparseLinearity::Update (cuSparseLinearity.cc:28-63) and CuBiasedLinearity::Update
    (cuBiasedLinearity.cc:46-64) under CuNetwork::Backpropagate"""

    def __init__(self, layers):
        self.L = layers
        self.corr, self.accu, self.corr_sum, self.nframes = {}, {}, {}, 0
        for k, l in enumerate(self.L):
            if l.W is not None:
                l.W, l.b = l.W.astype(np.float64), l.b.astype(np.float64)
                self.corr[k] = (np.zeros_like(l.W), np.zeros_like(l.b))
            if l.tag == "<sparselinearity>":
                l.extra.setdefault("mask", np.ones(l.W.shape, np.float32))
                self.accu[k] = np.zeros_like(l.W)
        self.xent = 0.0

    def step(self, X, lab, lr, mmt, wc, l1, gdf):
        acts = [np.asarray(X, np.float64)]
        for l in self.L:
            a = acts[-1]
            if l.W is not None:
                a = a @ l.W + l.b
            elif l.tag == "<sigmoid>":
                a = 1.0 / (1.0 + np.exp(-a))
            elif l.tag == "<softmax>":
                e = np.exp(a - a.max(axis=1, keepdims=True))
                a = e / e.sum(axis=1, keepdims=True)
            acts.append(a)
        Y, rows = acts[-1], len(lab)
        self.xent += -np.log(Y[np.arange(rows), lab]).sum()
        err = Y.copy()
        err[np.arange(rows), lab] -= 1.0
        scale = -lr / ((rows if gdf else 1.0) / (1.0 - mmt))
        frm = 1.0 if gdf else rows
        for k in range(len(self.L) - 1, -1, -1):
            l, a_in = self.L[k], acts[k]
            if l.tag == "<sigmoid>":
                err = err * acts[k + 1] * (1.0 - acts[k + 1])
            elif l.W is not None:
                e_in = err
                err = e_in @ l.W.T                                        # pre-update weights
                cw, cb = self.corr[k]
                cw, cb = a_in.T @ e_in + mmt * cw, e_in.sum(axis=0) + mmt * cb
                self.corr[k] = (cw, cb)
                w = l.W + scale * cw
                if l.tag == "<sparselinearity>":
                    self.accu[k] = self.accu[k] + cw
                    w = np.where(l.extra["mask"] != 0, w, 0.0)
                    if l1 > 0:
                        c = lr * l1 * frm
                        w = np.where(np.abs(w) < c, 0.0, np.where(w > 0, w - c, w + c))
                    if wc > 0:
                        w = w + (-lr * wc * frm) * w
                else:
                    w = w + (-lr * wc * frm) * w
                l.W = w
                l.b = l.b + scale * cb
        self.nframes += rows
        return Y


def make_net(text, lr, mmt, wc, l1, gdf):
    net = Network(text=text)
    net.set_learn_rate(lr)
    net.set_momentum(mmt)
    net.set_weightcost(wc)
    net.set_l1(l1)
    net.set_grad_div_frm(gdf)
    return net


def bunches(n, seed, n_in=N_IN):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((BUNCH, n_in)).astype(np.float32), rng.integers(0, N_CLS, BUNCH).astype(np.int32))
            for _ in range(n)]


# l1 so that the soft threshold c = lr*l1*(gdf ? 1 : rows) is 0.01 under either setting: a tenth of a typical weight
CONSTS = {True: dict(lr=0.05, mmt=0.5, wc=1e-3, l1=0.2), False: dict(lr=0.05, mmt=0.5, wc=1e-3, l1=0.2 / BUNCH)}


def matrices_of_first_component(text):
    """the text of the first component's matrices, split at their `m R C` headers"""
    head = text[:text.index("<sigmoid>")]
    parts = head.split("\nm ")
    return [parts[0]] + ["m " + p for p in parts[1:]]


@pytest.mark.parametrize("gdf", [True, False], ids=["graddivfrm", "nodiv"])
def test_component_train_write_read(gdf, tmp_path):
    k = CONSTS[gdf]
    text = net_text(sparse_net())
    assert text.startswith(f"<sparselinearity> {N_HID} {N_IN}\nm {N_HID} {N_IN}\n")
    net = make_net(text, gdf=gdf, **k)
    assert net.components()[0] == ("<sparselinearity>", N_IN, N_HID)
    net.keep_output(True)
    obj = Objective()
    ref = SparseOracle(formats.read_nnet(text))
    mask0 = ref.L[0].extra["mask"]
    W, b, mask, accu, nframes = net.sparse_params(0)
    np.testing.assert_array_equal(mask, mask0)
    np.testing.assert_array_equal(W, ref.L[0].W.astype(np.float32))
    assert nframes == 0 and not accu.any() and 0.35 < mask.mean() < 0.65
    corr_sum = np.zeros_like(ref.L[0].W)
    for X, lab in bunches(3, 61):
        net.train_bunch(obj, DeviceArray.from_numpy(X), DeviceArray.vector(lab))
        Yr = ref.step(X, lab, k["lr"], k["mmt"], k["wc"], k["l1"], gdf)
        corr_sum += ref.corr[0][0]
        np.testing.assert_allclose(net.output(3, BUNCH), Yr, rtol=2e-4, atol=2e-6)
        W, b, mask, accu, nframes = net.sparse_params(0)
        np.testing.assert_allclose(W, ref.L[0].W, rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(b, ref.L[0].b, rtol=2e-4, atol=2e-6)
        np.testing.assert_array_equal(mask, mask0)                        # updates never change the mask
        assert np.all(W[mask0 == 0] == 0.0)
        Wt, bt = net.get_params(2)
        np.testing.assert_allclose(Wt, ref.L[2].W, rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(bt, ref.L[2].b, rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(obj.stats()[0], ref.xent, rtol=1e-5)
    assert nframes == 3 * BUNCH == 99 == ref.nframes
    # accu is the sum of the three corrW
    np.testing.assert_array_equal(ref.accu[0], corr_sum)
    np.testing.assert_allclose(accu, corr_sum, rtol=2e-4, atol=2e-6)
    # the soft threshold took its share: active weights at exactly zero, and survivors of both signs
    assert (W[mask0 == 1] == 0).mean() > 0.05 and (W > 0).any() and (W < 0).any()

    # ---- write (UpdateMask runs first and changes the network), read back
    Wr = ref.L[0].W
    # the seed was picked so that no active reference weight lies within 1e-5 of the 1e-3 threshold: the rewritten
    # mask is then decided the same way in fp32 and in the restatement, and no element is excluded below
    assert not ((mask0 == 1) & (np.abs(np.abs(Wr) - 1e-3) < 1e-5)).any()
    Wcut, mask1 = mask_update_ref(Wr, mask0, ref.accu[0], 1e-3, 1e20, ref.nframes)
    assert (mask1 != mask0).any()                                         # the L1-zeroed weights are cut
    p1, p2, p3 = (str(tmp_path / f"sparse{i}.nnet") for i in (1, 2, 3))
    net.write(p1)
    W2, b2, mask2, accu2, nframes2 = net.sparse_params(0)
    np.testing.assert_array_equal(mask2, mask1)
    np.testing.assert_array_equal(W2, np.where(mask1 == 0, np.float32(0), W))
    np.testing.assert_array_equal(accu2, accu)                            # writing keeps accu and the count
    assert nframes2 == 99
    onfile = formats.read_nnet(p1)
    assert [l.tag for l in onfile] == ["<sparselinearity>", "<sigmoid>", "<biasedlinearity>", "<softmax>"]
    np.testing.assert_array_equal(onfile[0].extra["mask"], mask1)
    np.testing.assert_allclose(onfile[0].W, W2, rtol=1e-5, atol=1e-9)     # the writer's 6 digits
    np.testing.assert_allclose(onfile[0].extra["accu"], accu2, rtol=1e-5, atol=1e-9)
    back = Network(path=p1)
    W3, b3, mask3, accu3, nframes3 = back.sparse_params(0)
    np.testing.assert_array_equal(mask3, mask1)                           # the mask and the zeroed weights survive
    np.testing.assert_array_equal(W3, onfile[0].W)
    assert np.all(W3[mask1 == 0] == 0.0)
    np.testing.assert_array_equal(b3, onfile[0].b)
    assert not accu3.any() and nframes3 == 0                              # accu is read and dropped
    np.testing.assert_array_equal(back.get_params(2)[0], onfile[2].W)
    # a second writing of the same network: UpdateMask finds nothing more to do, the text is the same
    net.write(p2)
    assert open(p2).read() == open(p1).read()
    # a writing of the network read back: the same text apart from the accu matrix, which is zero now
    back.write(p3)
    t1, t3 = open(p1).read(), open(p3).read()
    m1, m3 = matrices_of_first_component(t1), matrices_of_first_component(t3)
    assert len(m1) == len(m3) == 4 and m1[:3] == m3[:3] and m1[3] != m3[3]
    assert t1[t1.index("<sigmoid>"):] == t3[t3.index("<sigmoid>"):]
    assert not formats.read_nnet(p3)[0].extra["accu"].any()


def test_file_without_mask_gives_all_ones_and_matches_biasedlinearity():
    """no mask matrix: every weight active; with l1 = 0, wc = 0 the layer then trains like a <biasedlinearity> of
    the same weights"""
    layers = sparse_net(seed=62, density=1.0)
    text = net_text(layers)
    assert len(matrices_of_first_component(text)) == 2                    # the header line and W^T only
    twin = [formats.Layer("<biasedlinearity>", l.n_out, l.n_in, l.W, l.b) if l.tag == "<sparselinearity>" else l
            for l in layers]
    a = make_net(text, 0.05, 0.5, 0.0, 0.0, True)
    b = make_net(net_text(twin), 0.05, 0.5, 0.0, 0.0, True)
    assert a.sparse_params(0)[2].all()
    oa, ob = Objective(), Objective()
    for X, lab in bunches(3, 63):
        a.train_bunch(oa, DeviceArray.from_numpy(X), DeviceArray.vector(lab))
        b.train_bunch(ob, DeviceArray.from_numpy(X), DeviceArray.vector(lab))
        Wa, ba = a.sparse_params(0)[:2]
        Wb, bb = b.get_params(0)
        np.testing.assert_allclose(Wa, Wb, rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(ba, bb, rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(a.get_params(2)[0], b.get_params(2)[0], rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(oa.stats()[0], ob.stats()[0], rtol=1e-5)
    assert a.sparse_params(0)[2].all() and a.sparse_params(0)[4] == 99


def test_set_l1_without_a_sparse_layer_changes_nothing():
    text = net_text(formats.gen_mlp_init([N_IN, N_HID, N_CLS], seed=64))
    nets = [make_net(text, 0.05, 0.5, 1e-3, l1, True) for l1 in (0.0, 0.3)]
    (X, lab), = bunches(1, 65)
    for n in nets:
        n.train_bunch(Objective(), DeviceArray.from_numpy(X), DeviceArray.vector(lab))
    for (Wa, ba), (Wb, bb) in zip(nets[0].linear_params(), nets[1].linear_params()):
        np.testing.assert_array_equal(Wa, Wb)
        np.testing.assert_array_equal(ba, bb)


def test_sparse_abi_set_get_and_wrong_component():
    net = Network(text=net_text(sparse_net(seed=66)))
    W, b, mask, accu, nframes = net.sparse_params(0)
    Wn, bn = rnd(W.shape, 67, 0.1), rnd(b.shape, 68)
    mn = draw_mask(mask.shape, 0.7, 69)
    net.set_sparse_params(0, mask=mn * 3.0)                               # nonzero -> 1; W is not touched
    W1, b1, m1 = net.sparse_params(0)[:3]
    np.testing.assert_array_equal(m1, mn)
    np.testing.assert_array_equal(W1, W)
    net.set_sparse_params(0, W=Wn)
    net.set_sparse_params(0, b=bn)
    W2, b2, m2 = net.sparse_params(0)[:3]
    np.testing.assert_array_equal(W2, Wn)
    np.testing.assert_array_equal(b2, bn)
    np.testing.assert_array_equal(m2, mn)
    with pytest.raises(ValueError):
        net.set_sparse_params(0, W=Wn[:, :-1])
    for call in (lambda: net.sparse_params(2), lambda: net.set_sparse_params(2, b=bn[:N_CLS]),
                 lambda: net.set_sparse_thresholds(2, 1e-3, 1.0), lambda: net.sparse_update_mask(2),
                 lambda: net.sparse_params(1), lambda: net.sparse_params(9), lambda: net.get_params(0)):
        with pytest.raises(TnetError):
            call()


def test_unsparsify_branch_through_the_thresholds():
    """a finite unsparsify_accu (no setter in the reference, so the branch is unreachable there): after one step
    sparse_update_mask turns on exactly the weights the restatement names, from the layer's own accu"""
    net = make_net(net_text(sparse_net(seed=70)), 0.05, 0.5, 0.0, 0.0, True)
    (X, lab), = bunches(1, 71)
    net.train_bunch(Objective(), DeviceArray.from_numpy(X), DeviceArray.vector(lab))
    W, b, mask, accu, nframes = net.sparse_params(0)
    assert nframes == BUNCH and accu.any()
    ratio = np.abs(accu) / np.float32(nframes)
    unsp = float(np.float32(np.median(ratio[mask == 0])))                 # about half of the inactive weights wake up
    net.set_sparse_thresholds(0, unsparsify_accu=unsp)                    # the sparsify threshold stays at 1e-3
    net.sparse_update_mask(0)
    Wr, mr = mask_update_ref(W, mask, accu, 1e-3, unsp, nframes)
    W2, _, mask2, accu2, nframes2 = net.sparse_params(0)
    np.testing.assert_array_equal(mask2, mr)
    np.testing.assert_array_equal(W2, Wr)
    woken = (mask == 0) & (mr == 1)
    assert 0.3 < woken.sum() / (mask == 0).sum() < 0.7
    np.testing.assert_array_equal(accu2, accu)
    assert nframes2 == nframes
    # a negative value leaves a threshold alone.  With the same thresholds a second UpdateMask cuts the woken
    # weights again: they are active now and still hold the zero they had under the mask (as in the reference, a
    # woken weight survives only if training moves it past the sparsify threshold before the next UpdateMask)
    net.set_sparse_thresholds(0, -1.0, -1.0)
    net.sparse_update_mask(0)
    Wr2, mr2 = mask_update_ref(Wr, mr, accu, 1e-3, unsp, nframes)
    assert not mr2[woken].any()
    W2b, _, mask2b = net.sparse_params(0)[:3]
    np.testing.assert_array_equal(mask2b, mr2)
    np.testing.assert_array_equal(W2b, Wr2)
    # ... and a sparsify threshold of 1 cuts every active weight
    net.set_sparse_thresholds(0, sparsify_threshold=1.0, unsparsify_accu=1e20)
    net.sparse_update_mask(0)
    W3, _, mask3 = net.sparse_params(0)[:3]
    assert not mask3.any() and not W3.any()


def test_trainer_epoch_over_a_synthetic_corpus():
    net = make_net(net_text(sparse_net(seed=72)), 0.05, 0.5, 1e-3, 0.02, True)
    obj = Objective()
    corpus = formats.synth_corpus(3, N_IN, N_CLS, seed=73, min_len=50, max_len=80)
    tr = Trainer(net, obj, bunchsize=32, cachesize=128, seed=1)
    tr.train_corpus(corpus.feats, corpus.labels)
    err, frames, _ = obj.stats()
    assert tr.steps >= 4 and frames >= 32 * 4 and np.isfinite(err) and err > 0
    W, b, mask, accu, nframes = net.sparse_params(0)
    assert nframes == frames and np.isfinite(W).all() and np.all(W[mask == 0] == 0.0)


HEAD = "<sparselinearity> 2 3\n"
WT = "m 2 3\n1 3 5\n2 4 6\n"


@pytest.mark.parametrize("text,msg", [
    (HEAD + "v 2 0 0\n", "Failed to read matrix"),
    (HEAD + "m 0 0\nv 2 0 0\n", "Missing linearity matrix in network file"),
    (HEAD + WT + "<sigmoid> 2 2\n", "Failed to read vector"),
    (HEAD + WT + "v 0\n", "Missing bias vector in network file"),
    ("<sparselinearity> 2 4\n" + WT + "v 2 0 0\n", "Wrong dimensionalities"),
    ("<sparselinearity> 3 3\n" + WT + "v 3 0 0 0\n", "Wrong dimensionalities"),
    (HEAD + WT + "v 3 0 0 0\n", "Wrong dimensionalities"),
    (HEAD + WT + "v 2 0 0\nm 3 2\n1 0\n0 1\n1 1\n", "sparsity mask"),
    (HEAD + WT + "v 2 0 0\nm 2 2\n1 0\n0 1\n", "sparsity mask"),
], ids=["no-matrix", "empty-matrix", "no-bias", "empty-bias", "n_in", "n_out", "bias-dim", "mask-transposed",
        "mask-narrow"])
def test_library_rejects_malformed_sparse_files(text, msg):
    with pytest.raises(TnetError, match=msg):
        Network(text=text)


def test_library_reads_the_optional_matrices():
    """mask and accu present, followed by another component: the look-ahead does not eat the next tag"""
    text = HEAD + WT + "v 2 0.5 -0.5\n\nm 2 3\n1 0 1\n0 1 1\nm 2 3\n9 9 9\n9 9 9\n<sigmoid> 2 2\n"
    net = Network(text=text)
    assert [c[0] for c in net.components()] == ["<sparselinearity>", "<sigmoid>"]
    W, b, mask, accu, nframes = net.sparse_params(0)
    np.testing.assert_array_equal(W, [[1, 2], [3, 4], [5, 6]])            # not masked at load, only by updates
    np.testing.assert_array_equal(mask, [[1, 0], [0, 1], [1, 1]])
    np.testing.assert_array_equal(b, [0.5, -0.5])
    assert not accu.any() and nframes == 0
