"""<discretelinearity>: the grouped kernels (tnet_discrete_fwd / _bwd / _update, one launch per direction over all
blocks), the component, its C ABI and file format.

The reference has no CPU twin of this layer (src/TNetLib holds Biased, Shared and BlockArray only), so nothing
here is pinned to reference output: parity is RESTATED against float64 numpy written in this file
(cuDiscreteLinearity.cc:9-78 under CuNetwork::Backpropagate).

Tolerances (tests/test_gpu_shared.py's):
  GEMM-shaped results  |got - ref| <= 2e-5 * (|A||B|) + 1e-6 against float64 numpy; the update's weight tolerance
                       is 2e-5 * |scale| * (|X_k|^T |E_k|) + 2e-7 * |W| + 1e-7
  bias results         rtol 1e-5 (absolute floors 1e-6 on the bias, 1e-5 on the sum)
  component level      rtol 2e-4 / atol 2e-6 per step; xent rtol 1e-5
"""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tnet_amd import DeviceArray, DiscretePlan, Network, Objective, Trainer, TnetError, formats  # noqa: E402
from tnet_amd._lib import MatrixDim, check, lib  # noqa: E402

ERR_ARG = -1

# (rows, [(in_k, out_k), ...]): a single element; one block; stripe origins off 16 bytes with one-column blocks;
# several ragged tiles per block (the prefix search crosses block borders); odd everything; 68 blocks (more than a
# kernel-argument table would hold, a deep search)
SHAPES = [
    (1, [(1, 1)]),
    (16, [(24, 16)]),
    (33, [(39, 10), (1, 7), (5, 3)]),
    (130, [(72, 136), (8, 8), (200, 40)]),
    (45, [(37, 50), (37, 50), (3, 129)]),
    (32, [(4, 4)] * 67 + [(7, 5)]),
]
# the 128x128 tile: forward / backward take it from 200 filled tiles on (3 tile rows x 68 tile columns here, odd
# widths), the update from 200 tiles of W (11 x 11 + 8 x 11, three row slices)
BIG_FB = (260, [(8519, 13), (13, 8519)])
BIG_UPD = (70, [(1300, 1290), (900, 1290)])
# the backward pass runs a per-block loop from bunch 512 where the grouped grid has fewer than 256 workgroups and the
# deepest out_k is at least 200 per block (gemm_discrete.hip loop_class): the measured ragged layer on both sides of
# the bunch threshold (its Eo stripes are off 16 bytes: the loop stages and scatters), on the other side of the depth
# threshold (596 < 3 * 200), and with aligned stripes (the loop writes Eo directly)
RAGGED = [(39, 64), (120, 256), (281, 704)]
LOOP_SHAPES = [(512, RAGGED), (508, RAGGED), (512, [(39, 64), (120, 256), (281, 596)]),
               (512, [(40, 64), (120, 256), (280, 704)])]
FB_SHAPES = SHAPES + [BIG_FB, BIG_UPD] + LOOP_SHAPES
UPD_SHAPES = SHAPES + [BIG_UPD]


def ids(shapes):
    return [f"{r}x{len(b)}blk-{b[0][0]}to{b[0][1]}-last{b[-1][0]}to{b[-1][1]}" for r, b in shapes]


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
    host = np.empty((d.rows, d.stride), np.float32)
    check(lib().tnet_memcpy_d2h(host.ctypes.data, d.ptr, host.nbytes), "d2h")
    return host


def padding_untouched(d):
    return bool(np.isnan(raw(d)[:, d.cols:]).all())


def stripes(M, widths):
    o = np.concatenate([[0], np.cumsum(widths)])
    return [M[:, o[k]:o[k + 1]].astype(np.float64) for k in range(len(widths))]


def gen_blocks(blocks, seed, scale=0.1):
    return [rnd(b, seed + 1000 * k, scale) for k, b in enumerate(blocks)]


def fwd_ref(X, Ws, b):
    xs = stripes(X, [W.shape[0] for W in Ws])
    z = np.concatenate([x @ W.astype(np.float64) for x, W in zip(xs, Ws)], axis=1) + b
    mag = np.concatenate([np.abs(x) @ np.abs(W.astype(np.float64)) for x, W in zip(xs, Ws)], axis=1)
    return z, mag


def bwd_ref(E, Ws):
    es = stripes(E, [W.shape[1] for W in Ws])
    z = np.concatenate([e @ W.astype(np.float64).T for e, W in zip(es, Ws)], axis=1)
    mag = np.concatenate([np.abs(e) @ np.abs(W.astype(np.float64)).T for e, W in zip(es, Ws)], axis=1)
    return z, mag


def upd_ref(X, E, blocks):
    xs, es = stripes(X, [b[0] for b in blocks]), stripes(E, [b[1] for b in blocks])
    g = [x.T @ e for x, e in zip(xs, es)]
    mag = [np.abs(x).T @ np.abs(e) for x, e in zip(xs, es)]
    return g, mag, E.astype(np.float64).sum(axis=0)


def packed_dev(plan, Ws):
    """the blocks on the device in the plan's layout, NaN in the stride padding"""
    return DeviceArray.vector(plan.pack(Ws, fill=np.nan))


def run_fwd(plan, dX, dW, db, dY):
    return lib().tnet_discrete_fwd(dX.ptr, dX.dim, dW.ptr, plan.ptr, db.ptr, dY.ptr, dY.dim, S())


def run_bwd(plan, dE, dW, dO):
    return lib().tnet_discrete_bwd(dE.ptr, dE.dim, dW.ptr, plan.ptr, dO.ptr, dO.dim, S())


# ------------------------------------------------------------------------------------ kernel level
def test_plan_layout():
    """every base 16-byte aligned, every stride a multiple of 4, blocks back to back"""
    blocks = [(39, 10), (1, 7), (5, 3), (72, 136)]
    plan = DiscretePlan(blocks)
    assert lib().tnet_discrete_plan_blocks(plan.ptr) == 4
    end = 0
    for (ni, no), (off, ld) in zip(blocks, plan.layout):
        assert off == end and off % 4 == 0 and ld % 4 == 0 and no <= ld < no + 4
        end = off + ni * ld
    assert plan.floats == end
    Ws = gen_blocks(blocks, 1)
    for W, U in zip(Ws, plan.unpack(plan.pack(Ws))):
        np.testing.assert_array_equal(W, U)


@pytest.mark.parametrize("rows,blocks", FB_SHAPES, ids=ids(FB_SHAPES))
def test_discrete_fwd(rows, blocks):
    plan = DiscretePlan(blocks)
    n_in, n_out = sum(b[0] for b in blocks), sum(b[1] for b in blocks)
    X, Ws, b = rnd((rows, n_in), 1), gen_blocks(blocks, 2), rnd(n_out, 3)
    dX, dW, db = DeviceArray.from_numpy(X), packed_dev(plan, Ws), DeviceArray.vector(b)
    dY = dev_nan_pad(np.full((rows, n_out), np.nan, np.float32))
    check(run_fwd(plan, dX, dW, db, dY), "discrete_fwd")
    z, mag = fwd_ref(X, Ws, b)
    err = np.abs(dY.numpy() - z)
    print("fwd max err / bound:", float((err / (2e-5 * mag + 1e-6)).max()))
    assert np.all(err <= 2e-5 * mag + 1e-6)
    assert padding_untouched(dY)


@pytest.mark.parametrize("rows,blocks", FB_SHAPES, ids=ids(FB_SHAPES))
def test_discrete_bwd(rows, blocks):
    plan = DiscretePlan(blocks)
    n_in, n_out = sum(b[0] for b in blocks), sum(b[1] for b in blocks)
    E, Ws = rnd((rows, n_out), 4), gen_blocks(blocks, 5)
    dE, dW = DeviceArray.from_numpy(E), packed_dev(plan, Ws)
    dO = dev_nan_pad(np.full((rows, n_in), np.nan, np.float32))  # beta 0: NaN in the output must not survive
    check(run_bwd(plan, dE, dW, dO), "discrete_bwd")
    z, mag = bwd_ref(E, Ws)
    got = dO.numpy()
    assert np.isfinite(got).all()                                # every column of Eo written
    err = np.abs(got - z)
    print("bwd max err / bound:", float((err / (2e-5 * mag + 1e-6)).max()))
    assert np.all(err <= 2e-5 * mag + 1e-6)
    assert padding_untouched(dO)


@pytest.mark.parametrize("rows,blocks", LOOP_SHAPES[:1] + LOOP_SHAPES[3:], ids=ids(LOOP_SHAPES[:1] + LOOP_SHAPES[3:]))
def test_discrete_bwd_loop_and_grouped_agree(rows, blocks):
    """the routed class both ways (tnet_discrete_loop_routing): each inside the float64 bound, padding untouched"""
    plan = DiscretePlan(blocks)
    n_in, n_out = sum(b[0] for b in blocks), sum(b[1] for b in blocks)
    E, Ws = rnd((rows, n_out), 40), gen_blocks(blocks, 41)
    dE, dW = DeviceArray.from_numpy(E), packed_dev(plan, Ws)
    z, mag = bwd_ref(E, Ws)
    outs = []
    try:
        for routing in (1, 0):
            lib().tnet_discrete_loop_routing(routing)
            dO = dev_nan_pad(np.full((rows, n_in), np.nan, np.float32))
            check(run_bwd(plan, dE, dW, dO), "discrete_bwd")
            outs.append(dO.numpy())
            assert np.all(np.abs(outs[-1] - z) <= 2e-5 * mag + 1e-6) and padding_untouched(dO)
    finally:
        assert lib().tnet_discrete_loop_routing(1) == 0
    np.testing.assert_allclose(outs[0], outs[1], rtol=0, atol=float((4e-5 * mag + 2e-6).max()))


def run_update(plan, X, E, Ws, corrs, b, cb, scale, mmt, l2, with_corr=True):
    dX, dE = DeviceArray.from_numpy(X), DeviceArray.from_numpy(E)
    dW, db = packed_dev(plan, Ws), DeviceArray.vector(b)
    dC = packed_dev(plan, corrs) if with_corr else None
    dcb = DeviceArray.vector(cb) if with_corr else None
    check(lib().tnet_discrete_update(dX.ptr, dX.dim, dE.ptr, dE.dim, plan.ptr, dW.ptr, dC.ptr if dC else None, db.ptr,
                                     dcb.ptr if dcb else None, scale, mmt, l2, S()), "discrete_update")
    return dW, dC, db, dcb


@pytest.mark.parametrize("mmt,with_corr", [(0.0, True), (0.5, True), (0.0, False)],
                         ids=["mmt0", "mmt0.5", "null-corr"])
@pytest.mark.parametrize("rows,blocks", UPD_SHAPES, ids=ids(UPD_SHAPES))
def test_discrete_update(rows, blocks, mmt, with_corr):
    plan = DiscretePlan(blocks)
    n_in, n_out = sum(b[0] for b in blocks), sum(b[1] for b in blocks)
    X, E = rnd((rows, n_in), 6), rnd((rows, n_out), 7, 0.01)
    Ws, corrs = gen_blocks(blocks, 8), gen_blocks(blocks, 9, 0.01)
    b, cb = rnd(n_out, 10), rnd(n_out, 11, 0.01)
    scale, l2 = -0.3 / rows, -1e-4
    dW, dC, db, dcb = run_update(plan, X, E, Ws, corrs, b, cb, scale, mmt, l2, with_corr)
    g, mag, gb = upd_ref(X, E, blocks)
    got_w = plan.unpack(dW.numpy())
    got_c = plan.unpack(dC.numpy()) if with_corr else None
    worst = 0.0
    for k, W in enumerate(Ws):
        # with momentum 0 the kernel still forms c = g + 0 * corr and stores it when the buffers are given
        c = g[k] + mmt * corrs[k] if with_corr else g[k]
        w = W + scale * c
        w = w + l2 * w
        tol = 2e-5 * abs(scale) * mag[k] + 2e-7 * np.abs(W) + 1e-7
        errw = np.abs(got_w[k] - w)
        worst = max(worst, float((errw / tol).max()))
        assert np.all(errw <= tol), k
        if with_corr:
            assert np.all(np.abs(got_c[k] - c) <= 2e-5 * mag[k] + 1e-6), k
    print("update W max err / tol:", worst)
    assert np.isnan(plan.padding(dW.numpy())).all()              # the stride padding is never written
    cbr = gb + mmt * cb if with_corr else gb
    np.testing.assert_allclose(db.numpy().reshape(-1), b + scale * cbr, rtol=1e-5, atol=1e-6)
    if with_corr:
        assert np.isnan(plan.padding(dC.numpy())).all()
        np.testing.assert_allclose(dcb.numpy().reshape(-1), cbr, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("rows,blocks", [SHAPES[2], SHAPES[3], BIG_UPD], ids=ids([SHAPES[2], SHAPES[3], BIG_UPD]))
def test_discrete_update_is_deterministic(rows, blocks):
    """no floating-point atomics: two runs on the same inputs give the same bits"""
    plan = DiscretePlan(blocks)
    n_in, n_out = sum(b[0] for b in blocks), sum(b[1] for b in blocks)
    X, E = rnd((rows, n_in), 12), rnd((rows, n_out), 13, 0.01)
    Ws, corrs = gen_blocks(blocks, 14), gen_blocks(blocks, 15, 0.01)
    b, cb = rnd(n_out, 16), rnd(n_out, 17, 0.01)
    outs = []
    for _ in range(2):
        d = run_update(plan, X, E, Ws, corrs, b, cb, -0.01, 0.5, -1e-4)
        outs.append([x.numpy() for x in d])
    for a, c in zip(*outs):
        np.testing.assert_array_equal(a, c)


def test_update_with_zero_rows_applies_momentum_and_decay():
    blocks = [(5, 3), (2, 6)]
    plan = DiscretePlan(blocks)
    Ws, corrs = gen_blocks(blocks, 18), gen_blocks(blocks, 19, 0.01)
    b, cb = rnd(9, 20), rnd(9, 21, 0.01)
    dX, dE = DeviceArray(0, 7), DeviceArray(0, 9)
    dW, dC, db, dcb = packed_dev(plan, Ws), packed_dev(plan, corrs), DeviceArray.vector(b), DeviceArray.vector(cb)
    scale, mmt, l2 = -0.1, 0.5, -1e-3
    check(lib().tnet_discrete_update(dX.ptr, MatrixDim(0, 7, 64), dE.ptr, MatrixDim(0, 9, 64), plan.ptr, dW.ptr, dC.ptr,
                                     db.ptr, dcb.ptr, scale, mmt, l2, S()), "discrete_update rows=0")
    for W, c0, got, gotc in zip(Ws, corrs, plan.unpack(dW.numpy()), plan.unpack(dC.numpy())):
        c = mmt * c0.astype(np.float64)
        w = W + scale * c
        np.testing.assert_allclose(got, w + l2 * w, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(gotc, c, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(db.numpy().reshape(-1), b + scale * mmt * cb.astype(np.float64), rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------------ cross-checks
def test_one_block_meets_the_affine_bounds():
    """one block: the three entry points against tnet_affine_fwd, tnet_sgemm('N','T') and tnet_affine_update on the
    same data (both sides inside the same float64 bounds)"""
    rows, n_in, n_out = 130, 72, 136
    plan = DiscretePlan([(n_in, n_out)])
    X, E = rnd((rows, n_in), 22), rnd((rows, n_out), 23, 0.01)
    W, b = rnd((n_in, n_out), 24, 0.1), rnd(n_out, 25)
    dX, dE, dW, db = (DeviceArray.from_numpy(X), DeviceArray.from_numpy(E), DeviceArray.from_numpy(W),
                      DeviceArray.vector(b))
    dP = DeviceArray.vector(plan.pack([W]))
    z, mag = fwd_ref(X, [W], b)
    ys = [DeviceArray(rows, n_out), DeviceArray(rows, n_out)]
    check(run_fwd(plan, dX, dP, db, ys[0]))
    check(lib().tnet_affine_fwd(dX.ptr, dX.dim, dW.ptr, dW.dim, db.ptr, ys[1].ptr, ys[1].dim, 0, S()))
    for y in ys:
        assert np.all(np.abs(y.numpy() - z) <= 2e-5 * mag + 1e-6)
    z, mag = bwd_ref(E, [W])
    os_ = [DeviceArray(rows, n_in), DeviceArray(rows, n_in)]
    check(run_bwd(plan, dE, dP, os_[0]))
    check(lib().tnet_sgemm(b"N", b"T", rows, n_in, n_out, 1.0, dE.ptr, dE.stride, dW.ptr, dW.stride, 0.0, os_[1].ptr,
                           os_[1].stride, S()))
    for o in os_:
        assert np.all(np.abs(o.numpy() - z) <= 2e-5 * mag + 1e-6)
    scale, l2 = -0.3 / rows, -1e-4
    g, mag, gb = upd_ref(X, E, [(n_in, n_out)])
    w = W + scale * g[0]
    w = w + l2 * w
    tol = 2e-5 * abs(scale) * mag[0] + 2e-7 * np.abs(W) + 1e-7
    check(lib().tnet_discrete_update(dX.ptr, dX.dim, dE.ptr, dE.dim, plan.ptr, dP.ptr, None, db.ptr, None, scale, 0.0,
                                     l2, S()))
    check(lib().tnet_affine_update(dX.ptr, dX.dim, dE.ptr, dE.dim, dW.ptr, dW.dim, None, 0, scale, 0.0, l2, S()))
    for got in (plan.unpack(dP.numpy())[0], dW.numpy()):
        assert np.all(np.abs(got - w) <= tol)
    np.testing.assert_allclose(db.numpy().reshape(-1), b + scale * gb, rtol=1e-5, atol=1e-6)


def test_equal_blocks_meet_the_shared_bounds():
    """N equal blocks carrying the same W: forward / backward against tnet_shared_fwd / _bwd on the same data (the
    shared layer's bias is one block's; the discrete layer gets it tiled)"""
    rows, n, n_in, n_out = 33, 11, 39, 10
    plan = DiscretePlan([(n_in, n_out)] * n)
    X, E = rnd((rows, n * n_in), 26), rnd((rows, n * n_out), 27)
    W, b = rnd((n_in, n_out), 28, 0.1), rnd(n_out, 29)
    dX, dE, dW, db = (DeviceArray.from_numpy(X), DeviceArray.from_numpy(E), DeviceArray.from_numpy(W),
                      DeviceArray.vector(b))
    dP, dbt = DeviceArray.vector(plan.pack([W] * n)), DeviceArray.vector(np.tile(b, n))
    z, mag = fwd_ref(X, [W] * n, np.tile(b, n))
    ys = [DeviceArray(rows, n * n_out), DeviceArray(rows, n * n_out)]
    check(run_fwd(plan, dX, dP, dbt, ys[0]))
    check(lib().tnet_shared_fwd(dX.ptr, dX.dim, dW.ptr, dW.dim, db.ptr, n, ys[1].ptr, ys[1].dim, S()))
    for y in ys:
        assert np.all(np.abs(y.numpy() - z) <= 2e-5 * mag + 1e-6)
    z, mag = bwd_ref(E, [W] * n)
    os_ = [DeviceArray(rows, n * n_in), DeviceArray(rows, n * n_in)]
    check(run_bwd(plan, dE, dP, os_[0]))
    check(lib().tnet_shared_bwd(dE.ptr, dE.dim, dW.ptr, dW.dim, n, os_[1].ptr, os_[1].dim, S()))
    for o in os_:
        assert np.all(np.abs(o.numpy() - z) <= 2e-5 * mag + 1e-6)


def block_diag(Ws):
    D = np.zeros((sum(W.shape[0] for W in Ws), sum(W.shape[1] for W in Ws)), np.float32)
    r = c = 0
    for W in Ws:
        D[r:r + W.shape[0], c:c + W.shape[1]] = W
        r, c = r + W.shape[0], c + W.shape[1]
    return D


def test_fwd_bwd_equal_a_biasedlinearity_with_the_block_diagonal_matrix():
    """the layer against a <biasedlinearity> holding the block-diagonal matrix: forward through both components,
    backward through the kernels each component calls (the zeros add nothing to |A||B|, so one bound serves both)"""
    rows, blocks = 45, [(37, 50), (37, 50), (3, 129)]
    layer = formats.gen_discrete_init([b[0] for b in blocks], [b[1] for b in blocks], seed=30, negbias=False)[0]
    layer.b = rnd(layer.n_out, 31)
    Ws, D = layer.extra["Ws"], block_diag(layer.extra["Ws"])
    dense = formats.Layer("<biasedlinearity>", layer.n_out, layer.n_in, D, layer.b)
    X, E = rnd((rows, layer.n_in), 32), rnd((rows, layer.n_out), 33)
    dX, dE = DeviceArray.from_numpy(X), DeviceArray.from_numpy(E)
    z, mag = fwd_ref(X, Ws, layer.b)
    for net in (Network.from_layers([layer]), Network.from_layers([dense])):
        assert np.all(np.abs(net.propagate(dX).numpy() - z) <= 2e-5 * mag + 1e-6)
    plan = DiscretePlan(blocks)
    dP, dD = DeviceArray.vector(plan.pack(Ws)), DeviceArray.from_numpy(D)
    z, mag = bwd_ref(E, Ws)
    os_ = [DeviceArray(rows, layer.n_in), DeviceArray(rows, layer.n_in)]
    check(run_bwd(plan, dE, dP, os_[0]))
    check(lib().tnet_sgemm(b"N", b"T", rows, layer.n_in, layer.n_out, 1.0, dE.ptr, dE.stride, dD.ptr, dD.stride, 0.0,
                           os_[1].ptr, os_[1].stride, S()))
    for o in os_:
        assert np.all(np.abs(o.numpy() - z) <= 2e-5 * mag + 1e-6)


# --------------------------------------------------------------------------------- component level
DIMS_IN, DIMS_OUT = [20, 7, 9], [12, 5, 8]


def discrete_net(seed=50):
    """(20, 7, 9) -> (12, 5, 8) discrete, sigmoid, 25 -> 9 affine, softmax.  Zero bias in the discrete layer: with
    the --negbias draw (-4) its sigmoids sit at 0.02 and the gradients reaching it would test little."""
    return formats.gen_discrete_init(DIMS_IN, DIMS_OUT, seed=seed, negbias=False) + \
        formats.gen_mlp_init([25, 9], seed=seed + 1)


class DiscreteOracle:
    """float64 restatement of the GPU semantics: CuDiscreteLinearity::Update (cuDiscreteLinearity.cc:45-78) and
    CuBiasedLinearity::Update (cuBiasedLinearity.cc:46-64) under CuNetwork::Backpropagate"""

    def __init__(self, layers):
        self.L = layers
        for l in self.L:
            l.b = None if l.b is None else l.b.astype(np.float64)
            l.W = None if l.W is None else l.W.astype(np.float64)
            if "Ws" in l.extra:
                l.extra["Ws"] = [W.astype(np.float64) for W in l.extra["Ws"]]
        self.corr = {}
        for k, l in enumerate(self.L):
            if l.tag == "<discretelinearity>":
                self.corr[k] = ([np.zeros_like(W) for W in l.extra["Ws"]], np.zeros_like(l.b))
            elif l.W is not None:
                self.corr[k] = (np.zeros_like(l.W), np.zeros_like(l.b))
        self.xent = 0.0

    def forward(self, X):
        acts = [np.asarray(X, np.float64)]
        for l in self.L:
            a = acts[-1]
            if l.tag == "<biasedlinearity>":
                a = a @ l.W + l.b
            elif l.tag == "<discretelinearity>":
                Ws = l.extra["Ws"]
                a = np.concatenate([x @ W for x, W in zip(stripes(a, [W.shape[0] for W in Ws]), Ws)], axis=1) + l.b
            elif l.tag == "<sigmoid>":
                a = 1.0 / (1.0 + np.exp(-a))
            elif l.tag == "<softmax>":
                e = np.exp(a - a.max(axis=1, keepdims=True))
                a = e / e.sum(axis=1, keepdims=True)
            acts.append(a)
        return acts

    def step(self, X, lab, lr, mmt, wc, gdf):
        acts = self.forward(X)
        Y = acts[-1]
        rows = len(lab)
        self.xent += -np.log(Y[np.arange(rows), lab]).sum()
        err = Y.copy()
        err[np.arange(rows), lab] -= 1.0
        ndiv = (rows if gdf else 1.0) / (1.0 - mmt)
        for k in range(len(self.L) - 1, -1, -1):
            l, a_in = self.L[k], acts[k]
            if l.tag == "<sigmoid>":
                err = err * acts[k + 1] * (1.0 - acts[k + 1])
            elif l.tag == "<discretelinearity>":
                Ws = l.extra["Ws"]
                e_in = err
                es = stripes(e_in, [W.shape[1] for W in Ws])
                xs = stripes(a_in, [W.shape[0] for W in Ws])
                err = np.concatenate([e @ W.T for e, W in zip(es, Ws)], axis=1)   # pre-update weights
                cws, cb = self.corr[k]
                for j in range(len(Ws)):
                    cws[j] = xs[j].T @ es[j] + mmt * cws[j]
                    Ws[j] = Ws[j] + (-lr / ndiv) * cws[j]                         # no block-count factor
                    Ws[j] = Ws[j] + (-lr * wc) * Ws[j]                            # no rows factor
                cb = e_in.sum(axis=0) + mmt * cb
                self.corr[k] = (cws, cb)
                l.b = l.b + (-lr / ndiv) * cb                                     # no weight decay on the bias
            elif l.W is not None:
                e_in = err
                err = e_in @ l.W.T
                cw, cb = self.corr[k]
                cw, cb = a_in.T @ e_in + mmt * cw, e_in.sum(axis=0) + mmt * cb
                self.corr[k] = (cw, cb)
                l.W = l.W + (-lr / ndiv) * cw
                l.W = l.W + (-lr * wc * (1.0 if gdf else rows)) * l.W
                l.b = l.b + (-lr / ndiv) * cb
        return Y


def make_net(text, lr, mmt, wc, gdf):
    net = Network(text=text)
    net.set_learn_rate(lr)
    net.set_momentum(mmt)
    net.set_weightcost(wc)
    net.set_grad_div_frm(gdf)
    return net


@pytest.mark.parametrize("mmt,wc,gdf", [(0.0, 0.0, False), (0.9, 1e-3, True), (0.0, 1e-3, False), (0.9, 0.0, True)])
def test_component_train_bunch_vs_restatement(mmt, wc, gdf):
    buf = io.StringIO()
    formats.write_nnet(discrete_net(), buf, precision=9)
    lr = 0.05
    net = make_net(buf.getvalue(), lr, mmt, wc, gdf)
    assert net.components()[0] == ("<discretelinearity>", 36, 25)
    assert net.discrete_blocks(0) == list(zip(DIMS_IN, DIMS_OUT))
    net.keep_output(True)
    obj = Objective()
    ref = DiscreteOracle(formats.read_nnet(buf.getvalue()))
    rng = np.random.default_rng(51)
    B = 32
    for s in range(3):
        X = rng.standard_normal((B, 36)).astype(np.float32)
        lab = rng.integers(0, 9, B).astype(np.int32)
        net.train_bunch(obj, DeviceArray.from_numpy(X), DeviceArray.vector(lab))
        Yr = ref.step(X, lab, lr, mmt, wc, gdf)
        np.testing.assert_allclose(net.output(3, B), Yr, rtol=2e-4, atol=2e-6)
        Ws, b = net.discrete_params(0)
        for W, Wr in zip(Ws, ref.L[0].extra["Ws"]):
            np.testing.assert_allclose(W, Wr, rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(b, ref.L[0].b, rtol=2e-4, atol=2e-6)
        Wt, bt = net.get_params(2)
        np.testing.assert_allclose(Wt, ref.L[2].W, rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(bt, ref.L[2].b, rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(obj.stats()[0], ref.xent, rtol=1e-5)


def test_trainer_reproduces_train_bunch_and_replays():
    """Trainer (cache + generic step, randomize off) over the same net: the parameters of four train_bunch steps;
    replay serves this non-fusable network too and advances them"""
    buf = io.StringIO()
    formats.write_nnet(discrete_net(53), buf, precision=9)
    B, lr = 32, 0.05
    rng = np.random.default_rng(54)
    X = rng.standard_normal((4 * B, 36)).astype(np.float32)
    lab = rng.integers(0, 9, 4 * B).astype(np.int32)
    a, oa = make_net(buf.getvalue(), lr, 0.0, 0.0, False), Objective()
    for s in range(4):
        a.train_bunch(oa, DeviceArray.from_numpy(X[s * B:(s + 1) * B]), DeviceArray.vector(lab[s * B:(s + 1) * B]))
    b, ob = make_net(buf.getvalue(), lr, 0.0, 0.0, False), Objective()
    tr = Trainer(b, ob, bunchsize=B, cachesize=4 * B, seed=1, randomize=False)
    tr.add_utterance(X, lab)
    tr.finish()
    assert tr.steps == 4
    (Wa, ba), (Wb, bb) = a.discrete_params(0), b.discrete_params(0)
    for U, V in zip(Wa, Wb):
        np.testing.assert_allclose(V, U, rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(bb, ba, rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(b.get_params(2)[0], a.get_params(2)[0], rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(ob.stats()[0], oa.stats()[0], rtol=1e-5)
    tr.replay(2)
    assert tr.steps == 6
    W6 = b.discrete_params(0)[0]
    assert all(np.isfinite(W).all() for W in W6) and not np.array_equal(W6[0], Wb[0])


# ------------------------------------------------------------------------- ABI and file round trip
def test_discrete_params_abi_and_write_read(tmp_path):
    """set / get through the C ABI; a written file read back holds the same parameters bit for bit (parameters that
    6 significant digits -- the writer's precision -- represent exactly)"""
    layers = formats.round_trip_text(discrete_net(52), 6)
    net = Network.from_layers(layers, precision=6)
    Ws, b = net.discrete_params(0)
    assert [W.shape for W in Ws] == [(20, 12), (7, 5), (9, 8)] and b.shape == (25,)
    for W, W0 in zip(Ws, layers[0].extra["Ws"]):
        np.testing.assert_array_equal(W, W0)
    np.testing.assert_array_equal(b, layers[0].b)
    p = str(tmp_path / "discrete.nnet")
    net.write(p)
    back = Network(path=p)
    Ws2, b2 = back.discrete_params(0)
    for W, W2 in zip(Ws, Ws2):
        np.testing.assert_array_equal(W2, W)
    np.testing.assert_array_equal(b2, b)
    np.testing.assert_array_equal(back.get_params(2)[0], net.get_params(2)[0])
    again = formats.read_nnet(p)
    assert again[0].tag == "<discretelinearity>" and len(again[0].extra["Ws"]) == 3
    for W, W2 in zip(Ws, again[0].extra["Ws"]):
        np.testing.assert_array_equal(W2, W)
    np.testing.assert_array_equal(again[0].b, b)
    W1n, bn = (Ws[1] * 2).astype(np.float32), (b + 1).astype(np.float32)
    net.set_discrete_params(0, [None, W1n, None], None)
    got, gb = net.discrete_params(0)
    np.testing.assert_array_equal(got[1], W1n)
    np.testing.assert_array_equal(got[0], Ws[0])
    np.testing.assert_array_equal(got[2], Ws[2])
    np.testing.assert_array_equal(gb, b)
    net.set_discrete_params(0, None, bn)
    np.testing.assert_array_equal(net.discrete_params(0)[1], bn)
    with pytest.raises(ValueError):
        net.set_discrete_params(0, [Ws[0]], None)
    with pytest.raises(TnetError):
        net.discrete_params(2)     # a <biasedlinearity>
    with pytest.raises(TnetError):
        net.get_params(0)          # get_params stays <biasedlinearity>-only


@pytest.mark.parametrize("text,msg", [
    ("<discretelinearity> 3 4\n0\nm 2 3\n1 3 5\n2 4 6\n", "Bad number of blocks"),
    ("<discretelinearity> 3 4\n2\nm 2 3\n1 3 5\n2 4 6\nm 0 0\nv 3 0 0 0\n", "Missing linearity matrix in network file"),
    ("<discretelinearity> 3 4\n2\nm 2 3\n1 3 5\n2 4 6\nm 1 1\n0.5\nv 0\n", "Missing bias vector in network file"),
    ("<discretelinearity> 3 5\n2\nm 2 3\n1 3 5\n2 4 6\nm 1 1\n0.5\nv 3 0 0 0\n", "Wrong dimensionalities"),
    ("<discretelinearity> 4 4\n2\nm 2 3\n1 3 5\n2 4 6\nm 1 1\n0.5\nv 4 0 0 0 0\n", "Wrong dimensionalities"),
    ("<discretelinearity> 3 4\n2\nm 2 3\n1 3 5\n2 4 6\nm 1 1\n0.5\nv 2 0 0\n", "Wrong dimensionalities"),
])
def test_library_rejects_malformed_discrete_files(text, msg):
    with pytest.raises(TnetError, match=msg):
        Network(text=text)


# --------------------------------------------------------------------------------- argument errors
def test_argument_errors_return_err_arg():
    """refused before any launch (argument checks only: nothing here reaches a kernel)"""
    L = lib()
    rows, blocks = 8, [(8, 4), (4, 8)]
    plan = DiscretePlan(blocks)
    X, E, Y, Eo = DeviceArray(rows, 12), DeviceArray(rows, 12), DeviceArray(rows, 12), DeviceArray(rows, 12)
    Wp = DeviceArray.vector(np.zeros(plan.floats, np.float32))
    Cp = DeviceArray.vector(np.zeros(plan.floats, np.float32))
    b, cb = DeviceArray.vector(np.zeros(12, np.float32)), DeviceArray.vector(np.zeros(12, np.float32))
    good, s = MatrixDim(rows, 12, 64), S()

    def fwd(x=X.ptr, dx=good, w=Wp.ptr, pl=plan.ptr, bias=b.ptr, y=Y.ptr, dy=good):
        return L.tnet_discrete_fwd(x, dx, w, pl, bias, y, dy, s)

    def bwd(e=E.ptr, de=good, w=Wp.ptr, pl=plan.ptr, eo=Eo.ptr, deo=good):
        return L.tnet_discrete_bwd(e, de, w, pl, eo, deo, s)

    def upd(x=X.ptr, dx=good, e=E.ptr, de=good, pl=plan.ptr, w=Wp.ptr, c=Cp.ptr, bias=b.ptr, cbias=cb.ptr, mmt=0.5):
        return L.tnet_discrete_update(x, dx, e, de, pl, w, c, bias, cbias, -0.1, mmt, 0.0, s)

    assert fwd() == 0 and bwd() == 0 and upd() == 0
    # NULL or mis-sized
    assert fwd(x=None) == ERR_ARG and fwd(w=None) == ERR_ARG and fwd(pl=None) == ERR_ARG and fwd(bias=None) == ERR_ARG
    assert fwd(y=None) == ERR_ARG and bwd(eo=None) == ERR_ARG and upd(e=None) == ERR_ARG and upd(pl=None) == ERR_ARG
    assert fwd(dx=MatrixDim(rows, 12, 8)) == ERR_ARG                     # stride < cols
    # a stride that is no multiple of 4
    assert fwd(dx=MatrixDim(rows, 12, 62)) == ERR_ARG and fwd(dy=MatrixDim(rows, 12, 50)) == ERR_ARG
    assert bwd(de=MatrixDim(rows, 12, 62)) == ERR_ARG and bwd(deo=MatrixDim(rows, 12, 13)) == ERR_ARG
    assert upd(dx=MatrixDim(rows, 12, 62)) == ERR_ARG and upd(de=MatrixDim(rows, 12, 18)) == ERR_ARG
    # wrong column counts
    assert fwd(dx=MatrixDim(rows, 13, 64)) == ERR_ARG and fwd(dy=MatrixDim(rows, 11, 64)) == ERR_ARG
    assert bwd(de=MatrixDim(rows, 11, 64)) == ERR_ARG and bwd(deo=MatrixDim(rows, 13, 64)) == ERR_ARG
    assert upd(dx=MatrixDim(rows, 8, 64)) == ERR_ARG and upd(de=MatrixDim(rows, 16, 64)) == ERR_ARG
    # a row-count mismatch
    assert fwd(dy=MatrixDim(rows - 1, 12, 64)) == ERR_ARG and bwd(deo=MatrixDim(rows + 1, 12, 64)) == ERR_ARG
    assert upd(de=MatrixDim(rows - 1, 12, 64)) == ERR_ARG
    # parameter buffers overlapping activations, activations overlapping each other
    assert fwd(w=X.ptr) == ERR_ARG and fwd(w=Y.ptr) == ERR_ARG and fwd(w=X.ptr + 64) == ERR_ARG
    assert fwd(y=X.ptr) == ERR_ARG and fwd(bias=Y.ptr) == ERR_ARG
    assert bwd(w=E.ptr) == ERR_ARG and bwd(w=Eo.ptr) == ERR_ARG and bwd(eo=E.ptr) == ERR_ARG
    assert upd(w=X.ptr) == ERR_ARG and upd(w=E.ptr) == ERR_ARG and upd(c=X.ptr) == ERR_ARG and upd(c=E.ptr) == ERR_ARG
    assert upd(c=Wp.ptr) == ERR_ARG and upd(bias=E.ptr) == ERR_ARG and upd(cbias=X.ptr) == ERR_ARG
    # parameter buffers overlapping each other
    assert upd(bias=Wp.ptr + 16) == ERR_ARG and upd(cbias=Wp.ptr) == ERR_ARG and upd(bias=Cp.ptr) == ERR_ARG
    assert upd(cbias=Cp.ptr + 32) == ERR_ARG and upd(cbias=b.ptr) == ERR_ARG
    # NULL correction buffers exactly when mmt == 0
    assert upd(c=None) == ERR_ARG and upd(cbias=None) == ERR_ARG
    assert upd(c=None, cbias=None, mmt=0.0) == 0
