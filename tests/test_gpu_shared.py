"""<sharedlinearity> / <blockarray>: the instance-batched kernels (tnet_shared_fwd / _bwd / _update), the two
components, and the pins to the reference CPU TNet (tests/golden/make_shared.py).

Tolerances (tests/test_gpu_kernels.py):
  GEMM-shaped results  |got - ref| <= 2e-5 * (|A||B|) + 1e-6 against float64 numpy (N * rows <= 4096); for the
                       update (|A||B|) = sum_i |X_i|^T |E_i| and the weight tolerance is test_affine_update's
  bias results         rtol 1e-5 (reductions; absolute floors 1e-5 on the sum, 1e-6 on the bias, as test_col_sum)
  component level      rtol 2e-4 / atol 2e-6 per step (tests/test_gpu_train.py)
  reference pins       rtol 2e-4; atol 2e-6 outputs, 1e-6 parameters; xent rtol 1e-5
"""
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from golden_io import load_npz  # noqa: E402
from tnet_amd import DeviceArray, Network, Objective, Trainer, TnetError, formats  # noqa: E402
from tnet_amd._lib import check, lib  # noqa: E402

# (rows, N, in, out): a single element; the fixture's layer; unaligned windows (N*in = 429 is not the pitch);
# several tiles per instance with ragged edges; odd everything; a deep K with whole 64x64 tiles (pick_tile counts
# cdiv(M,128) * cdiv(N,128) * batch = 10 forward, 40 backward, 20 for the update: below the 200 from which the
# 128x128 tile runs -- tests/test_gpu_layer_views.py reaches that one, through the batch)
SHAPES = [(1, 1, 1, 1), (16, 3, 24, 16), (33, 11, 39, 10), (130, 5, 72, 136), (45, 2, 37, 50), (256, 5, 440, 128)]


# forward / backward also at the size from which they run the per-instance loop (rows * in * out = 2^28, aligned
# windows) and just below it (the batched launch)
FB_SHAPES = SHAPES + [(1024, 2, 512, 512), (1020, 2, 512, 512)]


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


def windows(M, n, w):
    return [M[:, i * w:(i + 1) * w].astype(np.float64) for i in range(n)]


def fwd_ref(X, W, b, n):
    W64 = W.astype(np.float64)
    z = np.concatenate([x @ W64 + b for x in windows(X, n, W.shape[0])], axis=1)
    mag = np.concatenate([np.abs(x) @ np.abs(W64) for x in windows(X, n, W.shape[0])], axis=1)
    return z, mag


def bwd_ref(E, W, n):
    Wt = W.astype(np.float64).T
    z = np.concatenate([e @ Wt for e in windows(E, n, W.shape[1])], axis=1)
    mag = np.concatenate([np.abs(e) @ np.abs(Wt) for e in windows(E, n, W.shape[1])], axis=1)
    return z, mag


def upd_ref(X, E, n, n_in, n_out):
    xs, es = windows(X, n, n_in), windows(E, n, n_out)
    g = sum(x.T @ e for x, e in zip(xs, es))
    mag = sum(np.abs(x).T @ np.abs(e) for x, e in zip(xs, es))
    gb = sum(e.sum(axis=0) for e in es)
    magb = sum(np.abs(e).sum(axis=0) for e in es)
    return g, mag, gb, magb


# ------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("rows,n,n_in,n_out", FB_SHAPES)
def test_shared_fwd(rows, n, n_in, n_out):
    X, W, b = rnd((rows, n * n_in), 1), rnd((n_in, n_out), 2, 0.1), rnd(n_out, 3)
    dX, dW, db = DeviceArray.from_numpy(X), DeviceArray.from_numpy(W), DeviceArray.vector(b)
    dY = dev_nan_pad(np.full((rows, n * n_out), np.nan, np.float32))
    check(lib().tnet_shared_fwd(dX.ptr, dX.dim, dW.ptr, dW.dim, db.ptr, n, dY.ptr, dY.dim, S()), "shared_fwd")
    z, mag = fwd_ref(X, W, b, n)
    err = np.abs(dY.numpy() - z)
    print("fwd max err / bound:", float((err / (2e-5 * mag + 1e-6)).max()))
    assert np.all(err <= 2e-5 * mag + 1e-6)
    assert padding_untouched(dY)


@pytest.mark.parametrize("rows,n,n_in,n_out", FB_SHAPES)
def test_shared_bwd(rows, n, n_in, n_out):
    E, W = rnd((rows, n * n_out), 4), rnd((n_in, n_out), 5, 0.1)
    dE, dW = DeviceArray.from_numpy(E), DeviceArray.from_numpy(W)
    dO = dev_nan_pad(np.full((rows, n * n_in), np.nan, np.float32))  # beta 0: garbage in the output is ignored
    check(lib().tnet_shared_bwd(dE.ptr, dE.dim, dW.ptr, dW.dim, n, dO.ptr, dO.dim, S()), "shared_bwd")
    z, mag = bwd_ref(E, W, n)
    err = np.abs(dO.numpy() - z)
    print("bwd max err / bound:", float((err / (2e-5 * mag + 1e-6)).max()))
    assert np.all(err <= 2e-5 * mag + 1e-6)
    assert padding_untouched(dO)


def run_update(X, E, W, corr, b, cb, n, scale, mmt, l2, with_corr=True):
    dX, dE = DeviceArray.from_numpy(X), DeviceArray.from_numpy(E)
    dW, db = dev_nan_pad(W), DeviceArray.vector(b)
    dC = dev_nan_pad(corr) if with_corr else None
    dcb = DeviceArray.vector(cb) if with_corr else None
    check(lib().tnet_shared_update(dX.ptr, dX.dim, dE.ptr, dE.dim, n, dW.ptr, dW.dim, dC.ptr if dC else None,
                                   dC.stride if dC else 0, db.ptr, dcb.ptr if dcb else None, scale, mmt, l2, S()),
          "shared_update")
    return dW, dC, db, dcb


@pytest.mark.parametrize("mmt,with_corr", [(0.0, True), (0.5, True), (0.0, False)],
                         ids=["mmt0", "mmt0.5", "null-corr"])
@pytest.mark.parametrize("rows,n,n_in,n_out", SHAPES)
def test_shared_update(rows, n, n_in, n_out, mmt, with_corr):
    X, E = rnd((rows, n * n_in), 6), rnd((rows, n * n_out), 7, 0.01)
    W, corr = rnd((n_in, n_out), 8, 0.1), rnd((n_in, n_out), 9, 0.01)
    b, cb = rnd(n_out, 10), rnd(n_out, 11, 0.01)
    scale, l2 = -0.3 / (rows * n), -1e-4
    dW, dC, db, dcb = run_update(X, E, W, corr, b, cb, n, scale, mmt, l2, with_corr)
    g, mag, gb, _ = upd_ref(X, E, n, n_in, n_out)
    # with momentum 0 the kernel still forms c = g + 0 * corr and stores it when the buffers are given
    c = g + mmt * corr if with_corr else g
    w = W + scale * c
    w = w + l2 * w
    tol = 2e-5 * abs(scale) * mag + 2e-7 * np.abs(W) + 1e-7
    errw = np.abs(dW.numpy() - w)
    print("update W max err / tol:", float((errw / tol).max()))
    assert np.all(errw <= tol)
    assert padding_untouched(dW)
    cbr = gb + mmt * cb if with_corr else gb
    # reductions tolerance: rtol 1e-5 with test_col_sum's absolute floors (1e-5 on the sum, 1e-6 on the bias)
    np.testing.assert_allclose(db.numpy().reshape(-1), b + scale * cbr, rtol=1e-5, atol=1e-6)
    if with_corr:
        assert np.all(np.abs(dC.numpy() - c) <= 2e-5 * mag + 1e-6)
        assert padding_untouched(dC)
        np.testing.assert_allclose(dcb.numpy().reshape(-1), cbr, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("rows,n,n_in,n_out", [(33, 11, 39, 10), (256, 5, 440, 128)])
def test_shared_update_is_deterministic(rows, n, n_in, n_out):
    """no floating-point atomics: two runs on the same inputs give the same bits"""
    X, E = rnd((rows, n * n_in), 12), rnd((rows, n * n_out), 13, 0.01)
    W, corr = rnd((n_in, n_out), 14, 0.1), rnd((n_in, n_out), 15, 0.01)
    b, cb = rnd(n_out, 16), rnd(n_out, 17, 0.01)
    outs = []
    for _ in range(2):
        d = run_update(X, E, W, corr, b, cb, n, -0.01, 0.5, -1e-4)
        outs.append([x.numpy() for x in d])
    for a, c in zip(*outs):
        np.testing.assert_array_equal(a, c)


def test_shared_n1_meets_the_affine_bounds():
    """N = 1: the three entry points against the bounds of tnet_affine_fwd, tnet_sgemm('N','T') and
    tnet_affine_update on the same data (both sides checked against the same float64 reference)"""
    rows, n_in, n_out = 130, 72, 136
    X, E = rnd((rows, n_in), 18), rnd((rows, n_out), 19, 0.01)
    W, b = rnd((n_in, n_out), 20, 0.1), rnd(n_out, 21)
    dX, dE, dW, db = (DeviceArray.from_numpy(X), DeviceArray.from_numpy(E), DeviceArray.from_numpy(W),
                      DeviceArray.vector(b))
    z, mag = fwd_ref(X, W, b, 1)
    ys = [DeviceArray(rows, n_out), DeviceArray(rows, n_out)]
    check(lib().tnet_shared_fwd(dX.ptr, dX.dim, dW.ptr, dW.dim, db.ptr, 1, ys[0].ptr, ys[0].dim, S()))
    check(lib().tnet_affine_fwd(dX.ptr, dX.dim, dW.ptr, dW.dim, db.ptr, ys[1].ptr, ys[1].dim, 0, S()))
    for y in ys:
        assert np.all(np.abs(y.numpy() - z) <= 2e-5 * mag + 1e-6)
    z, mag = bwd_ref(E, W, 1)
    os_ = [DeviceArray(rows, n_in), DeviceArray(rows, n_in)]
    check(lib().tnet_shared_bwd(dE.ptr, dE.dim, dW.ptr, dW.dim, 1, os_[0].ptr, os_[0].dim, S()))
    check(lib().tnet_sgemm(b"N", b"T", rows, n_in, n_out, 1.0, dE.ptr, dE.stride, dW.ptr, dW.stride, 0.0, os_[1].ptr,
                           os_[1].stride, S()))
    for o in os_:
        assert np.all(np.abs(o.numpy() - z) <= 2e-5 * mag + 1e-6)
    scale, l2 = -0.3 / rows, -1e-4
    g, mag, gb, magb = upd_ref(X, E, 1, n_in, n_out)
    w = W + scale * g
    w = w + l2 * w
    tol = 2e-5 * abs(scale) * mag + 2e-7 * np.abs(W) + 1e-7
    dW2, db2 = DeviceArray.from_numpy(W), DeviceArray.vector(b)
    check(lib().tnet_shared_update(dX.ptr, dX.dim, dE.ptr, dE.dim, 1, dW.ptr, dW.dim, None, 0, db.ptr, None, scale,
                                   0.0, l2, S()))
    check(lib().tnet_affine_update(dX.ptr, dX.dim, dE.ptr, dE.dim, dW2.ptr, dW2.dim, None, 0, scale, 0.0, l2, S()))
    for d in (dW, dW2):
        assert np.all(np.abs(d.numpy() - w) <= tol)
    np.testing.assert_allclose(db.numpy().reshape(-1), b + scale * gb, rtol=1e-5, atol=1e-7)


# --------------------------------------------------------------------------------- component level
def shared_net(seed=50):
    """3 x (20 -> 12) shared, sigmoid, 36 -> 9 affine, softmax"""
    return formats.gen_shared_init(3, 20, 12, seed=seed, negbias=False) + formats.gen_mlp_init([36, 9], seed=seed + 1)


class SharedOracle:
    """float64 restatement of the GPU semantics: CuSharedLinearity::Update (cuSharedLinearity.cc:65-94) and
    CuBiasedLinearity::Update (cuBiasedLinearity.cc:46-64) under CuNetwork::Backpropagate"""

    def __init__(self, layers):
        self.L = [formats.Layer(l.tag, l.n_out, l.n_in, None if l.W is None else l.W.astype(np.float64),
                                None if l.b is None else l.b.astype(np.float64), dict(l.extra)) for l in layers]
        self.corr = {k: (np.zeros_like(l.W), np.zeros_like(l.b)) for k, l in enumerate(self.L) if l.W is not None}
        self.xent = 0.0

    def forward(self, X):
        acts = [np.asarray(X, np.float64)]
        for l in self.L:
            a = acts[-1]
            if l.tag == "<biasedlinearity>":
                a = a @ l.W + l.b
            elif l.tag == "<sharedlinearity>":
                a = np.concatenate([x @ l.W + l.b for x in windows(a, l.extra["n_inst"], l.W.shape[0])], axis=1)
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
        for k in range(len(self.L) - 1, -1, -1):
            l, a_in = self.L[k], acts[k]
            if l.tag == "<sigmoid>":
                err = err * acts[k + 1] * (1.0 - acts[k + 1])
            elif l.W is not None:
                shared = l.tag == "<sharedlinearity>"
                n = l.extra["n_inst"] if shared else 1
                ni, no = l.W.shape
                e_in = err
                err = np.concatenate([e @ l.W.T for e in windows(e_in, n, no)], axis=1)  # pre-update weights
                g, _, gb, _ = upd_ref(a_in, e_in, n, ni, no)
                N = (rows if gdf else 1.0) / (1.0 - mmt) * n
                l2 = -lr * wc * (1.0 if (shared or gdf) else rows)   # no rows factor in the shared layer
                cw, cb = self.corr[k]
                cw, cb = g + mmt * cw, gb + mmt * cb
                self.corr[k] = (cw, cb)
                l.W = l.W + (-lr / N) * cw
                l.W = l.W + l2 * l.W
                l.b = l.b + (-lr / N) * cb
        return Y


@pytest.mark.parametrize("mmt,wc,gdf", [(0.0, 0.0, False), (0.9, 1e-3, True), (0.0, 1e-3, False), (0.9, 0.0, True)])
def test_component_train_bunch_vs_restatement(mmt, wc, gdf):
    layers = shared_net()
    buf = io.StringIO()
    formats.write_nnet(layers, buf, precision=9)
    net = Network(text=buf.getvalue())
    assert net.components()[0] == ("<sharedlinearity>", 60, 36)
    lr = 0.05
    net.set_learn_rate(lr)
    net.set_momentum(mmt)
    net.set_weightcost(wc)
    net.set_grad_div_frm(gdf)
    net.keep_output(True)
    obj = Objective()
    ref = SharedOracle(formats.read_nnet(buf.getvalue()))
    rng = np.random.default_rng(51)
    B = 32
    for s in range(3):
        X = rng.standard_normal((B, 60)).astype(np.float32)
        lab = rng.integers(0, 9, B).astype(np.int32)
        net.train_bunch(obj, DeviceArray.from_numpy(X), DeviceArray.vector(lab))
        Yr = ref.step(X, lab, lr, mmt, wc, gdf)
        np.testing.assert_allclose(net.output(3, B), Yr, rtol=2e-4, atol=2e-6)
        W, b, n = net.shared_params(0)
        assert n == 3
        np.testing.assert_allclose(W, ref.L[0].W, rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(b, ref.L[0].b, rtol=2e-4, atol=2e-6)
        Wt, bt = net.get_params(2)
        np.testing.assert_allclose(Wt, ref.L[2].W, rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(bt, ref.L[2].b, rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(obj.stats()[0], ref.xent, rtol=1e-5)


def test_shared_params_abi_and_write_read(tmp_path):
    """set / get through the C ABI; a written file read back holds the same parameters bit for bit (parameters
    that 6 significant digits -- the writer's precision, CuBiasedLinearity's -- represent exactly)"""
    layers = formats.round_trip_text(shared_net(52), 6)
    net = Network.from_layers(layers, precision=6)
    W, b, n = net.shared_params(0)
    assert n == 3 and W.shape == (20, 12) and b.shape == (12,)
    np.testing.assert_array_equal(W, layers[0].W)
    np.testing.assert_array_equal(b, layers[0].b)
    p = str(tmp_path / "shared.nnet")
    net.write(p)
    back = Network(path=p)
    W2, b2, n2 = back.shared_params(0)
    assert n2 == 3
    np.testing.assert_array_equal(W2, W)
    np.testing.assert_array_equal(b2, b)
    np.testing.assert_array_equal(back.get_params(2)[0], net.get_params(2)[0])
    again = formats.read_nnet(p)
    assert again[0].extra["n_inst"] == 3
    np.testing.assert_array_equal(again[0].W, W)
    Wn = (W * 2).astype(np.float32)
    net.set_shared_params(0, Wn, None)
    np.testing.assert_array_equal(net.shared_params(0)[0], Wn)
    np.testing.assert_array_equal(net.shared_params(0)[1], b)
    with pytest.raises(TnetError):
        net.shared_params(2)       # a <biasedlinearity>
    with pytest.raises(TnetError):
        net.get_params(0)          # get_params stays <biasedlinearity>-only


@pytest.mark.parametrize("text,msg", [
    ("<sharedlinearity> 48 72\n0\nm 16 24\n", "Bad number of instances"),
    ("<sharedlinearity> 48 72\n5\nm 16 24\n", "divisible"),
    ("<sharedlinearity> 4 6\n2\nm 2 2\n1 2\n3 4\nv 2 0 0\n", "Wrong dimensionalities"),
])
def test_library_rejects_malformed_shared_headers(text, msg):
    with pytest.raises(TnetError, match=msg):
        Network(text=text)


# ----------------------------------------------------------------------------------- reference pins
def _golden(golden_dir, name):
    return load_npz(os.path.join(golden_dir, name))


def _pin_params(net, g, s):
    k = 0
    for i, (tag, _, _) in enumerate(net.components()):
        if tag == "<sharedlinearity>":
            W, b, _ = net.shared_params(i)
        elif tag == "<biasedlinearity>":
            W, b = net.get_params(i)
        else:
            continue
        np.testing.assert_allclose(W, g[f"step{s}_W{k}"], rtol=2e-4, atol=1e-6)
        np.testing.assert_allclose(b, g[f"step{s}_b{k}"], rtol=2e-4, atol=1e-6)
        k += 1
    assert k > 0


@pytest.mark.parametrize("name", ["shared_steps_first.npz", "shared_steps_stack.npz"])
def test_train_bunch_matches_reference_cpu_tnet(golden_dir, name):
    """GRADDIVFRM off, momentum 0, wc 0 == the CPU twin's single-thread step (SharedLinearity.cc:232-274)"""
    g = _golden(golden_dir, name)
    B = int(g["bunch"])
    net = Network(text=str(g["nnet"]))
    net.set_learn_rate(float(g["lr"]))
    net.set_weightcost(float(g["wc"]))
    net.set_grad_div_frm(False)
    net.keep_output(True)
    obj = Objective()
    X, lab = g["X"], g["labels"]
    nsteps = X.shape[0] // B
    assert nsteps == (4 if "first" in name else 1)
    for s in range(nsteps):
        net.train_bunch(obj, DeviceArray.from_numpy(X[s * B:(s + 1) * B]), DeviceArray.vector(lab[s * B:(s + 1) * B]))
        Y = net.output(len(net.components()) - 1, B)
        np.testing.assert_allclose(Y, g[f"Y_{s}"], rtol=2e-4, atol=2e-6)
        _pin_params(net, g, s)
    err, frames, _ = obj.stats()
    assert frames == int(g["frames"])
    np.testing.assert_allclose(err, float(g["xent_sum"]), rtol=1e-5)


def test_trainer_reproduces_the_pinned_steps(golden_dir):
    """Trainer (cache + generic step, randomize off) over the shared_steps_first net: the same 4-step parameters"""
    g = _golden(golden_dir, "shared_steps_first.npz")
    B = int(g["bunch"])
    net = Network(text=str(g["nnet"]))
    net.set_learn_rate(float(g["lr"]))
    net.set_grad_div_frm(False)
    obj = Objective()
    tr = Trainer(net, obj, bunchsize=B, cachesize=4 * B, seed=1, randomize=False)
    tr.add_utterance(g["X"], g["labels"])
    tr.finish()
    assert tr.steps == 4
    _pin_params(net, g, 3)
    np.testing.assert_allclose(obj.stats()[0], float(g["xent_sum"]), rtol=1e-5)
    # replay serves a non-fusable network too: it is the same generic step over the rewound cache
    W3 = net.shared_params(0)[0]
    tr.replay(2)
    assert tr.steps == 6
    W5 = net.shared_params(0)[0]
    assert np.isfinite(W5).all() and not np.array_equal(W5, W3)


def test_blockarray_forward_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "blockarray_fwd.npz"))
    net = Network(text=str(g["nnet"]))
    assert net.components() == [("<blockarray>", 28, 17)]
    Y = net.propagate(DeviceArray.from_numpy(g["X"])).numpy()
    np.testing.assert_allclose(Y, g["Y"], rtol=2e-4, atol=2e-6)


def test_blockarray_write_read_and_no_backward(golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "blockarray_fwd.npz"))
    net = Network(text=str(g["nnet"]))
    p = str(tmp_path / "ba.nnet")
    net.write(p)
    back = formats.read_nnet(p)
    orig = formats.read_nnet(str(g["nnet"]))
    assert [[l.tag for l in blk] for blk in back[0].extra["blocks"]] == \
           [[l.tag for l in blk] for blk in orig[0].extra["blocks"]]
    np.testing.assert_allclose(back[0].extra["blocks"][1][0].W, orig[0].extra["blocks"][1][0].W, rtol=1e-5, atol=1e-7)
    again = Network(path=p)
    X = DeviceArray.from_numpy(g["X"])
    np.testing.assert_allclose(again.propagate(X).numpy(), g["Y"], rtol=1e-4, atol=1e-5)
    # the backward pass raises the library's error (cuBlockArray.cc:41-54): no crash, no silent pass --
    # BackpropagateFnc with the learn rate at its default 0, Update once a learn rate makes it the stopper
    net.propagate(X)
    with pytest.raises(TnetError, match="Unimplemented"):
        net.backpropagate(DeviceArray(33, 17))
    net.set_learn_rate(0.1)
    net.propagate(X)
    with pytest.raises(TnetError, match="Unimplemented"):
        net.backpropagate(DeviceArray(33, 17))
