"""CPU-only checks of <sharedlinearity> / <blockarray>: the .nnet text format in tnet_amd.formats (round trips, the
block-array text the reference CPU TNet read for tests/golden/blockarray_fwd.npz, the three malformed shared
headers of cuSharedLinearity.cc:99-157) and the argument refusals of tnet_shared_fwd / _bwd / _update, which
come before any launch (fake addresses, never dereferenced)."""
import ctypes
import io
import os

import numpy as np
import pytest

from tnet_amd import _lib, formats
from tnet_amd._lib import MatrixDim

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _text(layers, precision=9):
    buf = io.StringIO()
    formats.write_nnet(layers, buf, precision)
    return buf.getvalue()


def _block_array():
    b1 = formats.gen_mlp_init([10, 7], seed=1)
    b1[-1] = formats.Layer("<sigmoid>", 7, 7)
    b2 = formats.gen_shared_init(2, 9, 5, seed=2)
    return [formats.Layer("<blockarray>", 17, 28, extra={"blocks": [b1, b2]})]


def test_shared_round_trip():
    layers = formats.gen_shared_init(3, 24, 16, seed=4) + formats.gen_mlp_init([48, 10], seed=5)
    assert (layers[0].tag, layers[0].n_out, layers[0].n_in) == ("<sharedlinearity>", 48, 72)
    assert layers[0].W.shape == (24, 16) and layers[0].b.shape == (16,) and layers[0].extra["n_inst"] == 3
    text = _text(layers)
    # the reference's layout (cuSharedLinearity.cc:160-176): instance count, transposed matrix, bias
    assert text.startswith("<sharedlinearity> 48 72\n3\nm 16 24\n")
    back = formats.read_nnet(text)
    assert [l.tag for l in back] == ["<sharedlinearity>", "<sigmoid>", "<biasedlinearity>", "<softmax>"]
    assert back[0].extra["n_inst"] == 3
    np.testing.assert_array_equal(back[0].W, layers[0].W)
    np.testing.assert_array_equal(back[0].b, layers[0].b)
    np.testing.assert_array_equal(back[2].W, layers[2].W)
    assert _text(back) == text
    six = formats.round_trip_text(layers, 6)
    np.testing.assert_allclose(six[0].W, layers[0].W, rtol=1e-5, atol=1e-7)
    assert _text(formats.round_trip_text(six, 6), 6) == _text(six, 6)


def test_gen_shared_init_draws_like_gen_mlp_init():
    """the same distribution: a hidden layer of gen_mlp_init with the same seed and shape has the same parameters"""
    shared = formats.gen_shared_init(5, 20, 12, seed=7)[0]
    mlp = formats.gen_mlp_init([20, 12, 3], seed=7)[0]
    np.testing.assert_array_equal(shared.W, mlp.W)
    np.testing.assert_array_equal(shared.b, mlp.b)
    assert (shared.n_in, shared.n_out) == (100, 60)


def test_blockarray_round_trip():
    layers = _block_array()
    text = _text(layers)
    # cuBlockArray.cc:125-135: " nBlocks " then per block "<block> k", the nested network, "<endblock>"
    assert text.startswith("<blockarray> 17 28\n 2 <block> 1\n<biasedlinearity> 7 10\n")
    assert text.count("<endblock>\n") == 2 and "<block> 2\n<sharedlinearity> 10 18\n2\n" in text
    back = formats.read_nnet(text)
    assert len(back) == 1 and back[0].tag == "<blockarray>"
    blocks = back[0].extra["blocks"]
    assert [[l.tag for l in b] for b in blocks] == [["<biasedlinearity>", "<sigmoid>"], ["<sharedlinearity>", "<sigmoid>"]]
    np.testing.assert_array_equal(blocks[0][0].W, layers[0].extra["blocks"][0][0].W)
    np.testing.assert_array_equal(blocks[1][0].W, layers[0].extra["blocks"][1][0].W)
    assert blocks[1][0].extra["n_inst"] == 2
    assert _text(back) == text
    # a layer after the array is read after the last <endblock>
    more = formats.read_nnet(text + _text(formats.gen_mlp_init([17, 4], seed=3)))
    assert [l.tag for l in more] == ["<blockarray>", "<biasedlinearity>", "<softmax>"]


def test_reads_the_block_array_text_the_reference_read():
    g = np.load(os.path.join(GOLDEN, "blockarray_fwd.npz"))
    layers = formats.read_nnet(str(g["nnet"]))
    assert (layers[0].tag, layers[0].n_out, layers[0].n_in) == ("<blockarray>", 17, 28)
    b1, b2 = layers[0].extra["blocks"]
    assert (b1[0].tag, b1[0].W.shape) == ("<biasedlinearity>", (10, 7))
    assert (b2[0].tag, b2[0].W.shape, b2[0].extra["n_inst"]) == ("<sharedlinearity>", (9, 5), 2)
    # its float64 forward is the reference's output
    X = g["X"].astype(np.float64)
    y1 = 1 / (1 + np.exp(-(X[:, :10] @ b1[0].W + b1[0].b)))
    y2 = [1 / (1 + np.exp(-(X[:, 10 + 9 * i:19 + 9 * i] @ b2[0].W + b2[0].b))) for i in range(2)]
    np.testing.assert_allclose(np.concatenate([y1] + y2, axis=1), g["Y"], rtol=2e-4, atol=2e-6)


@pytest.mark.parametrize("text,msg", [
    ("<sharedlinearity> 48 72\n0\nm 16 24\n", "Bad number of instances"),
    ("<sharedlinearity> 48 72\n5\nm 16 24\n", "divisible by number of instances"),
    ("<sharedlinearity> 4 6\n2\nm 2 2\n1 2\n3 4\nv 2 0 0\n", "Wrong dimensionalities"),
])
def test_rejects_malformed_shared_headers(text, msg):
    with pytest.raises(ValueError, match=msg):
        formats.read_nnet(text)


def test_existing_tags_write_the_same_bytes():
    """the two new tags changed nothing for the old ones: a fixed MLP's text, byte for byte"""
    layers = [formats.Layer("<biasedlinearity>", 2, 3, np.array([[1, 2], [3, 4], [5, 6]], np.float32),
                            np.array([0.5, -1.25], np.float32)), formats.Layer("<softmax>", 2, 2)]
    assert _text(layers, 6) == ("<biasedlinearity> 2 3\nm 2 3\n1 3 5 \n2 4 6 \nv 2  0.5 -1.25 \n\n<softmax> 2 2\n")


# ---------------------------------------------------------------- argument refusals of the kernel entry points
def _fake(k, off=0):
    """a 16-B aligned device-address stand-in (never dereferenced: the refusals come before any launch)"""
    return ctypes.c_void_p((1 << 44) + k * (1 << 28) + off)


ROWS, N, NIN, NOUT = 64, 3, 24, 16
X, E, W, C, b, cb, Y, EO = (_fake(k) for k in range(8))
dX, dE = MatrixDim(ROWS, N * NIN, 128), MatrixDim(ROWS, N * NOUT, 64)
dW, dY, dEo = MatrixDim(NIN, NOUT, 64), MatrixDim(ROWS, N * NOUT, 64), MatrixDim(ROWS, N * NIN, 128)


def test_symbols_exist():
    L = _lib.lib()
    for name in ("tnet_shared_fwd", "tnet_shared_bwd", "tnet_shared_update", "tnet_net_shared_get",
                 "tnet_net_shared_set"):
        assert hasattr(L, name)


def test_shared_fwd_refusals():
    L = _lib.lib()

    def fwd(x=X, dx=dX, w=W, dw=dW, bias=b, n=N, y=Y, dy=dY):
        return L.tnet_shared_fwd(x, dx, w, dw, bias, n, y, dy, None)
    assert fwd(n=0) == -1 and fwd(n=-2) == -1
    assert fwd(n=2) == -1                                             # dX.cols != n_inst * dW.rows
    assert fwd(dx=MatrixDim(ROWS, N * NIN + 1, 128)) == -1
    assert fwd(dy=MatrixDim(ROWS, N * NOUT - 1, 64)) == -1            # dY.cols != n_inst * dW.cols
    assert fwd(dy=MatrixDim(ROWS + 1, N * NOUT, 64)) == -1
    assert fwd(dx=MatrixDim(ROWS, N * NIN, 74)) == -1                 # strides: multiples of 4
    assert fwd(dw=MatrixDim(NIN, NOUT, 18)) == -1
    assert fwd(dy=MatrixDim(ROWS, N * NOUT, 50)) == -1
    assert fwd(bias=None) == -1
    assert fwd(w=X) == -1 and fwd(w=Y) == -1                          # W overlaps X / Y
    assert fwd(w=_fake(0, 64)) == -1                                  # ... partly


def test_shared_bwd_refusals():
    L = _lib.lib()

    def bwd(e=E, de=dE, w=W, dw=dW, n=N, eo=EO, deo=dEo):
        return L.tnet_shared_bwd(e, de, w, dw, n, eo, deo, None)
    assert bwd(n=0) == -1
    assert bwd(n=4) == -1                                             # dE.cols != n_inst * dW.cols
    assert bwd(deo=MatrixDim(ROWS, N * NIN - 1, 128)) == -1
    assert bwd(deo=MatrixDim(ROWS - 1, N * NIN, 128)) == -1
    assert bwd(de=MatrixDim(ROWS, N * NOUT, 49)) == -1
    assert bwd(deo=MatrixDim(ROWS, N * NIN, 73)) == -1
    assert bwd(w=E) == -1 and bwd(w=EO) == -1


def test_shared_update_refusals():
    L = _lib.lib()

    def upd(x=X, dx=dX, e=E, de=dE, n=N, w=W, dw=dW, c=C, ldc=64, bias=b, cbias=cb, mmt=0.5):
        return L.tnet_shared_update(x, dx, e, de, n, w, dw, c, ldc, bias, cbias, -0.1, mmt, 0.0, None)
    assert upd(n=0) == -1
    assert upd(n=2) == -1
    assert upd(de=MatrixDim(ROWS, N * NOUT + 4, 64)) == -1
    assert upd(de=MatrixDim(ROWS + 1, N * NOUT, 64)) == -1            # X and E rows differ
    assert upd(dx=MatrixDim(ROWS, N * NIN, 75)) == -1
    assert upd(dw=MatrixDim(NIN, NOUT, 17)) == -1
    assert upd(ldc=18) == -1
    assert upd(bias=None) == -1
    assert upd(c=None) == -1 and upd(cbias=None) == -1                # nullable only with momentum 0
    for bad in (X, E):                                                # W / corrW overlapping X / E
        assert upd(w=bad) == -1
        assert upd(c=bad) == -1
    assert upd(c=W) == -1
