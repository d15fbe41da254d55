"""CPU-only checks of <discretelinearity> in tnet_amd.formats: the .nnet text layout of
cuDiscreteLinearity.cc:139-156 (block count, one transposed matrix per block, one bias), round trips of ragged
blocks, gen_discrete_init, and the malformed files of cuDiscreteLinearity.cc:81-136."""
import io

import numpy as np
import pytest

from tnet_amd import _lib, formats


def _text(layers, precision=9):
    buf = io.StringIO()
    formats.write_nnet(layers, buf, precision)
    return buf.getvalue()


RAGGED_IN, RAGGED_OUT = [20, 7, 9], [12, 5, 8]


@pytest.mark.parametrize("precision", [6, 9])
def test_discrete_round_trip_ragged(precision):
    layers = formats.gen_discrete_init(RAGGED_IN, RAGGED_OUT, seed=4) + formats.gen_mlp_init([25, 9], seed=5)
    assert (layers[0].tag, layers[0].n_out, layers[0].n_in) == ("<discretelinearity>", 25, 36)
    text = _text(layers, precision)
    assert text.startswith("<discretelinearity> 25 36\n3\nm 12 20\n")
    back = formats.read_nnet(text)
    assert [l.tag for l in back] == ["<discretelinearity>", "<sigmoid>", "<biasedlinearity>", "<softmax>"]
    assert back[0].W is None and len(back[0].extra["Ws"]) == 3
    for W, W0, ni, no in zip(back[0].extra["Ws"], layers[0].extra["Ws"], RAGGED_IN, RAGGED_OUT):
        assert W.shape == (ni, no) and W.dtype == np.float32
        if precision == 9:      # 9 significant digits identify a float32
            np.testing.assert_array_equal(W, W0)
        else:
            np.testing.assert_allclose(W, W0, rtol=1e-5, atol=1e-7)
    if precision == 9:
        np.testing.assert_array_equal(back[0].b, layers[0].b)
    np.testing.assert_array_equal(back[2].W, formats.round_trip_text(layers, precision)[2].W)
    # a second trip at the same precision changes nothing more
    assert _text(back, precision) == text
    again = formats.round_trip_text(back, precision)
    for W, W1 in zip(again[0].extra["Ws"], back[0].extra["Ws"]):
        np.testing.assert_array_equal(W, W1)
    np.testing.assert_array_equal(again[0].b, back[0].b)


def test_gen_discrete_init_shapes_and_seed():
    a = formats.gen_discrete_init(RAGGED_IN, RAGGED_OUT, seed=7)
    b = formats.gen_discrete_init(RAGGED_IN, RAGGED_OUT, seed=7)
    c = formats.gen_discrete_init(RAGGED_IN, RAGGED_OUT, seed=8)
    assert [l.tag for l in a] == ["<discretelinearity>", "<sigmoid>"]
    assert (a[0].n_in, a[0].n_out, a[1].n_in, a[1].n_out) == (36, 25, 25, 25)
    assert a[0].W is None and a[0].b.shape == (25,)
    assert [W.shape for W in a[0].extra["Ws"]] == [(20, 12), (7, 5), (9, 8)]
    for Wa, Wb, Wc in zip(a[0].extra["Ws"], b[0].extra["Ws"], c[0].extra["Ws"]):
        np.testing.assert_array_equal(Wa, Wb)
        assert not np.array_equal(Wa, Wc)
    np.testing.assert_array_equal(a[0].b, b[0].b)
    # the distributions of the other gen_*_init functions
    big = formats.gen_discrete_init([200, 100], [150, 250], seed=9)[0]
    w = np.concatenate([W.reshape(-1) for W in big.extra["Ws"]])
    assert abs(float(w.mean())) < 2e-3 and abs(float(w.std()) - 0.1) < 2e-3
    assert big.b.min() >= -4.1 and big.b.max() <= -3.9
    uni = formats.gen_discrete_init([200, 100], [150, 250], seed=9, gauss=False, negbias=False)[0]
    w = np.concatenate([W.reshape(-1) for W in uni.extra["Ws"]])
    assert w.min() >= -0.1 and w.max() <= 0.1 and abs(float(w.std()) - 0.2 / np.sqrt(12)) < 2e-3
    assert not uni.b.any()
    # the first block is drawn as gen_mlp_init draws a hidden layer of that shape
    np.testing.assert_array_equal(a[0].extra["Ws"][0], formats.gen_mlp_init([20, 12, 3], seed=7)[0].W)
    with pytest.raises(ValueError):
        formats.gen_discrete_init([3, 4], [5], seed=1)


def test_writer_byte_layout():
    """block k is written as W_k^T ('m out_k in_k'), then one bias; numbers as CuBiasedLinearity's writer does"""
    W0 = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], np.float32)      # 3 -> 2
    W1 = np.array([[0.5]], np.float32)                                     # 1 -> 1
    L = formats.Layer("<discretelinearity>", 3, 4, None, np.array([0.25, -1.0, 8.0], np.float32), {"Ws": [W0, W1]})
    assert _text([L], 6) == ("<discretelinearity> 3 4\n"
                             "2\n"
                             "m 2 3\n"
                             "1 3 5 \n"
                             "2 4 6 \n"
                             "m 1 1\n"
                             "0.5 \n"
                             "v 3  0.25 -1 8 \n"
                             "\n")
    back = formats.read_nnet(_text([L], 6))[0]
    np.testing.assert_array_equal(back.extra["Ws"][0], W0)
    np.testing.assert_array_equal(back.extra["Ws"][1], W1)
    np.testing.assert_array_equal(back.b, L.b)


@pytest.mark.parametrize("text,msg", [
    ("<discretelinearity> 3 4\n0\nm 2 3\n1 3 5\n2 4 6\n", "Bad number of blocks"),
    ("<discretelinearity> 3 4\n2\nm 2 3\n1 3 5\n2 4 6\nm 0 0\nv 3 0 0 0\n", "Missing linearity matrix"),
    ("<discretelinearity> 3 4\n2\nm 2 3\n1 3 5\n2 4 6\nm 1 1\n0.5\nv 0\n", "Missing bias vector"),
    ("<discretelinearity> 3 5\n2\nm 2 3\n1 3 5\n2 4 6\nm 1 1\n0.5\nv 3 0 0 0\n", "Wrong dimensionalities"),
    ("<discretelinearity> 4 4\n2\nm 2 3\n1 3 5\n2 4 6\nm 1 1\n0.5\nv 4 0 0 0 0\n", "Wrong dimensionalities"),
    ("<discretelinearity> 3 4\n2\nm 2 3\n1 3 5\n2 4 6\nm 1 1\n0.5\nv 2 0 0\n", "Wrong dimensionalities"),
])
def test_rejects_malformed_discrete_files(text, msg):
    with pytest.raises(ValueError, match=msg):
        formats.read_nnet(text)


def test_library_exports_the_discrete_entry_points():
    declared, L = set(_lib.header_symbols()), _lib.lib()
    for name in ("tnet_discrete_plan_create", "tnet_discrete_plan_free", "tnet_discrete_plan_floats",
                 "tnet_discrete_plan_blocks", "tnet_discrete_plan_block", "tnet_discrete_fwd", "tnet_discrete_bwd",
                 "tnet_discrete_update", "tnet_net_discrete_blocks", "tnet_net_discrete_get",
                 "tnet_net_discrete_set"):
        assert name in declared and hasattr(L, name)


def test_plan_create_refuses_bad_block_lists():
    """refused before anything touches the device"""
    import ctypes
    L, ERR_ARG = _lib.lib(), -1
    ni, no = np.array([3, 0], np.int32), np.array([2, 2], np.int32)
    p = ctypes.c_void_p()
    assert L.tnet_discrete_plan_create(ni.ctypes.data, no.ctypes.data, 0, ctypes.byref(p)) == ERR_ARG
    assert L.tnet_discrete_plan_create(ni.ctypes.data, no.ctypes.data, 2, ctypes.byref(p)) == ERR_ARG  # in_1 = 0
    assert L.tnet_discrete_plan_create(None, no.ctypes.data, 2, ctypes.byref(p)) == ERR_ARG
    assert L.tnet_discrete_plan_create(ni.ctypes.data, no.ctypes.data, 1, None) == ERR_ARG
    assert p.value is None
    assert L.tnet_discrete_plan_free(None) == 0
