"""CPU-only checks of <sparselinearity> in tnet_amd.formats: the .nnet text layout of cuSparseLinearity.cc:163-186
(W^T, bias, then the optional mask^T and accu^T), round trips with and without them, the `m` / `<` look-ahead in front
of the next component, gen_sparse_init, and the malformed files of cuSparseLinearity.cc:100-160."""
import io

import numpy as np
import pytest

from tnet_amd import formats


def _text(layers, precision=9):
    buf = io.StringIO()
    formats.write_nnet(layers, buf, precision)
    return buf.getvalue()


def _net(with_mask, with_accu, seed=3):
    """<sparselinearity> 25 -> 9, <sigmoid>, <biasedlinearity> 9 -> 4, <softmax>"""
    layers = formats.gen_sparse_init(25, 9, seed=seed, density=0.5 if with_mask else 1.0)
    if with_accu:
        layers[0].extra["accu"] = (np.random.default_rng(seed + 1).standard_normal((25, 9)) * 3).astype(np.float32)
    return layers + formats.gen_mlp_init([9, 4], seed=seed + 2)


@pytest.mark.parametrize("precision", [6, 9])
@pytest.mark.parametrize("with_mask,with_accu", [(False, False), (True, False), (True, True)],
                         ids=["plain", "mask", "mask+accu"])
def test_sparse_round_trip(precision, with_mask, with_accu):
    layers = _net(with_mask, with_accu)
    assert (layers[0].tag, layers[0].n_out, layers[0].n_in) == ("<sparselinearity>", 9, 25)
    text = _text(layers, precision)
    assert text.startswith("<sparselinearity> 9 25\nm 9 25\n")
    # the matrices of the first component: W^T, then mask^T and accu^T when present
    head = text[:text.index("<sigmoid>")]
    assert head.count("m 9 25\n") == 1 + with_mask + with_accu and head.count("v 9 ") == 1
    back = formats.read_nnet(text)
    # the look-ahead for the optional matrices must not eat the next tag
    assert [l.tag for l in back] == ["<sparselinearity>", "<sigmoid>", "<biasedlinearity>", "<softmax>"]
    L, L0 = back[0], layers[0]
    assert L.W.shape == (25, 9) and L.W.dtype == np.float32 and L.b.shape == (9,)
    if precision == 9:      # 9 significant digits identify a float32
        np.testing.assert_array_equal(L.W, L0.W)
        np.testing.assert_array_equal(L.b, L0.b)
    else:
        np.testing.assert_allclose(L.W, L0.W, rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(L.b, L0.b, rtol=1e-5)
    assert ("mask" in L.extra) == with_mask and ("accu" in L.extra) == with_accu
    if with_mask:
        np.testing.assert_array_equal(L.extra["mask"], L0.extra["mask"])    # 0 / 1 at any precision
        assert set(np.unique(L.extra["mask"])) == {0.0, 1.0}
        assert np.all(L.W[L.extra["mask"] == 0] == 0.0)
    if with_accu:
        np.testing.assert_allclose(L.extra["accu"], L0.extra["accu"], rtol=1e-5 if precision == 6 else 0)
    # the component behind it is read exactly as without the sparse layer in front
    np.testing.assert_array_equal(back[2].W, formats.round_trip_text(layers[2:], precision)[0].W)
    np.testing.assert_array_equal(back[2].b, formats.round_trip_text(layers[2:], precision)[0].b)
    # a second trip at the same precision changes nothing more
    assert _text(back, precision) == text


def test_sparse_accu_is_dropped_without_trace():
    """the trailing accu matrix changes nothing of what a reader takes from the file but extra['accu']"""
    a, b = formats.read_nnet(_text(_net(True, False))), formats.read_nnet(_text(_net(True, True)))
    for x, y in zip(a, b):
        assert (x.tag, x.n_in, x.n_out) == (y.tag, y.n_in, y.n_out)
        for p, q in ((x.W, y.W), (x.b, y.b), (x.extra.get("mask"), y.extra.get("mask"))):
            assert (p is None) == (q is None)
            if p is not None:
                np.testing.assert_array_equal(p, q)


def test_sparse_last_component_and_case():
    """the layer at the end of the file (the look-ahead meets the end, not a tag); tags are case-insensitive"""
    layers = formats.gen_sparse_init(7, 5, seed=1, density=0.4)[:1]
    for text in (_text(layers), _text(layers).replace("<sparselinearity>", "<SparseLinearity>")):
        back = formats.read_nnet(text)
        assert len(back) == 1 and back[0].tag == "<sparselinearity>"
        np.testing.assert_array_equal(back[0].extra["mask"], layers[0].extra["mask"])
    plain = formats.read_nnet(_text(formats.gen_sparse_init(7, 5, seed=1)[:1]))
    assert len(plain) == 1 and "mask" not in plain[0].extra


def test_gen_sparse_init_shapes_seed_density():
    a = formats.gen_sparse_init(40, 24, seed=7, density=0.3)
    b = formats.gen_sparse_init(40, 24, seed=7, density=0.3)
    c = formats.gen_sparse_init(40, 24, seed=8, density=0.3)
    full = formats.gen_sparse_init(40, 24, seed=7)
    assert [l.tag for l in a] == ["<sparselinearity>", "<sigmoid>"]
    assert (a[0].n_in, a[0].n_out, a[1].n_in, a[1].n_out) == (40, 24, 24, 24)
    assert a[0].W.shape == (40, 24) and a[0].b.shape == (24,) and a[0].extra["mask"].shape == (40, 24)
    np.testing.assert_array_equal(a[0].W, b[0].W)
    np.testing.assert_array_equal(a[0].extra["mask"], b[0].extra["mask"])
    assert not np.array_equal(a[0].W, c[0].W)
    # density 1: no mask; a lower density zeroes W under a 0/1 mask and leaves the other weights and the bias alone
    assert "mask" not in full[0].extra and np.all(full[0].W != 0)
    m = a[0].extra["mask"]
    assert set(np.unique(m)) == {0.0, 1.0}
    np.testing.assert_array_equal(a[0].W, full[0].W * m)
    np.testing.assert_array_equal(a[0].b, full[0].b)
    # 960 draws at p = 0.3: mean 288, standard deviation 14.2 -- six of them
    assert abs(m.sum() - 0.3 * m.size) < 6 * np.sqrt(m.size * 0.3 * 0.7)
    # the other gen_*_init functions' distributions: W ~ 0.1 N(0,1), bias U[-4.1, -3.9]
    assert 0.08 < full[0].W.std() < 0.12 and np.all((full[0].b >= -4.1) & (full[0].b <= -3.9))
    u = formats.gen_sparse_init(40, 24, seed=7, gauss=False, negbias=False)
    assert np.all(np.abs(u[0].W) <= 0.1) and np.all(u[0].b == 0)
    assert formats.gen_sparse_init(6, 4, seed=0, density=0.0)[0].extra["mask"].sum() == 0
    with pytest.raises(ValueError):
        formats.gen_sparse_init(6, 4, seed=0, density=1.5)


def _parts(with_mask=True):
    text = _text(formats.gen_sparse_init(6, 4, seed=2, density=0.5 if with_mask else 1.0)[:1])
    assert text.startswith("<sparselinearity> 4 6\nm 4 6\n")
    return text


def test_sparse_malformed_files():
    good = _parts()
    assert formats.read_nnet(good)[0].W.shape == (6, 4)
    # missing bias: the vector cut out (the mask matrix then follows the weights directly)
    v0 = good.index("v 4 ")
    v1 = good.index("\n", v0)
    with pytest.raises(ValueError, match="Missing bias"):
        formats.read_nnet(good[:v0] + good[v1:])
    # missing matrix
    with pytest.raises(ValueError, match="Missing linearity"):
        formats.read_nnet("<sparselinearity> 4 6\n" + good[v0:])
    # wrong dimensions: the header disagrees with the matrix, or the bias with the header
    with pytest.raises(ValueError, match="Wrong dimensionalities"):
        formats.read_nnet(good.replace("<sparselinearity> 4 6", "<sparselinearity> 4 7"))
    with pytest.raises(ValueError, match="Wrong dimensionalities"):
        formats.read_nnet(good.replace("<sparselinearity> 4 6", "<sparselinearity> 5 6"))
    plain = _parts(False)
    with pytest.raises(ValueError, match="Wrong dimensionalities"):
        formats.read_nnet(plain[:plain.index("v 4 ")] + "v 3  0 0 0 \n\n")
    # a mask of another shape than W
    with pytest.raises(ValueError, match="sparsity mask"):
        formats.read_nnet(plain + "m 3 6\n" + "1 0 1 1 0 1 \n" * 3)
    with pytest.raises(ValueError, match="sparsity mask"):
        formats.read_nnet(plain + "m 6 4\n" + "1 0 1 1 \n" * 6)
    # an accu matrix cannot be written without a mask in front of it (the reader would take it for the mask)
    L = formats.gen_sparse_init(6, 4, seed=2)[0]
    L.extra["accu"] = np.zeros((6, 4), np.float32)
    with pytest.raises(ValueError):
        _text([L])
