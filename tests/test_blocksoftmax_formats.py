"""<blocksoftmax> without a GPU: the .nnet text of the tag, the generator, and the float64 restatement
(tests/blocksoftmax_cases.py) the GPU tests compare against -- it reproduces both reference fixtures within their pin
tolerances, and its one-step parameter change is the finite-difference gradient of the summed cross-entropy."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import blocksoftmax_cases as cases  # noqa: E402
from tnet_amd import formats  # noqa: E402

# the procedure and tolerance of tests/test_stack_cases_cpu.py: central differences with h = 1e-6, rtol 1e-5 over a
# rounding floor.  The floor there, 1e-8, is sqrt(32 rows) * 4e-15 (a row's loss of about 2 out of five products of
# some hundred terms) / (2 h); this net has 16 rows and two products of at most 16 terms, so its quotient's rounding
# is smaller and the same floor holds.
FD_H, FD_RTOL, FD_FLOOR = 1e-6, 1e-5, 1e-8


def _text(layers, precision=9):
    buf = io.StringIO()
    formats.write_nnet(layers, buf, precision)
    return buf.getvalue()


def test_write_read_write_is_text_identical():
    layers = formats.gen_mlp_init([7, 9, 4], seed=1)[:2] + formats.gen_blocksoftmax_top(9, (3, 5, 2), seed=2)
    text = _text(layers)
    assert "<blocksoftmax> 10 10\nv 3  3 5 2 \n" in text
    back = formats.read_nnet(text)
    assert _text(back) == text
    assert [L.tag for L in back] == ["<biasedlinearity>", "<sigmoid>", "<biasedlinearity>", "<blocksoftmax>"]


@pytest.mark.parametrize("dims", [(1,), (1, 1, 1), (3, 5, 2), (135,) * 24, (135, 4000)])
def test_dims_survive_a_round_trip(dims):
    n = sum(dims)
    L = formats.Layer("<blocksoftmax>", n, n, extra={"dims": list(dims)})
    for back in (formats.read_nnet(_text([L])), formats.round_trip_text([L])):
        assert len(back) == 1 and back[0].tag == "<blocksoftmax>" and (back[0].n_out, back[0].n_in) == (n, n)
        assert back[0].extra["dims"] == list(dims)
        assert all(type(d) is int for d in back[0].extra["dims"])
    # tags are case-insensitive, as everywhere in the format
    assert formats.read_nnet(_text([L]).replace("<blocksoftmax>", "<BlockSoftmax>"))[0].extra["dims"] == list(dims)


@pytest.mark.parametrize("text", [
    "<blocksoftmax> 10 10\nv 3  3 5 3 \n",      # sum 11 != 10
    "<blocksoftmax> 10 10\nv 2  3 5 \n",        # sum 8 != 10
    "<blocksoftmax> 10 10\nv 3  5 0 5 \n",      # a zero dim
    "<blocksoftmax> 10 10\nv 3  12 -2 0 \n",    # a negative dim (the sum would fit)
    "<blocksoftmax> 10 10\nv 0  \n",            # no block
])
def test_bad_dims_are_rejected_on_read(text):
    with pytest.raises(ValueError):
        formats.read_nnet(text)


def test_the_sum_mismatch_carries_the_reference_message():
    with pytest.raises(ValueError, match="Non-matching dimension of sum of softmaxes, the sum:11 GetNOutputs:10"):
        formats.read_nnet("<blocksoftmax> 10 10\nv 3  3 5 3 \n")


@pytest.mark.parametrize("dims", [(3, 5, 3), (5, 0, 5), (12, -2), ()])
def test_bad_dims_are_rejected_on_write_and_by_the_generator(dims):
    with pytest.raises(ValueError):
        _text([formats.Layer("<blocksoftmax>", 10, 10, extra={"dims": list(dims)})])
    if not dims or min(dims) <= 0:
        with pytest.raises(ValueError):
            formats.gen_blocksoftmax_top(6, dims, seed=0)


def test_gen_blocksoftmax_top_shapes():
    lin, bs = formats.gen_blocksoftmax_top(16, (3, 5, 2), seed=4)
    assert lin.tag == "<biasedlinearity>" and (lin.n_out, lin.n_in) == (10, 16)
    assert lin.W.shape == (16, 10) and lin.W.dtype == np.float32 and lin.b.shape == (10,) and not lin.b.any()
    assert 0.05 < lin.W.std() < 0.2                    # 0.1 N(0,1), as gen_mlp_init's output layer
    assert bs.tag == "<blocksoftmax>" and (bs.n_out, bs.n_in) == (10, 10) and bs.extra["dims"] == [3, 5, 2]
    assert bs.W is None and bs.b is None
    again = formats.gen_blocksoftmax_top(16, (3, 5, 2), seed=4)[0]
    np.testing.assert_array_equal(again.W, lin.W)
    assert np.abs(formats.gen_blocksoftmax_top(16, (3, 5, 2), seed=5)[0].W - lin.W).max() > 0
    flat = formats.gen_blocksoftmax_top(16, (3, 5, 2), seed=4, gauss=False)[0].W
    assert np.abs(flat).max() <= 0.1


# ------------------------------------------------------------------------------- restatement
def test_restatement_pieces():
    rng = np.random.default_rng(0)
    Z = rng.standard_normal((9, 10)) * 3
    dims = (3, 5, 2)
    Y = cases.block_softmax(Z, dims)
    off = cases.offsets(dims)
    assert list(off) == [0, 3, 8, 10]
    for lo, hi in zip(off[:-1], off[1:]):
        np.testing.assert_allclose(Y[:, lo:hi].sum(axis=1), 1.0, rtol=1e-14)
    # one block is the plain softmax
    e = np.exp(Z - Z.max(axis=1, keepdims=True))
    np.testing.assert_allclose(cases.block_softmax(Z, (10,)), e / e.sum(axis=1, keepdims=True), rtol=1e-15)
    lab = np.array([0, 4, 9, -1, 12, 3, 7, 8, 2])
    E, masked, xent, correct = cases.objective(Y, lab, dims)
    for r, t in enumerate(cases.clean_labels(lab, 10)):
        for j, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
            if lo <= t < hi:
                np.testing.assert_array_equal(masked[r, lo:hi], E[r, lo:hi])
            else:
                assert not masked[r, lo:hi].any()
    assert not masked[3].any() and not masked[4].any()        # -1 and an id >= N: unlabeled rows
    has = cases.clean_labels(lab, 10) >= 0
    np.testing.assert_allclose(xent, -np.log(Y[np.arange(9)[has], lab[has]]).sum(), rtol=1e-15)
    # the sum rule on sums that are neither 0 nor 1
    bad = np.zeros((1, 10))
    bad[0, 0], bad[0, 3], bad[0, 8] = 0.5, -3.0, 1.0
    out, invalid = cases.sum_rule(bad, dims)
    assert invalid == 2 and not out.any()


@pytest.mark.parametrize("name", cases.FIXTURES)
def test_restatement_reproduces_the_reference_fixture(name):
    g = cases.load_fixture(name)
    layers = formats.read_nnet(str(g["nnet"]))
    dims = [int(d) for d in g["dims"]]
    assert layers[-1].tag == "<blocksoftmax>" and layers[-1].extra["dims"] == dims
    assert tuple(dims) == (cases.MLP_DIMS if name == cases.FIXTURES[0] else cases.SHARED_DIMS)
    lab, off = g["labels"], cases.offsets(dims)
    assert (lab[6::7] == -1).all() and all(((lab >= lo) & (lab < hi)).any() for lo, hi in zip(off[:-1], off[1:]))
    xent, correct, steps = 0.0, 0, 0
    for s, X, lab_s, Y, E, x, c, net in cases.replay_fixture(g, layers):
        assert cases.margin_ok(Y).all()
        np.testing.assert_allclose(g[f"Y_{s}"], Y, rtol=cases.RTOL, atol=cases.ATOL_Y)
        np.testing.assert_allclose(g[f"E_{s}"], E, rtol=cases.RTOL, atol=cases.ATOL_Y)
        for key, ref in net.params(f"step{s}_").items():
            np.testing.assert_allclose(g[key], ref, rtol=cases.RTOL, atol=cases.ATOL_P, err_msg=key)
        xent, correct, steps = xent + x, correct + c, steps + 1
    assert steps == 4 and int(g["frames"]) == len(g["X"]) == 64
    np.testing.assert_allclose(float(g["xent_sum"]), xent, rtol=cases.XENT_RTOL)
    assert int(g["correct"]) == correct


def test_one_step_change_is_the_finite_difference_gradient():
    """On the 12 -> 16 -> 10 net of the MLP fixture (blocks 3, 5, 2; labels in every block and unlabeled rows):
    (parameter after one step - before) / -lr is the central-difference gradient of the summed cross-entropy, for
    every parameter -- so the masked error is the gradient of what the objective reports."""
    g = cases.load_fixture(cases.FIXTURES[0])
    layers = formats.read_nnet(str(g["nnet"]))
    X, lab = g["X"][:16].astype(np.float64), g["labels"][:16]
    assert (lab < 0).any() and len({int(np.searchsorted(cases.offsets(cases.MLP_DIMS), t, "right")) for t in lab
                                   if t >= 0}) == 3
    lr = 0.1
    ref = cases.Net(layers)
    before = {k: v.copy() for k, v in ref.params().items()}
    ref.step(X, lab, lr)
    after = ref.params()
    probe = cases.Net(layers)
    worst = 0.0
    for key, arr in probe.params().items():
        fd = np.zeros_like(arr)
        for idx in np.ndindex(arr.shape):
            old = arr[idx]
            arr[idx] = old + FD_H
            hi, up = arr[idx], probe.xent(X, lab)
            arr[idx] = old - FD_H
            fd[idx] = (up - probe.xent(X, lab)) / (hi - arr[idx])
            arr[idx] = old
        grad = (after[key] - before[key]) / -lr
        assert np.abs(grad).max() > 1e-4, key
        ratio = float((np.abs(fd - grad) / (FD_RTOL * np.abs(grad) + FD_FLOOR)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{key}: |fd - g| / (rtol |g| + floor) = {ratio:.3g}"
    print(f"finite differences: worst |fd - g| / (1e-5 |g| + 1e-8) = {worst:.3g}")
