"""<blocksoftmax> on the GPU: the three kernels against float64 numpy and against each other, on views, and the
component inside the fused step, the generic step, the Trainer and the one-rank data-parallel step -- pinned to the
reference CPU TNet's output (tests/golden/blocksoftmax_steps_*.npz) and to the float64 restatement of
tests/blocksoftmax_cases.py.

One clause of the kernels' contract cannot hold for every row and is narrowed here: "B == 1 gives tnet_softmax_xent's E
bit for bit" holds on labelled rows.  On an unlabeled row the plain kernel's error is y (an all-zero target), the block
softmax's is +0.0f (its one block sums to 1: inactive, as in the reference's backward pass and in the three-call
chain); Y and the statistics agree on every row."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import blocksoftmax_cases as cases  # noqa: E402
from kernel_views import PoisonView, assert_frame_untouched, assert_unchanged  # noqa: E402
from tnet_amd import Comm, DeviceArray, Network, Objective, Trainer, TnetError, formats  # noqa: E402
from tnet_amd._lib import check, lib  # noqa: E402

ROWS = (1, 37, 300)
MIXED = tuple(int(w) for w in np.r_[np.random.default_rng(5).integers(2, 41, size=33), 1,
                                    np.random.default_rng(6).integers(2, 41, size=34)])
DIMS = {
    "one": (1,),
    "ones": (1, 1, 1),
    "3-5-2": (3, 5, 2),
    "3x135": (135, 135, 135),                  # offsets that are no multiples of 4
    "straddle": (255, 2, 255, 513),            # blocks across the 256-column unit and the 1024 boundary
    "68mixed": MIXED,                          # 68 blocks of width 1..40
    "4x1000": (1000, 1000, 1000, 1000),
    "wide": (135, 4000),                       # wider than the 4096-column register cache
    "4096": (4096,),
    "4097": (4097,),
}
assert len(MIXED) == 68 and min(MIXED) == 1 and max(MIXED) <= 40 and MIXED.count(1) == 1


def S():
    return lib().tnet_stream()


def dev_ints(v):
    return DeviceArray.vector(np.asarray(v, np.int32))


def new_stats():
    return DeviceArray(1, 1024, np.float64, stride=1024)


def stat_sums(stats):
    s = stats.numpy()[0]
    return float(s[0::2].sum()), int(round(s[1::2].sum()))


@functools.lru_cache(maxsize=None)
def case(rows, key):
    """(Z, labels with -1 and ids >= N among them, float64 Y, masked E, xent sum, correct), computed once and shared
    (the arrays are read-only).  Rows are redrawn until two conditions hold:
      * the margin condition (cases.MARGIN), so that `correct` can be compared exactly;
      * the label's posterior is either exactly 1 (a block of one column) or at most 0.99.  E = y - 1 there is formed
        from a float32 y, whose spacing just below 1 is 6e-8: rounding y alone leaves up to 3e-8 in E, and the
        tolerance 2e-5 |E| + 1e-8 is smaller than that once 1 - y < 1e-3 -- no float32 kernel can meet it there,
        the plain tnet_softmax_xent included (its test's labels, random among >= 10 columns, stay clear of it too).
        0.99 leaves ten times that room."""
    dims = DIMS[key]
    N = sum(dims)
    rng = np.random.default_rng(1000 * rows + len(dims) + N)
    Z = (rng.standard_normal((rows, N)) * 2.5).astype(np.float32)
    lab = rng.integers(0, N, size=rows).astype(np.int32)
    lab[3::7] = -1
    lab[5::11] = N
    lab[8::13] = N + 1000
    t = cases.clean_labels(lab, N)
    for _ in range(400):
        Y = cases.block_softmax(Z, dims)
        yt = np.where(t >= 0, Y[np.arange(rows), np.maximum(t, 0)], 0.0)
        bad = (yt > 0.99) & (yt < 1.0)
        if key != "ones":   # (1, 1, 1): every posterior is exactly 1.0f in any arithmetic and the first column wins
            bad |= ~cases.margin_ok(Y)
        if not bad.any():
            break
        Z[bad] = (rng.standard_normal((int(bad.sum()), N)) * 2.5).astype(np.float32)
    assert not bad.any()
    Y = cases.block_softmax(Z, dims)
    _, E, xent, correct = cases.objective(Y, lab, dims)
    for a in (Z, lab, Y, E):
        a.setflags(write=False)
    return Z, lab, Y, E, xent, correct


def run_fused(Z, dims, lab, want_y=True, want_e=True):
    rows, N = Z.shape
    dZ, dO, dL = DeviceArray.from_numpy(Z), dev_ints(cases.offsets(dims)), dev_ints(lab)
    dY = DeviceArray(rows, N) if want_y else None
    dE = DeviceArray(rows, N) if want_e else None
    stats = new_stats()
    check(lib().tnet_block_softmax_xent(dZ.ptr, dZ.dim, dO.ptr, len(dims), dL.ptr, dY.ptr if dY else None,
                                        dY.stride if dY else 0, dE.ptr if dE else None, dE.stride if dE else 0,
                                        stats.ptr, S()), "block_softmax_xent")
    return (dY.numpy() if dY else None, dE.numpy() if dE else None) + stat_sums(stats)


def run_chain(Z, dims, lab):
    """tnetF_block_softmax -> tnet_softmax_xent(Z = NULL) -> tnet_block_softmax_bwd (in place)"""
    rows, N = Z.shape
    dZ, dO, dL = DeviceArray.from_numpy(Z), dev_ints(cases.offsets(dims)), dev_ints(lab)
    dY, dE = DeviceArray(rows, N), DeviceArray(rows, N)
    stats, inv = new_stats(), dev_ints([0])
    check(lib().tnetF_block_softmax(dY.ptr, dZ.ptr, dZ.dim, dO.ptr, len(dims), S()), "block_softmax")
    check(lib().tnet_softmax_xent(None, dY.dim, dL.ptr, dY.ptr, dY.stride, dE.ptr, dE.stride, stats.ptr, S()))
    check(lib().tnet_block_softmax_bwd(dE.ptr, dE.dim, dO.ptr, len(dims), dE.ptr, dE.stride, inv.ptr, S()))
    assert int(inv.numpy()[0, 0]) == 0
    return (dY.numpy(), dE.numpy()) + stat_sums(stats)


# ------------------------------------------------------------------------- kernels vs float64
@pytest.mark.parametrize("key", list(DIMS))
@pytest.mark.parametrize("rows", ROWS)
def test_fused_call_against_float64(rows, key):
    """test_softmax_xent_labels' tolerances; labels include -1 and ids >= N"""
    Z, lab, Yref, Eref, xent, correct = case(rows, key)
    Y, E, x, c = run_fused(Z, DIMS[key], lab)
    np.testing.assert_allclose(Y, Yref, rtol=2e-5, atol=1e-9)
    np.testing.assert_allclose(E, Eref, rtol=2e-5, atol=1e-8)
    np.testing.assert_allclose(x, xent, rtol=1e-5, atol=1e-5)
    assert c == correct


@pytest.mark.parametrize("key", list(DIMS))
@pytest.mark.parametrize("rows", ROWS)
def test_forward_against_float64(rows, key):
    Z, _, Yref, _, _, _ = case(rows, key)
    dZ, dO = DeviceArray.from_numpy(Z), dev_ints(cases.offsets(DIMS[key]))
    dY = DeviceArray(*Z.shape)
    check(lib().tnetF_block_softmax(dY.ptr, dZ.ptr, dZ.dim, dO.ptr, len(DIMS[key]), S()), "block_softmax")
    np.testing.assert_allclose(dY.numpy(), Yref, rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize("dims", [(40, 60), (300, 724), (2000, 2135)], ids=["100", "1024", "4135"])
def test_per_block_range(dims):
    """one block's logits around +60, the other's around -200: a kernel that subtracts the row maximum instead of
    the block's turns the second block into 0 / 0"""
    rows, N = 9, sum(dims)
    rng = np.random.default_rng(3)
    Z = rng.standard_normal((rows, N)).astype(np.float32)
    Z[:, :dims[0]] += 60.0
    Z[:, dims[0]:] -= 200.0
    lab = rng.integers(0, N, size=rows).astype(np.int32)
    Y, E, x, _ = run_fused(Z, dims, lab)
    assert np.isfinite(Y).all() and np.isfinite(E).all() and np.isfinite(x)
    off = cases.offsets(dims)
    for lo, hi in zip(off[:-1], off[1:]):
        np.testing.assert_allclose(Y[:, lo:hi].sum(axis=1, dtype=np.float64), 1.0, atol=1e-5)
    assert (Y.max(axis=1) > 0).all()
    np.testing.assert_allclose(Y, cases.block_softmax(Z, dims), rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize("key", ["3-5-2", "3x135", "straddle", "68mixed", "4x1000", "wide"])
def test_exact_zeros_and_determinism(key):
    """E is +0.0f (the bits, not -0.0f) outside the label's block and in unlabeled rows; two runs give the same bits"""
    Z, lab, _, _, _, _ = case(37, key)
    dims, N = DIMS[key], Z.shape[1]
    Y, E, x, c = run_fused(Z, dims, lab)
    off = cases.offsets(dims)
    t = cases.clean_labels(lab, N)
    blk = np.searchsorted(off, t, side="right") - 1
    inside = (np.arange(N)[None, :] >= off[blk][:, None]) & (np.arange(N)[None, :] < off[blk + 1][:, None]) & \
        (t >= 0)[:, None]
    assert (t < 0).any() and inside.any() and not inside[t < 0].any()
    assert not E.view(np.uint32)[~inside].any()
    assert (E[inside] != 0).any()
    Y2, E2, x2, c2 = run_fused(Z, dims, lab)
    np.testing.assert_array_equal(Y.view(np.uint32), Y2.view(np.uint32))
    np.testing.assert_array_equal(E.view(np.uint32), E2.view(np.uint32))
    assert c == c2 and abs(x - x2) <= 1e-12 * abs(x)


# ----------------------------------------------------------------------- relations between calls
@pytest.mark.parametrize("rows,N", [(1, 1), (37, 10), (300, 135), (37, 405), (37, 1024), (37, 1028), (300, 4000),
                                    (37, 4096), (37, 4097), (5, 5000)])
def test_one_block_is_the_plain_softmax_xent_bit_for_bit(rows, N):
    """every path of tnet_softmax_xent: unaligned widths, one wave a row, four waves a row (1025..4096 aligned
    columns), the re-reading fallback.  Y, the statistics' slots and -- on labelled rows -- E are the same bits; an
    unlabeled row's E is +0.0f here (module docstring)."""
    rng = np.random.default_rng(N)
    Z = (rng.standard_normal((rows, N)) * 3).astype(np.float32)
    lab = rng.integers(0, N, size=rows).astype(np.int32)
    lab[2::5] = -1
    dZ, dL, dO = DeviceArray.from_numpy(Z), dev_ints(lab), dev_ints([0, N])
    out = []
    for block in (False, True):
        dY, dE, stats = DeviceArray(rows, N), DeviceArray(rows, N), new_stats()
        if block:
            check(lib().tnet_block_softmax_xent(dZ.ptr, dZ.dim, dO.ptr, 1, dL.ptr, dY.ptr, dY.stride, dE.ptr,
                                                dE.stride, stats.ptr, S()))
        else:
            check(lib().tnet_softmax_xent(dZ.ptr, dZ.dim, dL.ptr, dY.ptr, dY.stride, dE.ptr, dE.stride, stats.ptr, S()))
        out.append((dY.numpy(), dE.numpy(), stats.numpy()[0]))
    (Yp, Ep, sp), (Yb, Eb, sb) = out
    np.testing.assert_array_equal(Yb.view(np.uint32), Yp.view(np.uint32))
    np.testing.assert_array_equal(Eb.view(np.uint32)[lab >= 0], Ep.view(np.uint32)[lab >= 0])
    assert not Eb.view(np.uint32)[lab < 0].any()
    np.testing.assert_array_equal(sb, sp)     # slot by slot (at most one addition a slot at these sizes)


@pytest.mark.parametrize("key", list(DIMS))
@pytest.mark.parametrize("rows", [37, 300])
def test_fused_call_equals_the_three_call_chain(rows, key):
    """the relation test_affine_softmax_xent holds between the fused top layer and its three calls: Y and E bit for
    bit, xent to rtol 1e-12, correct exactly"""
    Z, lab, _, _, _, _ = case(rows, key)
    Yf, Ef, xf, cf = run_fused(Z, DIMS[key], lab)
    Yc, Ec, xc, cc = run_chain(Z, DIMS[key], lab)
    np.testing.assert_array_equal(Yf.view(np.uint32), Yc.view(np.uint32))
    np.testing.assert_array_equal(Ef.view(np.uint32), Ec.view(np.uint32))
    np.testing.assert_allclose(xf, xc, rtol=1e-12)
    assert cf == cc
    # Y and E are optional outputs of the fused call and do not change what the others get
    _, E2, x2, c2 = run_fused(Z, DIMS[key], lab, want_y=False)
    Y3, _, x3, c3 = run_fused(Z, DIMS[key], lab, want_e=False)
    np.testing.assert_array_equal(E2.view(np.uint32), Ef.view(np.uint32))
    np.testing.assert_array_equal(Y3.view(np.uint32), Yf.view(np.uint32))
    assert (c2, c3) == (cf, cf) and abs(x2 - xf) <= 1e-12 * abs(xf) and abs(x3 - xf) <= 1e-12 * abs(xf)


def dense_error_rows(dims):
    """rows whose block sums are, block by block, 0 / 1 / 0.5 / -3 in rotating order, and which blocks to keep"""
    rng = np.random.default_rng(9)
    off = cases.offsets(dims)
    rows = 8
    E = np.zeros((rows, off[-1]), np.float32)
    sums = (0.0, 1.0, 0.5, -3.0)
    for r in range(rows):
        for j, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
            v = rng.standard_normal(hi - lo)
            v += (sums[(r + j) % 4] - v.sum()) / (hi - lo)
            E[r, lo:hi] = v
    return E


@pytest.mark.parametrize("key", ["3-5-2", "3x135", "straddle", "68mixed", "4x1000", "wide"])
def test_sum_rule_on_dense_errors_in_place_and_out_of_place(key):
    dims = DIMS[key]
    E = dense_error_rows(dims)
    ref, invalid = cases.sum_rule(E, dims)
    assert invalid >= len(dims) * 8 // 2 - 8 and ref.any()
    dO = dev_ints(cases.offsets(dims))
    dIn, dOut, inv = DeviceArray.from_numpy(E), DeviceArray(*E.shape), dev_ints([7])
    check(lib().tnet_block_softmax_bwd(dIn.ptr, dIn.dim, dO.ptr, len(dims), dOut.ptr, dOut.stride, inv.ptr, S()))
    out = dOut.numpy()
    np.testing.assert_array_equal(out, ref.astype(np.float32))          # a copy or +0.0f, nothing computed
    assert not out.view(np.uint32)[ref == 0].any()
    assert int(inv.numpy()[0, 0]) == 7 + invalid                        # the kernel adds to the counter
    np.testing.assert_array_equal(dIn.numpy(), E)
    check(lib().tnet_block_softmax_bwd(dIn.ptr, dIn.dim, dO.ptr, len(dims), dIn.ptr, dIn.stride, None, S()))
    np.testing.assert_array_equal(dIn.numpy().view(np.uint32), out.view(np.uint32))


def test_component_counts_invalid_sums():
    """a caller's own error through the component: blocks summing to 0.5 and -3 are zeroed and counted"""
    dims = (3, 5, 2)
    net = Network(text="<blocksoftmax> 10 10\nv 3  3 5 2 \n")
    assert net.components() == [("<blocksoftmax>", 10, 10)]
    assert net.blocksoftmax_dims(0) == [3, 5, 2]
    assert net.blocksoftmax_invalid(0) == 0
    Z = np.random.default_rng(1).standard_normal((8, 10)).astype(np.float32)
    Y = net.propagate(DeviceArray.from_numpy(Z)).numpy()
    np.testing.assert_allclose(Y, cases.block_softmax(Z, dims), rtol=2e-5, atol=1e-9)
    E = dense_error_rows(dims)
    _, invalid = cases.sum_rule(E, dims)
    assert invalid == 12
    net.backpropagate(DeviceArray.from_numpy(E))
    assert net.blocksoftmax_invalid(0) == invalid
    net.backpropagate(DeviceArray.from_numpy(E))
    assert net.blocksoftmax_invalid(0, reset=True) == 2 * invalid
    assert net.blocksoftmax_invalid(0) == 0
    with pytest.raises(TnetError, match="not <blocksoftmax>"):
        Network.from_layers(formats.gen_mlp_init([4, 3], seed=0)).blocksoftmax_dims(0)


@pytest.mark.parametrize("text,msg", [
    ("<blocksoftmax> 10 10\nv 3  3 5 3 \n", "Non-matching dimension of sum of softmaxes, the sum:11 GetNOutputs:10"),
    ("<blocksoftmax> 10 10\nv 3  5 0 5 \n", "non-positive block dimension"),
    ("<blocksoftmax> 10 10\nv 3  12 -2 0 \n", "non-positive block dimension"),
    ("<blocksoftmax> 10 10\n", "expected the block dimensions"),
])
def test_library_rejects_malformed_dims(text, msg):
    with pytest.raises(TnetError, match=msg):
        Network(text=text)


# ------------------------------------------------------------------------------------ views
VIEW_DIMS = {"3-5-2": (3, 5, 2), "4x135": (135,) * 4, "wide": (135, 4000)}   # scalar, 16-byte, re-reading


@pytest.mark.parametrize("key", list(VIEW_DIMS))
@pytest.mark.parametrize("layout", ["tight", "offset", "shifted", "odd"])
def test_three_calls_on_poisoned_views(layout, key):
    """tight / offset: 16-byte aligned rows where the width allows (4 x 135 = 540 columns, offsets unaligned);
    shifted / odd: a base that is only 4-byte aligned.  Every operand is a window in a NaN-poisoned buffer: inputs
    unchanged, no word of any frame written, and the results of plain matrices -- the same bits where the view
    takes the same loads as a plain matrix (16-byte ones, or a width that allows none anywhere), the float64
    tolerances where it takes scalar loads instead (a lane then sums other columns); E is in every case exactly
    the view's own Y minus the target, masked."""
    dims = VIEW_DIMS[key]
    rows, N = 7, sum(dims)
    rng = np.random.default_rng(N + len(layout))
    Z = (rng.standard_normal((rows, N)) * 2).astype(np.float32)
    lab = rng.integers(0, N, size=rows).astype(np.int32)
    lab[2] = -1
    vlay = layout if layout in ("tight", "offset") else "shifted"        # the 1 x n operands' layouts
    vZ, vO, vL = PoisonView(Z, layout), PoisonView.vector(cases.offsets(dims), vlay), PoisonView.vector(lab, vlay)
    Yp, Ep, xp, cp = run_fused(Z, dims, lab)
    # fused
    vY, vE = PoisonView.empty(rows, N, layout), PoisonView.empty(rows, N, layout)
    vS = PoisonView(np.zeros((1, 1024)), "offset", dtype=np.float64)
    check(lib().tnet_block_softmax_xent(vZ.ptr, vZ.dim, vO.ptr, len(dims), vL.ptr, vY.ptr, vY.stride, vE.ptr,
                                        vE.stride, vS.ptr, S()))
    for v, what in ((vY, "Y"), (vE, "E"), (vS, "stats")):
        assert_frame_untouched(v, f"fused {what}")
    for v, what in ((vZ, "Z"), (vO, "offsets"), (vL, "labels")):
        assert_unchanged(v, v.initial, f"fused {what}")
    same_path = layout in ("tight", "offset") or N % 4 != 0 or N > 4096
    Yv, Ev = vY.numpy(), vE.numpy()
    if same_path:
        np.testing.assert_array_equal(Yv.view(np.uint32), Yp.view(np.uint32))
    else:
        np.testing.assert_allclose(Yv, cases.block_softmax(Z, dims), rtol=2e-5, atol=1e-9)
    off = cases.offsets(dims)
    T = np.zeros((rows, N), np.float32)
    keep = np.zeros((rows, N), bool)
    for r, t in enumerate(lab):
        if t >= 0:
            j = np.searchsorted(off, t, side="right") - 1
            T[r, t], keep[r, off[j]:off[j + 1]] = 1.0, True
    np.testing.assert_array_equal(Ev.view(np.uint32), np.where(keep, Yv - T, np.float32(0)).view(np.uint32))
    s = vS.numpy()[0]
    assert int(round(s[1::2].sum())) == cp
    np.testing.assert_allclose(s[0::2].sum(), xp, rtol=1e-12 if same_path else 1e-5)
    # forward (x and y share one stride: the same layout)
    vY2 = PoisonView.empty(rows, N, layout)
    check(lib().tnetF_block_softmax(vY2.ptr, vZ.ptr, vZ.dim, vO.ptr, len(dims), S()))
    assert_frame_untouched(vY2, "forward y")
    assert_unchanged(vZ, vZ.initial, "forward x")
    np.testing.assert_array_equal(vY2.numpy().view(np.uint32), Yv.view(np.uint32))
    # backward: out of place, then in place
    Ed = dense_error_rows(dims)[:rows]
    ref, invalid = cases.sum_rule(Ed, dims)
    vIn, vOut = PoisonView(Ed, layout), PoisonView.empty(rows, N, layout)
    vI = PoisonView.vector(np.zeros(1, np.int32), vlay)
    check(lib().tnet_block_softmax_bwd(vIn.ptr, vIn.dim, vO.ptr, len(dims), vOut.ptr, vOut.stride, vI.ptr, S()))
    assert_frame_untouched(vOut, "backward Eout")
    assert_frame_untouched(vI, "backward counter")
    assert_unchanged(vIn, vIn.initial, "backward Ein")
    np.testing.assert_array_equal(vOut.numpy(), ref.astype(np.float32))
    assert int(vI.numpy()[0, 0]) == invalid
    check(lib().tnet_block_softmax_bwd(vIn.ptr, vIn.dim, vO.ptr, len(dims), vIn.ptr, vIn.stride, None, S()))
    assert_frame_untouched(vIn, "backward in place")
    np.testing.assert_array_equal(vIn.numpy(), ref.astype(np.float32))


# ----------------------------------------------------------------------------- network level
def fixture(name):
    g = cases.load_fixture(name)
    return g, int(g["bunch"]), formats.read_nnet(str(g["nnet"]))


def fixture_net(g, keep=True):
    net = Network(text=str(g["nnet"]))
    net.set_learn_rate(float(g["lr"]))
    net.set_weightcost(float(g["wc"]))
    net.set_grad_div_frm(False)
    net.keep_output(keep)
    return net


def net_params(net):
    out, k = {}, 0
    for i, (tag, _, _) in enumerate(net.components()):
        if tag == "<sharedlinearity>":
            W, b, _ = net.shared_params(i)
        elif tag == "<biasedlinearity>":
            W, b = net.get_params(i)
        else:
            continue
        out[f"W{k}"], out[f"b{k}"] = W, b
        k += 1
    return out


def bunches(g, B):
    for s in range(len(g["X"]) // B):
        yield s, g["X"][s * B:(s + 1) * B], g["labels"][s * B:(s + 1) * B]


@pytest.mark.parametrize("name", cases.FIXTURES)
def test_train_bunch_matches_reference_cpu_tnet(name):
    """the MLP fixture takes the fused step (and must not take the <= 256-class fused top layer, a plain softmax:
    its Y would sum to 1 over the whole row), the shared one the generic step"""
    g, B, _ = fixture(name)
    net = fixture_net(g)
    assert net.components()[-1] == ("<blocksoftmax>", net.n_out, net.n_out)
    assert net.blocksoftmax_dims(len(net.components()) - 1) == [int(d) for d in g["dims"]]
    obj = Objective()
    for s, X, lab in bunches(g, B):
        net.train_bunch(obj, DeviceArray.from_numpy(X), DeviceArray.vector(lab))
        Y = net.output(len(net.components()) - 1, B)
        np.testing.assert_allclose(Y, g[f"Y_{s}"], rtol=cases.RTOL, atol=cases.ATOL_Y)
        for k, v in net_params(net).items():
            np.testing.assert_allclose(v, g[f"step{s}_{k}"], rtol=cases.RTOL, atol=cases.ATOL_P, err_msg=k)
    err, frames, correct = obj.stats()
    assert frames == int(g["frames"]) and int(round(correct)) == int(g["correct"])
    np.testing.assert_allclose(err, float(g["xent_sum"]), rtol=cases.XENT_RTOL)
    assert net.blocksoftmax_invalid(len(net.components()) - 1) == 0


def test_trainer_reproduces_the_mlp_fixture():
    g, B, _ = fixture(cases.FIXTURES[0])
    net = fixture_net(g, keep=False)
    obj = Objective()
    tr = Trainer(net, obj, bunchsize=B, cachesize=4 * B, seed=1, randomize=False)
    tr.add_utterance(g["X"], g["labels"])
    tr.finish()
    assert tr.steps == 4
    for k, v in net_params(net).items():
        np.testing.assert_allclose(v, g[f"step3_{k}"], rtol=cases.RTOL, atol=cases.ATOL_P, err_msg=k)
    err, frames, correct = obj.stats()
    np.testing.assert_allclose(err, float(g["xent_sum"]), rtol=cases.XENT_RTOL)
    assert frames == 64 and int(round(correct)) == int(g["correct"])


@pytest.mark.parametrize("name", cases.FIXTURES)
def test_write_read_train_again_and_crossval(name, tmp_path):
    g, B, _ = fixture(name)
    net = fixture_net(g)
    obj = Objective()
    todo = list(bunches(g, B))
    for s, X, lab in todo[:2]:
        net.train_bunch(obj, DeviceArray.from_numpy(X), DeviceArray.vector(lab))
    p = str(tmp_path / "two.nnet")
    net.write(p)
    assert formats.read_nnet(p)[-1].extra["dims"] == [int(d) for d in g["dims"]]
    back = Network(p)
    p2 = str(tmp_path / "again.nnet")
    back.write(p2)
    assert open(p2).read() == open(p).read()
    assert back.components() == net.components()
    last = len(net.components()) - 1
    assert back.blocksoftmax_dims(last) == net.blocksoftmax_dims(last)
    back.set_learn_rate(float(g["lr"]))
    back.set_grad_div_frm(False)
    # a cross-validation bunch changes nothing but the statistics
    before = net_params(net)
    cv = Objective()
    _, X, lab = todo[2]
    net.train_bunch(cv, DeviceArray.from_numpy(X), DeviceArray.vector(lab), train=False)
    for k, v in net_params(net).items():
        np.testing.assert_array_equal(v, before[k])
    np.testing.assert_allclose(net.output(last, B), g["Y_2"], rtol=cases.RTOL, atol=cases.ATOL_Y)
    assert cv.stats()[1] == B and cv.stats()[0] > 0
    # the written net continues as the one in memory does.  The writer keeps 6 significant digits (the reference's
    # stream precision): the read net starts within 5e-6 relative of the one in memory, 40 times inside the
    # component tolerance (rtol 2e-4 / atol 2e-6) that its parameters are held to after two more steps
    for k, v in net_params(back).items():
        np.testing.assert_allclose(v, before[k], rtol=5e-6, atol=0, err_msg=k)
    for s, X, lab in todo[2:]:
        for n in (net, back):
            n.train_bunch(Objective(), DeviceArray.from_numpy(X), DeviceArray.vector(lab))
    got, ref = net_params(back), net_params(net)
    for k in ref:
        np.testing.assert_allclose(got[k], ref[k], rtol=2e-4, atol=2e-6, err_msg=k)
        np.testing.assert_allclose(ref[k], g[f"step3_{k}"], rtol=cases.RTOL, atol=cases.ATOL_P, err_msg=k)


@pytest.mark.parametrize("name", cases.FIXTURES)
@pytest.mark.parametrize("mmt,wc,gdf", [(0.9, 1e-3, True), (0.9, 1e-3, False), (0.0, 0.0, True)])
def test_constants_against_the_restatement(name, mmt, wc, gdf):
    """momentum, weight cost and GradDivFrm: test_gpu_shared.py's component tolerance (rtol 2e-4 / atol 2e-6)"""
    g, B, layers = fixture(name)
    lr = 0.5 if gdf else 0.5 / B
    net = Network(text=str(g["nnet"]))
    net.set_learn_rate(lr)
    net.set_momentum(mmt)
    net.set_weightcost(wc)
    net.set_grad_div_frm(gdf)
    net.keep_output(True)
    ref = cases.Net(layers)
    obj = Objective()
    xent = 0.0
    for s, X, lab in bunches(g, B):
        net.train_bunch(obj, DeviceArray.from_numpy(X), DeviceArray.vector(lab))
        Y, _, x, _ = ref.step(X, lab, lr, mmt=mmt, wc=wc, gdf=gdf)
        xent += x
        np.testing.assert_allclose(net.output(len(layers) - 1, B), Y, rtol=2e-4, atol=2e-6)
        got = net_params(net)
        for k, v in ref.params().items():
            np.testing.assert_allclose(got[k], v, rtol=2e-4, atol=2e-6, err_msg=f"step {s} {k}")
    np.testing.assert_allclose(obj.stats()[0], xent, rtol=1e-5)


@pytest.mark.parametrize("name", cases.FIXTURES)
def test_frozen_top_layer_still_backpropagates_the_masked_error(name):
    g, B, layers = fixture(name)
    net = Network(text=str(g["nnet"]))
    net.set_learn_rate(0.5 / B, "1,0")
    net.set_grad_div_frm(False)
    ref = cases.Net(layers)
    before = net_params(net)
    for s, X, lab in bunches(g, B):
        net.train_bunch(Objective(), DeviceArray.from_numpy(X), DeviceArray.vector(lab))
        ref.step(X, lab, 0.5 / B, factors=[1.0, 0.0])
    got = net_params(net)
    np.testing.assert_array_equal(got["W1"], before["W1"])
    np.testing.assert_array_equal(got["b1"], before["b1"])
    assert np.abs(got["W0"] - before["W0"]).max() > 1e-4
    for k, v in ref.params().items():
        np.testing.assert_allclose(got[k], v, rtol=2e-4, atol=2e-6, err_msg=k)


@pytest.mark.parametrize("name", cases.FIXTURES)
@pytest.mark.parametrize("shard", ["0", "1"])
def test_dp_world1_equals_local_step(monkeypatch, name, shard):
    """the pattern and tolerance of test_dp_rccl_world1_equals_local_update: the MLP net against the fused step, the
    shared net against its local generic step"""
    g, B, _ = fixture(name)
    monkeypatch.setenv("TNET_DP_SHARD", shard)
    comm = Comm(0, 1, Comm.unique_id())
    runs = []
    for use_comm in (False, True):
        net = Network(text=str(g["nnet"]))
        net.set_learn_rate(0.5 / B)
        net.set_momentum(0.5)
        net.set_grad_div_frm(False)
        if use_comm:
            net.set_comm(comm)
        obj = Objective()
        for s, X, lab in bunches(g, B):
            net.train_bunch(obj, DeviceArray.from_numpy(X), DeviceArray.vector(lab))
        runs.append((net_params(net), obj.stats()))
    (p0, s0), (p1, s1) = runs
    for k in p0:
        np.testing.assert_allclose(p1[k], p0[k], rtol=1e-5, atol=1e-7, err_msg=k)
    assert s1[1] == s0[1] and s1[2] == s0[2]
    np.testing.assert_allclose(s1[0], s0[0], rtol=1e-6)
