"""CPU-side checks that make the restatement of tests/stack_cases.py trustworthy on its own (no GPU): its one-step
parameter change is the finite-difference gradient of the float64 cross-entropy for every parameter of every layer of
every stack order, and run in float32 it stays within a quarter of the GPU comparison's tolerance over every
trajectory tests/test_gpu_stacks.py compares -- so the inputs leave that tolerance room.  Both tests print their
worst ratios; tests/stack_cases.py's docstring holds a copy."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stack_cases as cases  # noqa: E402
from tnet_amd import formats  # noqa: E402

ORDER_IDS = [cases.order_id(o) for o in cases.ORDERS]
CONSTS_IDS = [cases.consts_id(c) for c in cases.CONSTS]
FD_H, FD_RTOL = 1e-6, 1e-5
# Rounding floor of the difference quotient.  A row's loss (about 2) comes out of five matrix products of some
# hundred terms each and carries a few times 1e-15 of rounding; the rows' loss differences are formed per row and
# then summed, so the quotient's rounding is about sqrt(32) * 4e-15 / (2 h) = 1e-8.  The truncation term, O(h^2) =
# 1e-12 times a third derivative of order one, lies far below it.  Measured worst |fd - g| / (rtol |g| + floor): 0.35.
FD_FLOOR = 1e-8


def test_case_geometry():
    # every ordered pair of the three layers is adjacent in one order
    pairs = {(o[i], o[i + 1]) for o in cases.ORDERS for i in range(2)}
    assert pairs == {(a, b) for a in cases.KINDS for b in cases.KINDS if a != b}
    assert all(sorted(o) == sorted(cases.KINDS) for o in cases.ORDERS) and len(set(cases.ORDERS)) == 6
    assert all(w % cases.N_INST == 0 and w % 32 and w <= 160 for w in cases.WIDTHS) and len(set(cases.WIDTHS)) == 4
    assert cases.ROWS == (32, 19, 64, 1)
    for order in cases.ORDERS:
        L = cases.layers(order)
        assert [l.tag for l in L] == ["<biasedlinearity>", "<sigmoid>", f"<{order[0]}linearity>", "<sigmoid>",
                                      f"<{order[1]}linearity>", "<sigmoid>", f"<{order[2]}linearity>", "<sigmoid>",
                                      "<biasedlinearity>", "<softmax>"]
        assert all(a.n_out == b.n_in for a, b in zip(L, L[1:])) and L[0].n_in == cases.D_IN and L[-1].n_out == cases.N_CLS
        for kind in cases.KINDS:
            l = L[cases.index_of(order, kind)]
            assert l.tag == f"<{kind}linearity>"
            if kind == "shared":
                # windows narrower than a tile whose origins leave 16-byte alignment on both sides
                wi, wo = l.W.shape
                assert l.extra["n_inst"] == 3 and wi < 64 and wo < 64 and (wi * 4) % 16 and (wo * 4) % 16
            elif kind == "discrete":
                ins, outs = [W.shape[0] for W in l.extra["Ws"]], [W.shape[1] for W in l.extra["Ws"]]
                assert len(set(ins)) == 3 and len(set(outs)) == 3
                assert any(o % 4 for o in np.cumsum(ins)[:-1]) and any(o % 4 for o in np.cumsum(outs)[:-1])
                assert min(ins) < 64 < max(ins) and min(outs) < 64       # a block narrower than a tile beside one wider
            else:
                assert l.n_out % 32 and 0.4 < l.extra["mask"].mean() < 0.6 and not l.W[l.extra["mask"] == 0].any()
    # the text the library reads holds the same float32 values
    L = cases.layers(cases.ORDERS[0])
    back = formats.read_nnet(cases.net_text(L))
    for a, b in zip(L, back):
        assert a.tag == b.tag
        if a.W is not None:
            np.testing.assert_array_equal(a.W, b.W)


@pytest.mark.parametrize("c", cases.CONSTS, ids=CONSTS_IDS)
def test_constants_put_the_soft_threshold_at_a_tenth_of_a_weight(c):
    k = cases.consts(c)
    assert k["l1"] > 0 and abs(k["lr"] * k["l1"] * (1 if k["gdf"] else cases.ROWS[0]) - cases.L1_THRESHOLD) < 1e-12
    assert abs(k["lr"] * (1 if k["gdf"] else cases.ROWS[0]) - cases.LR) < 1e-12


def _params(c):
    """(name, array, divisor factor, mask or None) of a component's parameters; the arrays are the oracle's own"""
    n = c.get("n", 1)
    if "Ws" in c:
        out = [(f"W_{j}", W, n, None) for j, W in enumerate(c["Ws"])]
    else:
        out = [("W", c["W"], n, c.get("mask"))]
    return out + [("b", c["b"], n, None)]


@pytest.mark.parametrize("order", cases.ORDERS, ids=ORDER_IDS)
def test_one_step_change_is_the_finite_difference_gradient(order):
    """momentum 0, weight cost 0, L1 0, GradDivFrm off: (parameter after one step - before) / -lr -- for the shared
    layer / (-lr / N) -- is the central-difference gradient of the summed cross-entropy, for every parameter of
    every layer; for a masked sparse weight it is 0.  rtol 1e-5 with the rounding floor FD_FLOOR (above)."""
    L = cases.layers(order)
    X, lab = cases.bunches()[0]
    lr = 0.1
    k = dict(lr=lr, mmt=0.0, wc=0.0, l1=0.0, gdf=False)
    ref = cases.Oracle(L)
    before = {key: np.array(v, copy=True) for key, v in ref.state().items()}
    ref.step(X, lab, k)
    after = ref.state()
    probe = cases.Oracle(L)
    acts = probe.forward(X)
    worst, checked = 0.0, 0
    for i, c in enumerate(probe.C):
        if c["tag"] not in cases.UPDATABLE:
            continue
        for name, arr, n, mask in _params(c):
            fd = np.zeros_like(arr)
            for idx in np.ndindex(arr.shape):
                old = arr[idx]
                arr[idx] = old + FD_H
                up = probe.row_losses(probe.forward(None, i, acts[i])[-1], lab)
                hi = arr[idx]
                arr[idx] = old - FD_H
                dn = probe.row_losses(probe.forward(None, i, acts[i])[-1], lab)
                fd[idx] = (up - dn).sum() / (hi - arr[idx])
                arr[idx] = old
            if mask is not None:
                assert np.abs(fd[mask == 0]).max() > 1e-4   # the loss does depend on them: the update must not
                fd = np.where(mask != 0, fd, 0.0)
            key = f"{i}.{name}"
            g = (after[key] - before[key]) / (-lr / n)
            ratio = float((np.abs(fd - g) / (FD_RTOL * np.abs(g) + FD_FLOOR)).max())
            worst = max(worst, ratio)
            checked += arr.size
            assert np.abs(g).max() > 1e-4, key
            assert ratio <= 1.0, f"{key}: |fd - g| / (rtol |g| + floor) = {ratio:.3g}"
    print(f"finite differences {cases.order_id(order)}: {checked} parameters, worst |fd - g| / (1e-5 |g| + 1e-8) = "
          f"{worst:.3g}")
    assert checked == sum(v.size for key, v in before.items() if not cases.is_exact(key) and not key.endswith("accu"))


# ---- float32 headroom: every trajectory tests/test_gpu_stacks.py compares with the restatement
def _headroom(L, k, data, **kw):
    s64, r64 = cases.trajectory(L, k, data, **kw)
    s32, r32 = cases.trajectory(L, k, data, dtype=np.float32, **kw)
    worst = 0.0
    near_keys = set()
    if r64.near is not None and r64.near.any():
        near_keys = {f"{kw['mask_update'][1]}.{n}" for n in ("W", "mask")}
    for (o64, st64), (o32, st32) in zip(s64, s32):
        for a, b in zip(o64, o32):
            assert b.dtype == np.float32
            worst = max(worst, float((np.abs(b - a) / (cases.ATOL + cases.RTOL * np.abs(a))).max()))
        for key, a in st64.items():
            b = st32[key]
            if cases.is_exact(key):
                if key not in near_keys:
                    np.testing.assert_array_equal(a, b, err_msg=key)
                continue
            assert b.dtype == np.float32
            r = np.abs(b - a) / (cases.ATOL + cases.RTOL * np.abs(a))
            if key in near_keys:
                r = r[~r64.near]
            worst = max(worst, float(r.max()))
    worst = max(worst, abs(r32.xent - r64.xent) / (1e-5 * abs(r64.xent)))   # the objective's sum: rtol 1e-5
    assert r32.frames == r64.frames == sum(len(lab) for _, lab in data)
    return worst, s64, r64


@pytest.mark.parametrize("c", cases.CONSTS, ids=CONSTS_IDS)
@pytest.mark.parametrize("order", cases.ORDERS, ids=ORDER_IDS)
def test_float32_restatement_stays_within_a_quarter_of_the_tolerance(order, c):
    """four bunches of 32, 19, 64 and 1 rows; also: the steps move every parameter of every layer -- the first
    layer's included, four sigmoids below the objective -- by at least ten times the comparison's tolerance, so a
    wrong error reaching a layer cannot hide inside it"""
    L = cases.layers(order)
    worst, steps, ref = _headroom(L, cases.consts(c), cases.bunches())
    print(f"float32 headroom {cases.order_id(order)} {cases.consts_id(c)}: worst deviation / tolerance = {worst:.3g}")
    assert worst <= cases.HEADROOM
    first = cases.Oracle(L).state()
    for key, v in steps[-1][1].items():
        assert np.isfinite(v).all()
        if not cases.is_exact(key) and not key.endswith("accu"):
            moved = np.abs(v - first[key]) / (cases.ATOL + cases.RTOL * np.abs(first[key]))
            assert moved.max() >= 10.0, f"{key} moved by {moved.max():.3g} tolerances"
    i = cases.index_of(order, "sparse")
    W, mask = steps[-1][1][f"{i}.W"], steps[-1][1][f"{i}.mask"]
    # the soft threshold took its share and left survivors; the steps never touch the mask
    assert (W[mask != 0] == 0).mean() > 0.02 and (W > 0).any() and (W < 0).any() and not W[mask == 0].any()
    np.testing.assert_array_equal(mask, L[i].extra["mask"])
    assert steps[-1][1][f"{i}.nframes"][0] == sum(cases.ROWS)


def test_mask_update_mid_trajectory_stays_under_the_excluded_cap():
    """UpdateMask between step 2 and step 3: tests/test_gpu_stacks.py excludes from the mask comparison the elements
    whose restated |W| lies within the tolerance of the sparsify threshold.  For the chosen seed the restatement alone
    has none (cap: 1 %), the update does cut weights, and the float32 run decides every bit as float64 does."""
    L = cases.layers(cases.MASK_ORDER)
    i = cases.index_of(cases.MASK_ORDER, "sparse")
    worst, steps, ref = _headroom(L, cases.consts(cases.MASK_CONSTS), cases.bunches(), mask_update=(2, i))
    print(f"float32 headroom mask update: near {int(ref.near.sum())} of {ref.near.size}, worst deviation / tolerance = "
          f"{worst:.3g}")
    assert ref.near.mean() <= cases.MASK_EXCLUDED_CAP
    assert not ref.near.any()           # nothing is excluded at this seed
    assert worst <= cases.HEADROOM
    m0, m1 = L[i].extra["mask"], steps[-1][1][f"{i}.mask"]
    assert (m1 != m0).any() and m1.sum() > 0.5 * m0.sum() and not (m1 > m0).any()
    np.testing.assert_array_equal(steps[1][1][f"{i}.mask"], m0)
    np.testing.assert_array_equal(steps[2][1][f"{i}.mask"], m1)
    assert not steps[-1][1][f"{i}.W"][m1 == 0].any()


STOPPER_CASES = {"frozen-below-B": "0,0,1,1,1", "frozen-middle": "1,1,0,1,1"}


@pytest.mark.parametrize("order", cases.ORDERS[:3], ids=ORDER_IDS[:3])
@pytest.mark.parametrize("name", STOPPER_CASES)
def test_stopper_rule_of_the_restatement(name, order):
    """factors that freeze the two layers below B make B the stopper; a factor 0 on B alone leaves the first layer
    the stopper and the error still flows through B to the trained layers below"""
    L = cases.layers(order)
    factors = STOPPER_CASES[name]
    ref = cases.Oracle(L)
    rates, stopper = ref.learn_rates(0.5, cases.parse_factors(factors))
    assert stopper == (4 if name == "frozen-below-B" else 0)
    assert [r for r in rates if r is not None] == [0.5 * f for f in cases.parse_factors(factors)]
    worst, steps, ref = _headroom(L, cases.consts(cases.CONSTS[1]), cases.bunches(), factors=factors)
    print(f"float32 headroom {name} {cases.order_id(order)}: worst deviation / tolerance = {worst:.3g}")
    assert worst <= cases.HEADROOM
    first, last = cases.Oracle(L).state(), steps[-1][1]
    frozen = (0, 2) if name == "frozen-below-B" else (4,)
    for key, v in last.items():
        if int(key.split(".")[0]) in frozen:
            np.testing.assert_array_equal(v, first[key], err_msg=key)      # accu and the frame count included
        elif not cases.is_exact(key):
            assert np.abs(v - first[key]).max() > 1e-4, key


def test_crossval_and_trainer_and_blockarray_trajectories_have_headroom(golden_dir):
    L = cases.layers(cases.ORDERS[0])
    k = cases.consts(cases.CONSTS[1])
    worst, steps, ref = _headroom(L, k, cases.bunches(), train=False)
    print(f"float32 headroom crossval: worst deviation / tolerance = {worst:.3g}")
    assert worst <= cases.HEADROOM
    first = cases.Oracle(L).state()
    for key, v in steps[-1][1].items():
        np.testing.assert_array_equal(v, first[key], err_msg=key)
    worst, _, _ = _headroom(L, k, cases.bunches((32, 32, 32, 32)))
    print(f"float32 headroom four bunches of 32 (trainer): worst deviation / tolerance = {worst:.3g}")
    assert worst <= cases.HEADROOM
    # the block array's output (the fixture's reference forward) is the restatement's input
    g = np.load(os.path.join(golden_dir, "blockarray_fwd.npz"))
    assert g["X"].shape == (33, 28) and g["Y"].shape == (33, 17)
    lab = cases.blockarray_labels()
    data = [(g["Y"][a:b], lab[a:b]) for a, b in cases.BLOCKARRAY_ROWS]
    U = cases.blockarray_upper()
    worst, steps, _ = _headroom(U, cases.consts(cases.BLOCKARRAY_CONSTS), data)
    print(f"float32 headroom block array below the stopper: worst deviation / tolerance = {worst:.3g}")
    assert worst <= cases.HEADROOM
    first = cases.Oracle(U).state()
    for key in ("0.W", "0.b", "2.W", "2.b"):
        assert np.abs(steps[-1][1][key] - first[key]).max() > 1e-4, key
