"""<sharedlinearity>, <discretelinearity> and <sparselinearity> in the MIDDLE of a trained stack (tests/stack_cases.py:
<biasedlinearity>, sigmoid, A, sigmoid, B, sigmoid, C, sigmoid, <biasedlinearity>, softmax for six orders of the
three layers): what CuNetwork composes, not what a kernel computes.  Here every special layer's Backpropagate output
is consumed by a trained layer below, special layers feed each other and read another component's output buffer, the
bunch size changes from step to step (32, 19, 64, 1 rows), learn-rate factors put the stopper on and below a special
layer, cross-validation runs over these nets, and the data-parallel split step has backward passes below its applies.

The reference is the float64 restatement of tests/stack_cases.py, which tests/test_stack_cases_cpu.py checks against
finite differences of the cross-entropy and, run in float32, against a quarter of the tolerance used here.

Tolerances
  against the restatement    the project's network-level rtol 2e-4 / atol 2e-6 for every component's output, every
                             parameter and the sparse layer's accu; mask and frame count exact; the objective's sum
                             rtol 1e-5 (tests/test_gpu_shared.py, test_gpu_discrete.py, test_gpu_sparse.py)
  frozen layers, cross-validation    bit-equal to the initial state
  one rank, split step against the fused step of the same library    tests/test_gpu_dp_layers.py's rtol 1e-5 /
                             atol 1e-7, mask and frame count exact
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stack_cases as cases  # noqa: E402
from tnet_amd import Comm, DeviceArray, Network, Objective, TnetError, Trainer  # noqa: E402
from tnet_amd._lib import check, lib  # noqa: E402

ORDER_IDS = [cases.order_id(o) for o in cases.ORDERS]
CONSTS_IDS = [cases.consts_id(c) for c in cases.CONSTS]
MAX_ROWS = max(cases.ROWS)


def make_net(L, k, factors=None, text=None):
    net = Network(text=cases.net_text(L) if text is None else text)
    cases.configure(net, k, factors)
    net.keep_output(True)
    return net


def component_outputs(net, rows):
    """every component's output buffer.  The host buffer holds more rows than the largest bunch and starts as NaN:
    a component that kept the row count of an earlier, larger bunch writes past `rows` and is caught here"""
    outs = []
    for i, (_, _, no) in enumerate(net.components()):
        buf = np.full((MAX_ROWS + 1, no), np.nan, np.float32)
        check(lib().tnet_net_output(net.h, i, buf.ctypes.data, no), "output")
        assert np.isnan(buf[rows:]).all(), f"component {i} holds more than the bunch's {rows} rows"
        outs.append(buf[:rows])
    return outs


def assert_outputs(got, want, what, first=0):
    assert len(got) == first + len(want)
    for i, (g, w) in enumerate(zip(got[first:], want)):
        np.testing.assert_allclose(g, w, rtol=cases.RTOL, atol=cases.ATOL, err_msg=f"{what}: output of component {first + i}")


def assert_state(got, want, what, shift=0, exclude=None, rtol=cases.RTOL, atol=cases.ATOL):
    """got: cases.state(net); want: the restatement's (component indices lower by `shift`); exclude: {key: bool
    array} of elements left out of that key's comparison"""
    want = {f"{int(key.split('.')[0]) + shift}.{key.split('.', 1)[1]}": v for key, v in want.items()}
    assert set(got) == set(want), what
    worst = 0.0
    for key, w in want.items():
        g = got[key]
        keep = ~exclude[key] if exclude and key in exclude else np.ones(w.shape, bool)
        if cases.is_exact(key):
            np.testing.assert_array_equal(g[keep], w[keep], err_msg=f"{what}: {key}")
        else:
            d = np.abs(g.astype(np.float64) - w)[keep] / (atol + rtol * np.abs(w[keep]))
            worst = max(worst, float(d.max()) if d.size else 0.0)
            np.testing.assert_allclose(g[keep], w[keep], rtol=rtol, atol=atol, err_msg=f"{what}: {key}")
    return worst


def assert_bit_equal(got, want, keys, what):
    for key in keys:
        np.testing.assert_array_equal(got[key].view(np.uint32) if got[key].dtype == np.float32 else got[key],
                                      want[key].view(np.uint32) if want[key].dtype == np.float32 else want[key],
                                      err_msg=f"{what}: {key}")


@functools.lru_cache(maxsize=None)
def reference(order, c, factors=None, train=True, rows=cases.ROWS, mask_update=None):
    """the restatement's trajectory, computed once per case and shared"""
    steps, ref = cases.trajectory(cases.layers(order), cases.consts(c), cases.bunches(rows), factors=factors,
                                  train=train, mask_update=mask_update)
    for outs, st in steps:
        for v in list(outs) + list(st.values()):
            v.setflags(write=False)
    return steps, ref


def run_steps(net, obj, data, steps, what, train=True):
    worst = 0.0
    for s, (X, lab) in enumerate(data):
        dX, dL = DeviceArray.from_numpy(X), DeviceArray.vector(lab)
        net.train_bunch(obj, dX, dL, train=train)
        assert_outputs(component_outputs(net, len(lab)), steps[s][0], f"{what} step {s}")
        worst = max(worst, assert_state(cases.state(net), steps[s][1], f"{what} step {s}"))
    return worst


def assert_objective(obj, ref, data):
    err, frames, _ = obj.stats()
    assert frames == ref.frames == sum(len(lab) for _, lab in data)
    np.testing.assert_allclose(err, ref.xent, rtol=1e-5)


# ====================================================================================== the trained stack
@pytest.mark.parametrize("c", cases.CONSTS, ids=CONSTS_IDS)
@pytest.mark.parametrize("order", cases.ORDERS, ids=ORDER_IDS)
def test_train_bunch_vs_restatement(order, c):
    """after each of the four bunches every component's output, every layer's parameters, the sparse layer's mask
    (exact), accu and frame count; after the four the objective's sum and frame count"""
    steps, ref = reference(order, c)
    net, obj = make_net(cases.layers(order), cases.consts(c)), Objective()
    data = cases.bunches()
    worst = run_steps(net, obj, data, steps, cases.order_id(order))
    print(f"{cases.order_id(order)} {cases.consts_id(c)}: worst parameter deviation / tolerance {worst:.3g}")
    assert_objective(obj, ref, data)


def test_mask_update_mid_trajectory():
    """sparse_update_mask between step 2 and step 3.  A mask bit (and its weight) is left out of the comparison only
    where the restated |W| lies within the tolerance of the sparsify threshold; tests/test_stack_cases_cpu.py asserts
    that the restatement has no such element at this seed (cap: MASK_EXCLUDED_CAP)"""
    order, c = cases.MASK_ORDER, cases.MASK_CONSTS
    i = cases.index_of(order, "sparse")
    steps, ref = reference(order, c, mask_update=(2, i))
    assert ref.near.mean() <= cases.MASK_EXCLUDED_CAP
    net, obj = make_net(cases.layers(order), cases.consts(c)), Objective()
    data = cases.bunches()
    exclude = {f"{i}.mask": ref.near, f"{i}.W": ref.near}
    mask0 = cases.layers(order)[i].extra["mask"]
    for s, (X, lab) in enumerate(data):
        if s == 2:
            net.sparse_update_mask(i)
            W, _, mask, _, nframes = net.sparse_params(i)
            assert (mask != mask0).any() and not (mask > mask0).any() and not W[mask == 0].any()
            assert nframes == sum(cases.ROWS[:2])
        dX, dL = DeviceArray.from_numpy(X), DeviceArray.vector(lab)
        net.train_bunch(obj, dX, dL)
        if not ref.near.any():   # (an excluded bit decided the other way would move the outputs above it)
            assert_outputs(component_outputs(net, len(lab)), steps[s][0], f"mask update step {s}")
        assert_state(cases.state(net), steps[s][1], f"mask update step {s}", exclude=exclude if s >= 2 else None)
    assert_objective(obj, ref, data)


STOPPER_CASES = {"frozen-below-B": ("0,0,1,1,1", (0, 2)), "frozen-middle": ("1,1,0,1,1", (4,))}


@pytest.mark.parametrize("order", cases.ORDERS[:3], ids=ORDER_IDS[:3])
@pytest.mark.parametrize("name", STOPPER_CASES)
def test_stopper_and_frozen_layers(name, order):
    """frozen-below-B: factors freeze the first layer and A, so the stopper sits on the special layer B (each of the
    three in turn), which then runs no backward pass.  frozen-middle: factor 0 on B alone; its backward pass still
    carries the error to A and the first layer, its own parameters -- and a sparse B's accu and frame count -- stay.
    Frozen parameters are bit-unchanged, trained ones match the restatement."""
    factors, frozen = STOPPER_CASES[name]
    c = cases.CONSTS[1]
    steps, ref = reference(order, c, factors=factors)
    net, obj = make_net(cases.layers(order), cases.consts(c), factors), Objective()
    initial = cases.state(net)
    data = cases.bunches()
    run_steps(net, obj, data, steps, f"{name} {cases.order_id(order)}")
    assert_objective(obj, ref, data)
    got = cases.state(net)
    frozen_keys = [key for key in got if int(key.split(".")[0]) in frozen]
    assert len(frozen_keys) >= 2 * len(frozen)
    assert_bit_equal(got, initial, frozen_keys, name)
    for key in set(got) - set(frozen_keys):
        if not key.endswith(".mask"):
            assert not np.array_equal(got[key], initial[key]), key
    if order[1] == "sparse" and name == "frozen-middle":
        assert got["4.nframes"][0] == 0 and not got["4.accu"].any()


def test_crossval_leaves_everything():
    """train=False over the four bunches: every parameter, mask and accu bit-equal to the initial state, outputs and
    objective the restatement's forward"""
    order, c = cases.ORDERS[0], cases.CONSTS[1]
    steps, ref = reference(order, c, train=False)
    net, obj = make_net(cases.layers(order), cases.consts(c)), Objective()
    initial = cases.state(net)
    data = cases.bunches()
    run_steps(net, obj, data, steps, "crossval", train=False)
    assert_bit_equal(cases.state(net), initial, list(initial), "crossval")
    assert_objective(obj, ref, data)


def test_trainer_reproduces_train_bunch():
    """Trainer(randomize=False) over four concatenated bunches of 32 rows against the train_bunch loop over the same
    rows; the loop also against the restatement (equal bunch sizes: every error buffer is reused as it is, so a
    backward pass that accumulated into it would show here)"""
    order, c, rows = cases.ORDERS[0], cases.CONSTS[1], (32, 32, 32, 32)
    steps, ref = reference(order, c, rows=rows)
    data = cases.bunches(rows)
    L, k = cases.layers(order), cases.consts(c)
    loop, lobj = make_net(L, k), Objective()
    run_steps(loop, lobj, data, steps, "train_bunch loop")
    assert_objective(lobj, ref, data)
    net, obj = make_net(L, k), Objective()
    tr = Trainer(net, obj, bunchsize=32, cachesize=128, seed=1, randomize=False)
    tr.add_utterance(np.concatenate([X for X, _ in data]), np.concatenate([lab for _, lab in data]))
    tr.finish()
    assert tr.steps == 4
    worst = assert_state(cases.state(net), cases.state(loop), "trainer against the loop")
    print(f"trainer against the train_bunch loop: worst deviation / tolerance {worst:.3g}")
    assert_objective(obj, ref, data)


# ====================================================================================== one rank: split step = fused step
DP_CONSTS = (0.5, 1e-3, True)     # tests/dp_layers_cases.py's momentum and weight cost, whose one-rank bounds these are
_COMMS = {}


def one_rank_comm(transport):
    """communicators are kept for the module: "host" (all-reduce over one rank: nothing to add), "rccl", and
    "rccl-shard" (TNET_DP_SHARD=1 is read when the communicator is made)"""
    if transport not in _COMMS:
        if transport == "host":
            _COMMS[transport] = Comm.host(0, 1, lambda a: None)
        else:
            old = os.environ.get("TNET_DP_SHARD")
            os.environ["TNET_DP_SHARD"] = "1" if transport == "rccl-shard" else "0"
            try:
                _COMMS[transport] = Comm(0, 1, Comm.unique_id())
            finally:
                if old is None:
                    del os.environ["TNET_DP_SHARD"]
                else:
                    os.environ["TNET_DP_SHARD"] = old
    return _COMMS[transport]


def freeze_sparse(order):
    """factors with 0 on the sparse layer only"""
    f = ["1"] * 5
    f[1 + order.index("sparse")] = "0"
    return ",".join(f)


def train(order, factors, comm=None):
    net, obj = make_net(cases.layers(order), cases.consts(DP_CONSTS), factors), Objective()
    if comm is not None:
        net.set_comm(comm)
    data = cases.bunches()
    for s, (X, lab) in enumerate(data):
        if comm is not None and s == len(data) - 1:
            comm.capture(True)      # the last step's gradient blocks, copied on the reduction's stream
        dX, dL = DeviceArray.from_numpy(X), DeviceArray.vector(lab)
        net.train_bunch(obj, dX, dL)
    if comm is not None:
        # the split step did run: W and bias gradient of every trained layer went through the exchange
        trained = sum(1 for f in (factors or "1,1,1,1,1").split(",") if float(f) > 0)
        blocks = comm.captured()
        comm.capture(False)
        assert len(blocks) == 2 * trained
        for local, reduced in blocks:
            assert np.isfinite(local).all() and local.any()
    return net, obj


@functools.lru_cache(maxsize=None)
def fused_state(order, factors):
    """the fused single-process steps (no communicator), computed once and shared"""
    net, obj = train(order, factors)
    st = cases.state(net)
    for v in st.values():
        v.setflags(write=False)
    return st, obj.stats()


SHARD_ORDER = cases.ORDERS[1]      # the sparse layer in the middle: frozen, its backward pass still runs
ONE_RANK = [(o, t, None) for o in cases.ORDERS for t in ("host", "rccl")] + \
           [(SHARD_ORDER, "rccl-shard", freeze_sparse(SHARD_ORDER))]


@pytest.mark.parametrize("order,transport,factors", ONE_RANK,
                         ids=[f"{cases.order_id(o)}-{t}" for o, t, _ in ONE_RANK])
def test_one_rank_split_step_equals_fused_step(order, transport, factors):
    """the four bunches, momentum 0.5, weight cost and L1 on: the split ComputeGradient -> reduce -> ApplyGradient
    step of a one-rank communicator against the fused Update() step.  Every apply but the first layer's runs on the
    exchange's stream beside the backward passes of the layers below it.  rccl-shard: the sharded apply, on a net
    whose sparse layer a factor 0 takes out of the trained set (a trained one is refused: below)."""
    want, want_stats = fused_state(order, factors)
    net, obj = train(order, factors, one_rank_comm(transport))
    got = cases.state(net)
    worst = assert_state(got, want, f"{cases.order_id(order)} {transport}", rtol=1e-5, atol=1e-7)
    print(f"{cases.order_id(order)} {transport}: worst deviation / (1e-7 + 1e-5 |fused|) {worst:.3g}")
    i = cases.index_of(order, "sparse")
    assert got[f"{i}.nframes"][0] == (0 if factors else sum(cases.ROWS))
    np.testing.assert_allclose(obj.stats()[0], want_stats[0], rtol=1e-5)
    assert obj.stats()[1] == want_stats[1] == sum(cases.ROWS)


def test_sharded_apply_still_refuses_a_trained_sparse_layer():
    """the same stack with the sparse layer trained: refused before anything is enqueued, the network is unchanged"""
    net, obj = make_net(cases.layers(SHARD_ORDER), cases.consts(DP_CONSTS)), Objective()
    initial = cases.state(net)
    net.set_comm(one_rank_comm("rccl-shard"))
    X, lab = cases.bunches()[0]
    dX, dL = DeviceArray.from_numpy(X), DeviceArray.vector(lab)
    with pytest.raises(TnetError, match="cannot take the sharded apply"):
        net.train_bunch(obj, dX, dL)
    assert_bit_equal(cases.state(net), initial, list(initial), "refused step")
    assert obj.stats()[1] == 0


# ====================================================================================== a block array below the stopper
def test_blockarray_below_the_stopper(golden_dir):
    """<blockarray> 17 28 of tests/golden/blockarray_fwd.npz, <sparselinearity> 17 -> 12, sigmoid, <biasedlinearity>
    12 -> 9, softmax; two steps on rows of the fixture's input.  The block array has no backward pass and no update:
    its factor 0 puts the stopper on the sparse layer.  Its output is the fixture's forward; the layers above train to
    the restatement's values, the restatement taking the fixture's forward as its input."""
    g = np.load(os.path.join(golden_dir, "blockarray_fwd.npz"))
    U, k = cases.blockarray_upper(), cases.consts(cases.BLOCKARRAY_CONSTS)
    lab = cases.blockarray_labels()
    net = make_net(None, k, cases.BLOCKARRAY_FACTORS, text=str(g["nnet"]).rstrip("\n") + "\n" + cases.net_text(U))
    assert [t for t, _, _ in net.components()] == ["<blockarray>", "<sparselinearity>", "<sigmoid>",
                                                   "<biasedlinearity>", "<softmax>"]
    data = [(g["Y"][a:b], lab[a:b]) for a, b in cases.BLOCKARRAY_ROWS]
    steps, ref = cases.trajectory(U, k, data)
    obj = Objective()
    for s, (a, b) in enumerate(cases.BLOCKARRAY_ROWS):
        dX, dL = DeviceArray.from_numpy(np.ascontiguousarray(g["X"][a:b])), DeviceArray.vector(lab[a:b])
        net.train_bunch(obj, dX, dL)
        outs = component_outputs(net, b - a)
        np.testing.assert_allclose(outs[0], g["Y"][a:b], rtol=cases.RTOL, atol=cases.ATOL)
        assert_outputs(outs, steps[s][0], f"block array step {s}", first=1)
        assert_state(cases.state(net), steps[s][1], f"block array step {s}", shift=1)
    assert_objective(obj, ref, data)
