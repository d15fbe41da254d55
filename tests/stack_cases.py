"""Cases shared by tests/test_gpu_stacks.py and tests/test_stack_cases_cpu.py: networks with a <sharedlinearity>, a
<discretelinearity> and a <sparselinearity> in the MIDDLE of a trained stack, their SGD constants, their bunches, and
one float64 restatement of CuNetwork::Backpropagate for a net of any order of <biasedlinearity>, <sharedlinearity>,
<discretelinearity>, <sparselinearity>, <sigmoid> and <softmax>.  numpy only: nothing here touches the GPU.

The stack is  <biasedlinearity> 23 -> 111, sigmoid, A 111 -> 114, sigmoid, B 114 -> 117, sigmoid, C 117 -> 105, sigmoid,
<biasedlinearity> 105 -> 9, softmax  with {A, B, C} a permutation of the three layers: the three rotations of both
orientations, so every ordered pair of the three is adjacent once.  Every special layer is fed by another component's
output buffer, its error output is consumed by a trained layer below, and no two interfaces have the same width.
At these widths
  shared    3 instances of 37 -> 38, 38 -> 39 or 39 -> 35: windows narrower than a tile, origins 148, 152, 156 and 140
            bytes apart, none a multiple of 16
  discrete  ragged blocks (39, w_in - 44, 5) -> (64, 7, w_out - 71): stripe origins 39 and w_in - 5 / 64 and 71 are
            unaligned, the middle block is wider than the 64-tile on its input side (67, 70 or 73) and 7 wide on its
            output side
  sparse    n_out 114, 117 or 105 at mask density 0.5: four mask words per row, the last one partial (18, 21, 9 bits)
Bunches of 32, 19, 64 and 1 rows: the second shrinks every buffer, the third grows past the first allocation, the last
is a single row.

Per-layer constants of the restatement (tests/test_gpu_shared.py, test_gpu_discrete.py,
test_gpu_sparse.py and tests/dp_layers_cases.py restate the same reference formulas)
  every layer   Ndiv = (GradDivFrm ? rows : 1) / (1 - momentum); scale = -lr / Ndiv; frm = GradDivFrm ? 1 : rows
  biased        l2 = -lr * wc * frm                                  (cuBiasedLinearity.cc:46-64)
  shared        Ndiv *= N (the gradient is a sum over the N instances); l2 = -lr * wc   (cuSharedLinearity.cc:65-94)
  discrete      per block; l2 = -lr * wc, no rows factor             (cuDiscreteLinearity.cc:45-78)
  sparse        momentum -> accu += corrW -> mask -> L1 soft threshold lr*l1*frm -> L2 (-lr*wc*frm) -> bias
                                                                     (cuSparseLinearity.cc:28-63)
Per step (CuNetwork::Backpropagate, cuNetwork.cc): forward; then top down to the stopper -- the first updatable
component with a positive learn rate (CuNetwork::SetLearnRate, cuNetwork.cc:80-134) -- each component's error
through its PRE-update weights with beta 0 (not for the stopper), then that component's update if its learn rate is
positive.

Measured by tests/test_stack_cases_cpu.py (it prints them; copied here)
  finite differences   h = 1e-6 central differences of the float64 summed cross-entropy against the restatement's
                       one-step parameter change / -lr (shared: / (-lr / N)): worst |fd - g| / (1e-5 |g| + 1e-8) over
                       every parameter of every layer, per order:
                       shared-discrete-sparse 0.34, discrete-sparse-shared 0.30, sparse-shared-discrete 0.35,
                       sparse-discrete-shared 0.27, discrete-shared-sparse 0.28, shared-sparse-discrete 0.31
  float32 headroom     the restatement run in float32 numpy against float64 over the four steps, worst deviation /
                       (2e-6 + 2e-4 |ref|) over every output, parameter and accu, and the objective's sum against its
                       rtol 1e-5 (bound: 0.25), worst order per constants: mmt0-wc0-nodiv 0.094,
                       mmt0.9-wc0.001-div 0.107, mmt0-wc0.001-nodiv 0.094, mmt0.9-wc0-div 0.094; mask update
                       mid-trajectory 0.071; frozen layers 0.105; cross-validation 0.044; four bunches of 32 rows
                       0.055; block array below the stopper 0.021
"""
import io

import numpy as np

from tnet_amd import formats

N_CLS = 9
D_IN = 23
WIDTHS = (111, 114, 117, 105)         # the interfaces first -> A -> B -> C -> top: multiples of 3, none of 32
KINDS = ("shared", "discrete", "sparse")
ORDERS = (("shared", "discrete", "sparse"), ("discrete", "sparse", "shared"), ("sparse", "shared", "discrete"),
          ("sparse", "discrete", "shared"), ("discrete", "shared", "sparse"), ("shared", "sparse", "discrete"))
N_INST = 3
DENSITY = 0.5
ROWS = (32, 19, 64, 1)
INIT_SEED, DATA_SEED = 90, 91
# the project's four (momentum, weight cost, GradDivFrm) combinations (tests/test_gpu_shared.py, test_gpu_discrete.py)
CONSTS = ((0.0, 0.0, False), (0.9, 1e-3, True), (0.0, 1e-3, False), (0.9, 0.0, True))
LR = 0.5                              # per-frame rate; see consts()
L1_THRESHOLD = 0.01                   # a tenth of a typical weight (tests/dp_layers_cases.py)
SPARSIFY = 1e-3                       # CuSparseLinearity's default weight threshold of UpdateMask
RTOL, ATOL = 2e-4, 2e-6               # the project's network-level tolerance
HEADROOM = 0.25                       # the float32 restatement must stay within this share of it
MASK_EXCLUDED_CAP = 0.01
MASK_ORDER, MASK_CONSTS = ORDERS[1], CONSTS[1]   # the mask-update case: the sparse layer in the middle
UPDATABLE = ("<biasedlinearity>", "<sharedlinearity>", "<discretelinearity>", "<sparselinearity>")


def order_id(order):
    return "-".join(order)


def consts_id(c):
    return f"mmt{c[0]:g}-wc{c[1]:g}-{'div' if c[2] else 'nodiv'}"


def special(kind, w_in, w_out, seed):
    """[layer, <sigmoid>] of one special layer w_in -> w_out; zero biases"""
    if kind == "shared":
        return formats.gen_shared_init(N_INST, w_in // N_INST, w_out // N_INST, seed=seed, negbias=False)
    if kind == "discrete":
        return formats.gen_discrete_init((39, w_in - 44, 5), (64, 7, w_out - 71), seed=seed, negbias=False)
    if kind == "sparse":
        return formats.gen_sparse_init(w_in, w_out, seed=seed, density=DENSITY, negbias=False)
    raise ValueError(kind)


def layers(order, seed=INIT_SEED):
    """Zero biases below the top (negbias=False): with the --negbias draw (-4) the sigmoids sit at 0.02 and little
    gradient would reach the lower layers."""
    first = formats.gen_mlp_init([D_IN, WIDTHS[0]], seed=seed)[0]
    out = [first, formats.Layer("<sigmoid>", WIDTHS[0], WIDTHS[0])]
    for j, kind in enumerate(order):
        out += special(kind, WIDTHS[j], WIDTHS[j + 1], seed + 1 + j)
    return out + formats.gen_mlp_init([WIDTHS[3], N_CLS], seed=seed + 4)


def index_of(order, kind):
    """the component index of the `kind` layer in layers(order)"""
    return 2 + 2 * order.index(kind)


def net_text(L, precision=9):
    buf = io.StringIO()
    formats.write_nnet(L, buf, precision=precision)
    return buf.getvalue()


def consts(c, rows=ROWS[0]):
    """lr, momentum, weight cost and L1 of a (momentum, weight cost, GradDivFrm) combination, scaled as
    tests/dp_layers_cases.py's: without GradDivFrm the gradient is a sum over the rows, so the rate shrinks with the
    (first bunch's) rows; l1 puts the soft threshold lr*l1*(gdf ? 1 : rows) at 0.01 for a bunch of `rows` rows.
    The rate is ten times that file's: four sigmoids lie between the objective and the first layer, and its
    parameters must still move by many times the comparison's tolerance (test_stack_cases_cpu.py asserts it)."""
    mmt, wc, gdf = c
    lr = LR if gdf else LR / rows
    return dict(lr=lr, mmt=mmt, wc=wc, l1=L1_THRESHOLD / (lr * (1 if gdf else rows)), gdf=gdf)


def configure(net, c, factors=None):
    net.set_learn_rate(c["lr"], factors)
    net.set_momentum(c["mmt"])
    net.set_weightcost(c["wc"])
    net.set_l1(c["l1"])
    net.set_grad_div_frm(c["gdf"])


def bunches(rows=ROWS, seed=DATA_SEED, d=D_IN):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((r, d)).astype(np.float32), rng.integers(0, N_CLS, r).astype(np.int32)) for r in rows]


def parse_factors(factors):
    return None if factors is None else [float(f) for f in factors.replace(":", ",").split(",")]


# ---- the block array below the stopper: <blockarray> (tests/golden/blockarray_fwd.npz), <sparselinearity> 17 -> 12,
# sigmoid, <biasedlinearity> 12 -> 9, softmax.  The block array is an updatable component without an update: its
# factor 0 makes the sparse layer the stopper.
BLOCKARRAY_FACTORS = "0,1,1"
BLOCKARRAY_ROWS = ((0, 33), (5, 24))   # the fixture's rows each step trains on: all 33, then 19 from the middle
BLOCKARRAY_CONSTS = CONSTS[1]


def blockarray_upper(seed=INIT_SEED + 10):
    return formats.gen_sparse_init(17, 12, seed=seed, density=DENSITY, negbias=False) + \
        formats.gen_mlp_init([12, N_CLS], seed=seed + 1)


def blockarray_labels(seed=DATA_SEED + 10):
    return np.random.default_rng(seed).integers(0, N_CLS, 33).astype(np.int32)


# ---- what a test reads back from a network
def state(net):
    """every parameter of the network (and every sparse layer's mask, accu and frame count) as a dict of arrays keyed
    by the component index"""
    out = {}
    for i, (tag, _, _) in enumerate(net.components()):
        if tag == "<biasedlinearity>":
            out[f"{i}.W"], out[f"{i}.b"] = net.get_params(i)
        elif tag == "<sharedlinearity>":
            out[f"{i}.W"], out[f"{i}.b"], _ = net.shared_params(i)
        elif tag == "<discretelinearity>":
            Ws, out[f"{i}.b"] = net.discrete_params(i)
            for j, W in enumerate(Ws):
                out[f"{i}.W_{j}"] = W
        elif tag == "<sparselinearity>":
            W, b, mask, accu, nframes = net.sparse_params(i)
            out.update({f"{i}.W": W, f"{i}.b": b, f"{i}.mask": mask, f"{i}.accu": accu,
                        f"{i}.nframes": np.array([nframes], np.int64)})
    return out


def is_exact(key):
    """state entries compared bit for bit"""
    return key.endswith(".mask") or key.endswith(".nframes")


# ---- float64 restatement
def _stripes(M, widths):
    o = np.concatenate([[0], np.cumsum(widths)])
    return [M[:, o[i]:o[i + 1]] for i in range(len(widths))]


class Oracle:
    """CuNetwork::Propagate and CuNetwork::Backpropagate over a list of formats.Layer, in `dtype` (float64: the
    reference; float32: the headroom check).  The objective's sum is kept in float64 either way."""

    def __init__(self, L, dtype=np.float64):
        self.dt = dtype
        self.C = []
        for l in L:
            c = dict(tag=l.tag)
            if l.tag in UPDATABLE:
                c["b"] = l.b.astype(dtype)
                c["cb"] = np.zeros_like(c["b"])
                if l.tag == "<discretelinearity>":
                    c["Ws"] = [W.astype(dtype) for W in l.extra["Ws"]]
                    c["cw"] = [np.zeros_like(W) for W in c["Ws"]]
                else:
                    c["W"] = l.W.astype(dtype)
                    c["cw"] = np.zeros_like(c["W"])
                if l.tag == "<sharedlinearity>":
                    c["n"] = int(l.extra["n_inst"])
                if l.tag == "<sparselinearity>":
                    mask = l.extra.get("mask")
                    c["mask"] = np.ones(l.W.shape, np.float32) if mask is None else mask.astype(np.float32)
                    c["accu"] = np.zeros_like(c["W"])
                    c["nframes"] = 0
            elif l.tag not in ("<sigmoid>", "<softmax>"):
                raise ValueError(l.tag)
            self.C.append(c)
        self.xent, self.frames = 0.0, 0

    # -- forward
    def _propagate(self, c, a):
        tag = c["tag"]
        if tag in ("<biasedlinearity>", "<sparselinearity>"):
            return a @ c["W"] + c["b"]
        if tag == "<sharedlinearity>":
            wi = c["W"].shape[0]
            return np.concatenate([a[:, i * wi:(i + 1) * wi] @ c["W"] + c["b"] for i in range(c["n"])], axis=1)
        if tag == "<discretelinearity>":
            xs = _stripes(a, [W.shape[0] for W in c["Ws"]])
            return np.concatenate([x @ W for x, W in zip(xs, c["Ws"])], axis=1) + c["b"]
        if tag == "<sigmoid>":
            return 1.0 / (1.0 + np.exp(-a))
        e = np.exp(a - a.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    def forward(self, X, first=0, act=None):
        """the input and every component's output; first, act: start at component `first` from its input `act`"""
        acts = [np.asarray(X, self.dt) if act is None else act]
        for c in self.C[first:]:
            acts.append(self._propagate(c, acts[-1]))
        return acts

    def row_losses(self, Y, lab):
        return -np.log(Y[np.arange(len(lab)), lab]).astype(np.float64)

    # -- backward: the error a component hands down, through the weights it holds at the time of the call
    def _backpropagate(self, c, e, y):
        tag = c["tag"]
        if tag in ("<biasedlinearity>", "<sparselinearity>"):
            return e @ c["W"].T
        if tag == "<sharedlinearity>":
            wo = c["W"].shape[1]
            return np.concatenate([e[:, i * wo:(i + 1) * wo] @ c["W"].T for i in range(c["n"])], axis=1)
        if tag == "<discretelinearity>":
            es = _stripes(e, [W.shape[1] for W in c["Ws"]])
            return np.concatenate([x @ W.T for x, W in zip(es, c["Ws"])], axis=1)
        if tag == "<sigmoid>":
            return e * y * (1.0 - y)
        return e   # <softmax>: the objective's error is already the one of its input (cuActivation.cc:37-40)

    def _update(self, c, x, e, lr, k):
        T = self.dt
        mmt, wc, l1, gdf = T(k["mmt"]), k["wc"], k["l1"], k["gdf"]
        rows = x.shape[0]
        ndiv = (rows if gdf else 1.0) / (1.0 - k["mmt"])
        frm = 1.0 if gdf else float(rows)
        tag = c["tag"]
        if tag == "<biasedlinearity>":
            scale = T(-lr / ndiv)
            c["cw"], c["cb"] = x.T @ e + mmt * c["cw"], e.sum(axis=0) + mmt * c["cb"]
            c["W"] = c["W"] + scale * c["cw"]
            c["W"] = c["W"] + T(-lr * wc * frm) * c["W"]
            c["b"] = c["b"] + scale * c["cb"]
        elif tag == "<sharedlinearity>":
            n, (wi, wo) = c["n"], c["W"].shape
            scale = T(-lr / (ndiv * n))          # the gradient is a sum over the instances
            g = sum(x[:, i * wi:(i + 1) * wi].T @ e[:, i * wo:(i + 1) * wo] for i in range(n))
            gb = sum(e[:, i * wo:(i + 1) * wo].sum(axis=0) for i in range(n))
            c["cw"], c["cb"] = g + mmt * c["cw"], gb + mmt * c["cb"]
            c["W"] = c["W"] + scale * c["cw"]
            c["W"] = c["W"] + T(-lr * wc) * c["W"]   # no rows factor
            c["b"] = c["b"] + scale * c["cb"]
        elif tag == "<discretelinearity>":
            scale = T(-lr / ndiv)
            xs = _stripes(x, [W.shape[0] for W in c["Ws"]])
            es = _stripes(e, [W.shape[1] for W in c["Ws"]])
            for j in range(len(c["Ws"])):
                c["cw"][j] = xs[j].T @ es[j] + mmt * c["cw"][j]
                c["Ws"][j] = c["Ws"][j] + scale * c["cw"][j]
                c["Ws"][j] = c["Ws"][j] + T(-lr * wc) * c["Ws"][j]   # no rows factor
            c["cb"] = e.sum(axis=0) + mmt * c["cb"]
            c["b"] = c["b"] + scale * c["cb"]
        else:
            scale = T(-lr / ndiv)
            c["cw"], c["cb"] = x.T @ e + mmt * c["cw"], e.sum(axis=0) + mmt * c["cb"]
            w = c["W"] + scale * c["cw"]
            c["accu"] = c["accu"] + c["cw"]
            w = np.where(c["mask"] != 0, w, T(0))
            if l1 > 0:
                t = T(lr * l1 * frm)
                w = np.where(np.abs(w) < t, T(0), np.where(w > 0, w - t, w + t))
            if wc > 0:
                w = w + T(-lr * wc * frm) * w
            c["W"] = w
            c["b"] = c["b"] + scale * c["cb"]
            c["nframes"] += rows

    def learn_rates(self, lr, factors):
        """per component the learn rate (None: not updatable) and the stopper's index (CuNetwork::SetLearnRate)"""
        f = list(factors) if factors is not None else None
        rates, stopper = [], None
        for i, c in enumerate(self.C):
            if c["tag"] not in UPDATABLE:
                rates.append(None)
                continue
            rates.append(lr * (f.pop(0) if f is not None else 1.0))
            if stopper is None and rates[-1] > 0:
                stopper = i
        assert not f, "too many learn-rate factors"
        return rates, stopper

    def _backward(self, acts, err, k, rates, stopper):
        for i in range(len(self.C) - 1, -1, -1):
            c, e_in = self.C[i], err
            if i != stopper:
                err = self._backpropagate(c, e_in, acts[i + 1])     # pre-update weights, beta 0
            if rates[i] is not None and rates[i] > 0:
                self._update(c, acts[i], e_in, rates[i], k)
            if i == stopper:
                break

    def step(self, X, lab, k, factors=None, train=True):
        """one CuNetwork::TrainBunch; returns the input and every component's output"""
        acts = self.forward(X)
        Y, rows = acts[-1], len(lab)
        self.xent += float(self.row_losses(Y, lab).sum())
        self.frames += rows
        if train:
            err = Y.copy()
            err[np.arange(rows), lab] -= 1
            rates, stopper = self.learn_rates(k["lr"], factors)
            self._backward(acts, err, k, rates, stopper)
        return acts

    def update_mask(self, i):
        """CuSparseLinearity::UpdateMask (cuSparseLinearity.cc:66-97) of component i with the default thresholds:
        active weights below SPARSIFY are cut and zeroed, nothing wakes (unsparsify 1e20).  Returns `near`, the
        elements whose |W| lies within the float32 headroom -- the comparison's tolerance -- of the threshold: there
        fp32 and float64 may decide apart."""
        c = self.C[i]
        active = c["mask"] != 0
        near = active & (np.abs(np.abs(c["W"]) - SPARSIFY) <= ATOL + RTOL * SPARSIFY)
        cut = active & (np.abs(c["W"]) < SPARSIFY)
        c["mask"] = np.where(cut, 0.0, c["mask"]).astype(np.float32)
        c["W"] = np.where(cut, self.dt(0), c["W"])
        return near

    def state(self):
        out = {}
        for i, c in enumerate(self.C):
            if c["tag"] not in UPDATABLE:
                continue
            if "Ws" in c:
                for j, W in enumerate(c["Ws"]):
                    out[f"{i}.W_{j}"] = W
            else:
                out[f"{i}.W"] = c["W"]
            out[f"{i}.b"] = c["b"]
            if "mask" in c:
                out.update({f"{i}.mask": c["mask"], f"{i}.accu": c["accu"],
                            f"{i}.nframes": np.array([c["nframes"]], np.int64)})
        return out


def trajectory(L, k, data, factors=None, train=True, dtype=np.float64, mask_update=None):
    """the oracle over `data`: per step (outputs of every component, state after the step), and the oracle.
    mask_update = (step, component): UpdateMask of that component before that step; its `near` is ref.near"""
    ref = Oracle(L, dtype)
    ref.near = None
    f = parse_factors(factors) if isinstance(factors, str) else factors
    steps = []
    for s, (X, lab) in enumerate(data):
        if mask_update is not None and mask_update[0] == s:
            ref.near = ref.update_mask(mask_update[1])
        acts = ref.step(X, lab, k, f, train)
        steps.append((acts[1:], {key: np.array(v, copy=True) for key, v in ref.state().items()}))
    return steps, ref
