"""The float64 restatement of <blocksoftmax> and of the nets its fixtures train, shared by
tests/golden/make_blocksoftmax.py (which pins the reference's CPU output to it before saving),
tests/test_blocksoftmax_formats.py (CPU) and tests/test_gpu_blocksoftmax.py.

Semantics (the reference's BlockSoftmax, TNetLib Activation.cc:55-133, under CrossEntropy::Evaluate, ObjFun.cc:76-160):
  forward    every block of columns [off_j, off_j + d_j) is a softmax on its own maximum and sum
  objective  E = Y - T over the whole row; xent = -log y[label]; `correct` compares the argmax over the WHOLE row of
             Y with the target's column (column 0 for an all-zero target row)
  backward   per row and block the sum of E: in (-0.1, 0.1) the block held the target and its error passes; in
             (0.9, 1.1) it is inactive and its error is zero; anything else is the reference's "Invalid sum" error
             (here: zeroed and counted)
A label of -1 (or >= N) is an unlabeled row: every block sums to 1 and the whole error is discarded.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# pin tolerances of the fixtures (tests/golden/make_shared.py's)
RTOL, ATOL_Y, ATOL_P, XENT_RTOL = 2e-4, 2e-6, 1e-6, 1e-5
# the two largest whole-row posteriors differ by more than this (relative): 100 x the kernels' Y tolerance, so the
# integer `correct` can be compared exactly
MARGIN = 2e-3
FLT_MIN = float(np.finfo(np.float32).tiny)


def offsets(dims):
    return np.concatenate([[0], np.cumsum(np.asarray(dims, np.int64))]).astype(np.int32)


def block_softmax(Z, dims):
    Z = np.asarray(Z, np.float64)
    Y = np.empty_like(Z)
    off = offsets(dims)
    for lo, hi in zip(off[:-1], off[1:]):
        e = np.exp(Z[:, lo:hi] - Z[:, lo:hi].max(axis=1, keepdims=True))
        Y[:, lo:hi] = e / e.sum(axis=1, keepdims=True)
    return Y


def clean_labels(lab, n):
    """class ids with every id outside [0, n) turned into -1 (an unlabeled row)"""
    lab = np.asarray(lab, np.int64).copy()
    lab[(lab < 0) | (lab >= n)] = -1
    return lab


def sum_rule(E, dims):
    """BlockSoftmax::BackpropagateFnc on an error matrix: (masked error, number of invalid (row, block) sums)"""
    E = np.asarray(E, np.float64)
    out = np.zeros_like(E)
    off = offsets(dims)
    invalid = 0
    for lo, hi in zip(off[:-1], off[1:]):
        s = E[:, lo:hi].sum(axis=1)
        keep = (s > -0.1) & (s < 0.1)
        invalid += int((~keep & ~((s > 0.9) & (s < 1.1))).sum())
        out[keep, lo:hi] = E[keep, lo:hi]
    return out, invalid


def objective(Y, lab, dims):
    """(E = Y - T, the masked error, xent sum, correct count) of CrossEntropy::Evaluate + the backward pass"""
    Y = np.asarray(Y, np.float64)
    lab = clean_labels(lab, Y.shape[1])
    rows = np.arange(len(lab))
    has = lab >= 0
    T = np.zeros_like(Y)
    T[rows[has], lab[has]] = 1.0
    E = Y - T
    xent = float(-np.log(np.maximum(Y[rows[has], lab[has]], FLT_MIN)).sum())
    correct = int((Y.argmax(axis=1) == np.where(has, lab, 0)).sum())
    masked, invalid = sum_rule(E, dims)
    assert invalid == 0
    return E, masked, xent, correct


def margin_ok(Y):
    """True where the two largest posteriors of a row differ by more than MARGIN relative"""
    top = np.sort(np.asarray(Y, np.float64), axis=1)[:, -2:]
    return top[:, 1] - top[:, 0] > MARGIN * top[:, 1] if Y.shape[1] > 1 else np.ones(len(Y), bool)


# ------------------------------------------------------------------------------------- nets
def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


class Net:
    """float64 twin of a net of <biasedlinearity>, <sharedlinearity>, <sigmoid> layers under a <blocksoftmax>."""

    def __init__(self, layers):
        self.C = []
        for L in layers:
            c = {"tag": L.tag}
            if L.W is not None:
                c["W"], c["b"] = np.array(L.W, np.float64), np.array(L.b, np.float64)
                c["cw"], c["cb"] = np.zeros_like(c["W"]), np.zeros_like(c["b"])
            if L.tag == "<sharedlinearity>":
                c["n"] = int(L.extra["n_inst"])
            if L.tag == "<blocksoftmax>":
                c["dims"] = [int(d) for d in L.extra["dims"]]
            self.C.append(c)
        assert self.C[-1]["tag"] == "<blocksoftmax>"
        self.dims = self.C[-1]["dims"]

    def updatable(self):
        return [c for c in self.C if "W" in c]

    def forward(self, X):
        acts = [np.asarray(X, np.float64)]
        for c in self.C:
            a, tag = acts[-1], c["tag"]
            if tag == "<biasedlinearity>":
                a = a @ c["W"] + c["b"]
            elif tag == "<sharedlinearity>":
                wi = c["W"].shape[0]
                a = np.concatenate([a[:, i * wi:(i + 1) * wi] @ c["W"] + c["b"] for i in range(c["n"])], axis=1)
            elif tag == "<sigmoid>":
                a = sigmoid(a)
            elif tag == "<blocksoftmax>":
                a = block_softmax(a, c["dims"])
            else:
                raise ValueError(tag)
            acts.append(a)
        return acts

    def xent(self, X, lab):
        return objective(self.forward(X)[-1], lab, self.dims)[2]

    def step(self, X, lab, lr, mmt=0.0, wc=0.0, gdf=False, factors=None, train=True):
        """One SGD step with the library's constants (cuBiasedLinearity.cc:46-64, cuSharedLinearity.cc:65-94; with
        mmt = wc = 0 and gdf off they are the CPU twins': W -= lr X^T E, the shared layer's over its N instances
        W -= lr/N sum_i X_i^T E_i).  factors: one learn-rate factor per updatable layer; backpropagation stops at the
        first layer with a positive rate.  Returns (Y, E = Y - T, xent sum, correct)."""
        acts = self.forward(X)
        Y = acts[-1]
        E, err, xent, correct = objective(Y, lab, self.dims)
        if not train:
            return Y, E, xent, correct
        upd = self.updatable()
        rates = {id(c): lr * (1.0 if factors is None else factors[j]) for j, c in enumerate(upd)}
        stopper = next((c for c in upd if rates[id(c)] > 0), None)
        rows = len(X)
        ndiv = (rows if gdf else 1.0) / (1.0 - mmt)
        frm = 1.0 if gdf else float(rows)
        new = []
        for k in range(len(self.C) - 1, -1, -1):
            c, x, y, tag = self.C[k], acts[k], acts[k + 1], self.C[k]["tag"]
            e = err
            if c is not stopper:
                if tag == "<sigmoid>":
                    err = e * y * (1.0 - y)
                elif tag == "<biasedlinearity>":
                    err = e @ c["W"].T
                elif tag == "<sharedlinearity>":
                    wo = c["W"].shape[1]
                    err = np.concatenate([e[:, i * wo:(i + 1) * wo] @ c["W"].T for i in range(c["n"])], axis=1)
                # <blocksoftmax>: `err` is already the masked error
            if "W" in c and rates[id(c)] > 0:
                r = rates[id(c)]
                if tag == "<biasedlinearity>":
                    g, gb, scale, l2 = x.T @ e, e.sum(axis=0), -r / ndiv, -r * wc * frm
                else:
                    n, (wi, wo) = c["n"], c["W"].shape
                    g = sum(x[:, i * wi:(i + 1) * wi].T @ e[:, i * wo:(i + 1) * wo] for i in range(n))
                    gb = sum(e[:, i * wo:(i + 1) * wo].sum(axis=0) for i in range(n))
                    scale, l2 = -r / (ndiv * n), -r * wc
                new.append((c, g + mmt * c["cw"], gb + mmt * c["cb"], scale, l2))
            if c is stopper:
                break
        for c, cw, cb, scale, l2 in new:
            c["cw"], c["cb"] = cw, cb
            W = c["W"] + scale * cw
            c["W"] = W + l2 * W
            c["b"] = c["b"] + scale * cb
        return Y, E, xent, correct

    def params(self, prefix=""):
        out = {}
        for k, c in enumerate(self.updatable()):
            out[f"{prefix}W{k}"] = c["W"]
            out[f"{prefix}b{k}"] = c["b"]
        return out


# ------------------------------------------------------------------------------------- fixtures
FIXTURES = ("blocksoftmax_steps_mlp.npz", "blocksoftmax_steps_shared.npz")
MLP_DIMS, SHARED_DIMS = (3, 5, 2), (1, 6, 4)


def fixture_labels(dims, n, seed):
    """n class ids that cover every block, every seventh one -1"""
    rng = np.random.default_rng(seed)
    N = int(sum(dims))
    lab = rng.integers(0, N, size=n).astype(np.int32)
    lab[:N] = rng.permutation(N)     # every column, so every block, is some row's target
    lab[6::7] = -1
    off = offsets(dims)
    assert all(((lab >= lo) & (lab < hi)).any() for lo, hi in zip(off[:-1], off[1:]))
    return lab


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as g:
        return {k: g[k] for k in g.files}


def replay_fixture(g, layers):
    """Run the restatement over a fixture's bunches: yields (s, X_s, lab_s, Y, E, net after the step)"""
    net = Net(layers)
    bunch = int(g["bunch"])
    for s in range(len(g["X"]) // bunch):
        X, lab = g["X"][s * bunch:(s + 1) * bunch], g["labels"][s * bunch:(s + 1) * bunch]
        Y, E, xent, correct = net.step(X, lab, float(g["lr"]))
        yield s, X, lab, Y, E, xent, correct, net
