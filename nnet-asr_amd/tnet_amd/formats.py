"""Host-side data formats of the TNet training path (pure Python / numpy, no device code).

* ``.nnet`` text weight files -- the boundary format read/written by
  ``CuNetwork::ReadNetwork/WriteNetwork`` (src/CuTNetLib/cuNetwork.cc:47-73, factory/dumper
  :211-387): ``<tag> nOut nIn`` lines, ``m R C`` + R rows holding W^T, ``v N`` + N floats
  (src/KaldiLib/Matrix.tcc:521-600, Vector.tcc:525-571).
* HTK feature files (12-byte big-endian header, big-endian f32 payload;
  src/KaldiLib/Features.h:113-123) and HTK MLF label files
  (src/KaldiLib/Labels.cc:44-187: ``beg end state`` in 100 ns units, frame interval
  ``[(beg+P/2)/P, (end+P/2)/P)``).
* ``gen_mlp_init`` -- a seeded Python-3 restatement of tools/init/gen_mlp_init.py:36-68
  (``--gauss --negbias``: W ~ 0.1*N(0,1), hidden bias U[-4.1,-3.9], output bias 0).
* deterministic synthetic corpora (features ~ N(0,1), teacher-MLP or uniform labels) used by the
  tests and by bench.py.

The C++ product library has its own reader/writer for the same format (CuNetwork::ReadNetwork /
WriteNetwork and each component's ReadFromStream / WriteToStream, nnet-asr_amd/csrc/host/); this
module exists so tests and the bench can build inputs without touching the device.
"""
from __future__ import annotations

import io
import os
import struct
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

# --------------------------------------------------------------------------------------
# .nnet text format
# --------------------------------------------------------------------------------------


@dataclass
class Layer:
    tag: str                      # "<biasedlinearity>", "<sigmoid>", "<softmax>", "<rbm>", ...
    n_out: int
    n_in: int
    W: Optional[np.ndarray] = None   # stored as in memory: [n_in x n_out] (file holds W^T)
    b: Optional[np.ndarray] = None   # [n_out]
    extra: dict = field(default_factory=dict)


def _fmt(x: float, prec: int) -> str:
    return format(float(x), f".{prec}g")


def write_nnet(layers: Sequence[Layer], path_or_buf, precision: int = 6) -> None:
    """Write layers in the reference text format (default ostream precision = 6 digits)."""
    out = io.StringIO()
    _write_layers(out, layers, precision)
    text = out.getvalue()
    if hasattr(path_or_buf, "write"):
        path_or_buf.write(text)
    else:
        with open(path_or_buf, "w") as f:
            f.write(text)


def _write_layers(out, layers: Sequence[Layer], precision: int) -> None:
    for L in layers:
        out.write(f"{L.tag} {L.n_out} {L.n_in}\n")
        if L.tag in ("<biasedlinearity>", "<rbm>", "<recurrent>", "<sharedlinearity>"):
            if L.tag == "<rbm>":
                out.write(f"{L.extra.get('vis_type', 'bern')} {L.extra.get('hid_type', 'bern')}\n")
            if L.tag == "<sharedlinearity>":     # cuSharedLinearity.cc:160-176: the instance count first
                out.write(f"{int(L.extra['n_inst'])}\n")
            Wt = np.asarray(L.W, dtype=np.float32).T   # file holds [n_out x n_in(+n_out)]
            out.write(f"m {Wt.shape[0]} {Wt.shape[1]}\n")
            for row in Wt:
                out.write(" ".join(_fmt(v, precision) for v in row))
                out.write(" \n")
            if L.tag == "<rbm>":
                vb = np.asarray(L.extra["vis_bias"], dtype=np.float32)
                out.write(f"v {vb.shape[0]}  " + " ".join(_fmt(v, precision) for v in vb) + " ")
                out.write("\n")
            b = np.asarray(L.b, dtype=np.float32)
            out.write(f"v {b.shape[0]}  " + " ".join(_fmt(v, precision) for v in b) + " ")
            out.write("\n\n")
        elif L.tag == "<discretelinearity>":     # cuDiscreteLinearity.cc:139-156: count, transposed blocks, bias
            Ws = L.extra["Ws"]
            out.write(f"{len(Ws)}\n")
            for W in Ws:
                Wt = np.asarray(W, dtype=np.float32).T
                out.write(f"m {Wt.shape[0]} {Wt.shape[1]}\n")
                for row in Wt:
                    out.write(" ".join(_fmt(v, precision) for v in row))
                    out.write(" \n")
            b = np.asarray(L.b, dtype=np.float32)
            out.write(f"v {b.shape[0]}  " + " ".join(_fmt(v, precision) for v in b) + " ")
            out.write("\n\n")
        elif L.tag == "<sparselinearity>":       # cuSparseLinearity.cc:163-186: W^T, bias, then mask^T and accu^T
            mats = [L.W] + [L.extra[k] for k in ("mask", "accu") if L.extra.get(k) is not None]
            if "accu" in L.extra and L.extra.get("mask") is None:
                raise ValueError("<sparselinearity>: an accu matrix needs a mask matrix before it")
            for k, M in enumerate(mats):
                Mt = np.asarray(M, dtype=np.float32).T
                out.write(f"m {Mt.shape[0]} {Mt.shape[1]}\n")
                for row in Mt:
                    out.write(" ".join(_fmt(v, precision) for v in row))
                    out.write(" \n")
                if k == 0:
                    b = np.asarray(L.b, dtype=np.float32)
                    out.write(f"v {b.shape[0]}  " + " ".join(_fmt(v, precision) for v in b) + " ")
                    out.write("\n\n")
        elif L.tag == "<blockarray>":            # cuBlockArray.cc:125-135
            blocks = L.extra["blocks"]
            out.write(f" {len(blocks)} ")
            for k, block in enumerate(blocks):
                out.write(f"<block> {k + 1}\n")
                _write_layers(out, block, precision)
                out.write("<endblock>\n")
        else:
            _write_frontend(out, L, precision)


def _write_frontend(out, L: Layer, precision: int) -> None:
    """Payload of the front-end components (cuCRBEDctFeat.h:16-304 ReadFromStream/WriteToStream)."""
    def ivec(v):
        v = np.asarray(v, dtype=np.int64)
        out.write(f"v {v.shape[0]}  " + " ".join(str(int(x)) for x in v) + " \n")

    def fvec(v):
        v = np.asarray(v, dtype=np.float32)
        out.write(f"v {v.shape[0]}  " + " ".join(_fmt(x, precision) for x in v) + " \n")

    if L.tag == "<expand>":
        ivec(L.extra["offsets"])
    elif L.tag == "<copy>":
        ivec(np.asarray(L.extra["indices"]) + 1)          # the file is 1-based
    elif L.tag == "<transpose>":
        out.write(f" {int(L.extra['context'])}\n")
    elif L.tag == "<blocklinearity>":
        Bt = np.asarray(L.W, dtype=np.float32).T           # file holds the [bo x bi] transpose
        out.write(f"m {Bt.shape[0]} {Bt.shape[1]}\n")
        for row in Bt:
            out.write(" ".join(_fmt(v, precision) for v in row) + " \n")
    elif L.tag == "<bias>":
        fvec(L.b)
    elif L.tag == "<window>":
        fvec(L.extra["window"])
    elif L.tag == "<blocksoftmax>":                        # Activation.cc:73-75: the block widths
        ivec(_check_blocksoftmax_dims(L.extra["dims"], L.n_out))
    # <sigmoid>, <softmax>, <log>: no payload


def _check_blocksoftmax_dims(dims, n_out: int) -> np.ndarray:
    """The block widths of a <blocksoftmax>, refused as BlockSoftmax::ReadFromStream refuses them
    (Activation.cc:55-71) -- and when a width is not positive."""
    dims = np.asarray(dims, dtype=np.int64).reshape(-1)
    if dims.size == 0 or (dims <= 0).any():
        raise ValueError(f"<blocksoftmax>: non-positive or missing block dimension in {dims.tolist()}")
    if int(dims.sum()) != int(n_out):
        raise ValueError("Non-matching dimension of sum of softmaxes,"
                         f" the sum:{int(dims.sum())} GetNOutputs:{int(n_out)}")
    return dims


def _tokens(text: str):
    for tok in text.split():
        yield tok


def read_nnet(path_or_text: str) -> List[Layer]:
    """Parse a .nnet text file (tags are case-insensitive; ``<endblock>`` terminates)."""
    if os.path.exists(path_or_text):
        with open(path_or_text) as f:
            text = f.read()
    else:
        text = path_or_text
    toks = text.split()
    i = 0

    def read_matrix():
        nonlocal i
        assert toks[i] == "m", toks[i]
        r, c = int(toks[i + 1]), int(toks[i + 2])
        i += 3
        m = np.array(toks[i:i + r * c], dtype=np.float32).reshape(r, c)
        i += r * c
        return m

    def read_vector():
        nonlocal i
        assert toks[i] == "v", toks[i]
        n = int(toks[i + 1])
        i += 2
        v = np.array(toks[i:i + n], dtype=np.float32)
        i += n
        return v

    def read_layers() -> List[Layer]:
        nonlocal i
        layers: List[Layer] = []
        while i < len(toks):
            tag = toks[i].lower()
            if tag == "<endblock>":
                i += 1
                break
            n_out, n_in = int(toks[i + 1]), int(toks[i + 2])
            i += 3
            L = Layer(tag, n_out, n_in)
            if tag == "<biasedlinearity>" or tag == "<recurrent>":
                L.W = np.ascontiguousarray(read_matrix().T)
                L.b = read_vector()
            elif tag == "<sharedlinearity>":
                # cuSharedLinearity.cc:99-157 and its three error conditions
                n = int(toks[i])
                i += 1
                if n < 1:
                    raise ValueError(f"Bad number of instances:{n}")
                if n_in % n or n_out % n:
                    raise ValueError("Number of Inputs/Outputs must be divisible by number of instances"
                                     f" Inputs:{n_in} Outputs{n_out} Intances:{n}")
                L.extra["n_inst"] = n
                L.W = np.ascontiguousarray(read_matrix().T)
                L.b = read_vector()
                if L.W.shape != (n_in // n, n_out // n) or L.b.shape != (n_out // n,):
                    raise ValueError("Wrong dimensionalities of matrix/vector in network file")
            elif tag == "<discretelinearity>":
                # cuDiscreteLinearity.cc:81-136 and its error conditions
                nb = int(toks[i])
                i += 1
                if nb < 1:
                    raise ValueError(f"Bad number of blocks:{nb}")
                Ws = []
                for _ in range(nb):
                    Wt = read_matrix()
                    if Wt.size == 0:
                        raise ValueError("Missing linearity matrix in network file")
                    Ws.append(np.ascontiguousarray(Wt.T))
                L.b = read_vector()
                if L.b.size == 0:
                    raise ValueError("Missing bias vector in network file")
                if (sum(W.shape[1] for W in Ws) != n_out or sum(W.shape[0] for W in Ws) != n_in
                        or L.b.shape[0] != n_out):
                    raise ValueError("Wrong dimensionalities of matrix/vector in network file")
                L.extra["Ws"] = Ws
            elif tag == "<sparselinearity>":
                # cuSparseLinearity.cc:100-160: W^T, bias, then an optional mask^T and an optional accu^T (which
                # the library reads and drops); a mask of another shape than W is an error here too
                if i >= len(toks) or toks[i] != "m":
                    raise ValueError("Missing linearity matrix in network file")
                L.W = np.ascontiguousarray(read_matrix().T)
                if i >= len(toks) or toks[i] != "v":
                    raise ValueError("Missing bias vector in network file")
                L.b = read_vector()
                if L.W.size == 0:
                    raise ValueError("Missing linearity matrix in network file")
                if L.b.size == 0:
                    raise ValueError("Missing bias vector in network file")
                if L.W.shape != (n_in, n_out) or L.b.shape != (n_out,):
                    raise ValueError("Wrong dimensionalities of matrix/vector in network file")
                if i < len(toks) and toks[i] == "m":
                    L.extra["mask"] = np.ascontiguousarray(read_matrix().T)
                    if L.extra["mask"].shape != L.W.shape:
                        raise ValueError("Wrong dimensionality of the sparsity mask in network file")
                    if i < len(toks) and toks[i] == "m":
                        L.extra["accu"] = np.ascontiguousarray(read_matrix().T)
                # (no mask matrix: no "mask" key, every weight is active)
            elif tag == "<blockarray>":
                # cuBlockArray.cc:57-122
                nb = int(toks[i])
                i += 1
                if nb < 1:
                    raise ValueError(f"Bad number of blocks:{nb}")
                blocks = []
                for k in range(nb):
                    if toks[i].lower() != "<block>":
                        raise ValueError("<block> keywotd expected")
                    if int(toks[i + 1]) != k + 1:
                        raise ValueError(f"Expected block number:{k + 1} read block number: {toks[i + 1]}")
                    i += 2
                    block = read_layers()
                    if not block:
                        raise ValueError("Cannot read empty network to a block")
                    blocks.append(block)
                if sum(b[0].n_in for b in blocks) != n_in:
                    raise ValueError("Non-matching number of INPUTS!")
                if sum(b[-1].n_out for b in blocks) != n_out:
                    raise ValueError("Non-matching number of OUTPUTS!")
                L.extra["blocks"] = blocks
            elif tag == "<rbm>":
                L.extra["vis_type"] = toks[i].lower()
                L.extra["hid_type"] = toks[i + 1].lower()
                i += 2
                L.W = np.ascontiguousarray(read_matrix().T)
                L.extra["vis_bias"] = read_vector()
                L.b = read_vector()
            elif tag == "<expand>":
                L.extra["offsets"] = read_vector().astype(np.int64)
            elif tag == "<copy>":
                L.extra["indices"] = read_vector().astype(np.int64) - 1
            elif tag == "<transpose>":
                L.extra["context"] = int(toks[i])
                i += 1
            elif tag == "<blocklinearity>":
                L.W = np.ascontiguousarray(read_matrix().T)
            elif tag == "<bias>":
                L.b = read_vector()
            elif tag == "<window>":
                L.extra["window"] = read_vector()
            elif tag == "<blocksoftmax>":
                if i >= len(toks) or toks[i] != "v":
                    raise ValueError("<blocksoftmax>: missing block dimensions")
                n = int(toks[i + 1])
                dims = [int(t) for t in toks[i + 2:i + 2 + n]]
                i += 2 + n
                L.extra["dims"] = [int(d) for d in _check_blocksoftmax_dims(dims, n_out)]
            layers.append(L)
        return layers

    return read_layers()


def gen_mlp_init(dims: Sequence[int], seed: int, gauss: bool = True, negbias: bool = True) -> List[Layer]:
    """Seeded restatement of tools/init/gen_mlp_init.py:36-68 (numpy RNG, not Python 2's)."""
    rng = np.random.default_rng(seed)
    layers: List[Layer] = []
    for li in range(len(dims) - 1):
        n_in, n_out = dims[li], dims[li + 1]
        if gauss:
            Wt = (0.1 * rng.standard_normal((n_out, n_in))).astype(np.float32)
        else:
            Wt = (rng.random((n_out, n_in)) / 5.0 - 0.1).astype(np.float32)
        last = li == len(dims) - 2
        if last or not negbias:
            b = np.zeros(n_out, np.float32)
        else:
            b = (rng.random(n_out) / 5.0 - 4.1).astype(np.float32)
        layers.append(Layer("<biasedlinearity>", n_out, n_in, np.ascontiguousarray(Wt.T), b))
        layers.append(Layer("<softmax>" if last else "<sigmoid>", n_out, n_out))
    return layers


def gen_rbm_init(n_vis: int, n_hid: int, seed: int, vis_type: str = "gauss", hid_type: str = "bern",
                 gauss: bool = True, negbias: bool = True) -> List[Layer]:
    """Seeded restatement of tools/init/gen_rbm_init.py (one <rbm> layer): W^T ~ 0.1 N(0,1)
    (--gauss) or U[-0.1, 0.1]; a Gaussian unit layer gets zero biases, a Bernoulli one
    U[-4.1, -3.9] with --negbias (else 0)."""
    rng = np.random.default_rng(seed)
    if gauss:
        Wt = (0.1 * rng.standard_normal((n_hid, n_vis))).astype(np.float32)
    else:
        Wt = (rng.random((n_hid, n_vis)) / 5.0 - 0.1).astype(np.float32)

    def bias(n, kind):
        if kind == "gauss" or not negbias:
            return np.zeros(n, np.float32)
        return (rng.random(n) / 5.0 - 4.1).astype(np.float32)

    vb = bias(n_vis, vis_type)
    hb = bias(n_hid, hid_type)
    return [Layer("<rbm>", n_hid, n_vis, np.ascontiguousarray(Wt.T), hb,
                  {"vis_type": vis_type, "hid_type": hid_type, "vis_bias": vb})]


def gen_shared_init(n_inst: int, n_in: int, n_out: int, seed: int, gauss: bool = True,
                    negbias: bool = True) -> List[Layer]:
    """One <sharedlinearity> of ``n_inst`` instances of an n_in -> n_out transform (the layer is
    n_inst*n_in -> n_inst*n_out) followed by its <sigmoid>, parameters drawn as gen_mlp_init draws a
    hidden layer's: W^T ~ 0.1 N(0,1) (--gauss) or U[-0.1, 0.1], bias U[-4.1, -3.9] (--negbias) or 0."""
    rng = np.random.default_rng(seed)
    if gauss:
        Wt = (0.1 * rng.standard_normal((n_out, n_in))).astype(np.float32)
    else:
        Wt = (rng.random((n_out, n_in)) / 5.0 - 0.1).astype(np.float32)
    b = (rng.random(n_out) / 5.0 - 4.1).astype(np.float32) if negbias else np.zeros(n_out, np.float32)
    return [Layer("<sharedlinearity>", n_inst * n_out, n_inst * n_in, np.ascontiguousarray(Wt.T), b,
                  {"n_inst": int(n_inst)}),
            Layer("<sigmoid>", n_inst * n_out, n_inst * n_out)]


def gen_discrete_init(dims_in: Sequence[int], dims_out: Sequence[int], seed: int, gauss: bool = True,
                      negbias: bool = True) -> List[Layer]:
    """One <discretelinearity> of len(dims_in) blocks, block k a dims_in[k] -> dims_out[k] transform (the layer is
    sum(dims_in) -> sum(dims_out); tools/init/gen_discretelinearity_init.py writes equal blocks, the file format
    allows ragged ones) followed by its <sigmoid>, parameters drawn as gen_mlp_init draws a hidden layer's: every
    W_k^T ~ 0.1 N(0,1) (--gauss) or U[-0.1, 0.1] in block order, then the bias U[-4.1, -3.9] (--negbias) or 0.
    Layer.W is None; the blocks are extra["Ws"]."""
    if len(dims_in) != len(dims_out) or not len(dims_in):
        raise ValueError("gen_discrete_init: one input and one output size per block")
    rng = np.random.default_rng(seed)
    Ws = []
    for n_in, n_out in zip(dims_in, dims_out):
        if gauss:
            Wt = (0.1 * rng.standard_normal((n_out, n_in))).astype(np.float32)
        else:
            Wt = (rng.random((n_out, n_in)) / 5.0 - 0.1).astype(np.float32)
        Ws.append(np.ascontiguousarray(Wt.T))
    n_out, n_in = int(sum(dims_out)), int(sum(dims_in))
    b = (rng.random(n_out) / 5.0 - 4.1).astype(np.float32) if negbias else np.zeros(n_out, np.float32)
    return [Layer("<discretelinearity>", n_out, n_in, None, b, {"Ws": Ws}),
            Layer("<sigmoid>", n_out, n_out)]


def gen_sparse_init(n_in: int, n_out: int, seed: int, density: float = 1.0, gauss: bool = True,
                    negbias: bool = True) -> List[Layer]:
    """One <sparselinearity> n_in -> n_out followed by its <sigmoid>, parameters drawn as gen_mlp_init draws a hidden
    layer's: W^T ~ 0.1 N(0,1) (--gauss) or U[-0.1, 0.1], bias U[-4.1, -3.9] (--negbias) or 0.  density < 1: a random
    0/1 mask (each weight active with probability `density`, drawn after W and the bias, so W and b do not depend
    on the density) in extra["mask"], W zeroed under it; density 1: no mask matrix (the file then has none and every
    weight is active)."""
    if not 0.0 <= density <= 1.0:
        raise ValueError("gen_sparse_init: density must lie in [0, 1]")
    rng = np.random.default_rng(seed)
    if gauss:
        Wt = (0.1 * rng.standard_normal((n_out, n_in))).astype(np.float32)
    else:
        Wt = (rng.random((n_out, n_in)) / 5.0 - 0.1).astype(np.float32)
    b = (rng.random(n_out) / 5.0 - 4.1).astype(np.float32) if negbias else np.zeros(n_out, np.float32)
    W = np.ascontiguousarray(Wt.T)
    extra = {}
    if density < 1.0:
        mask = (rng.random((n_in, n_out)) < density).astype(np.float32)
        W = W * mask
        extra["mask"] = mask
    return [Layer("<sparselinearity>", n_out, n_in, W, b, extra),
            Layer("<sigmoid>", n_out, n_out)]


def gen_blocksoftmax_top(n_in: int, dims: Sequence[int], seed: int, gauss: bool = True) -> List[Layer]:
    """The output layer of a multi-task net: one <biasedlinearity> n_in -> sum(dims) drawn as gen_mlp_init draws
    its output layer (W^T ~ 0.1 N(0,1) with --gauss, else U[-0.1, 0.1]; zero bias) followed by a <blocksoftmax> of
    len(dims) blocks, block j dims[j] columns wide (extra["dims"])."""
    n_out = int(sum(int(d) for d in dims))
    dims = [int(d) for d in _check_blocksoftmax_dims(dims, n_out)]
    rng = np.random.default_rng(seed)
    if gauss:
        Wt = (0.1 * rng.standard_normal((n_out, n_in))).astype(np.float32)
    else:
        Wt = (rng.random((n_out, n_in)) / 5.0 - 0.1).astype(np.float32)
    return [Layer("<biasedlinearity>", n_out, n_in, np.ascontiguousarray(Wt.T), np.zeros(n_out, np.float32)),
            Layer("<blocksoftmax>", n_out, n_out, extra={"dims": dims})]


def gen_recurrent_init(n_in: int, n_hid: int, n_out: int, seed: int, gauss: bool = True,
                       negbias: bool = False) -> List[Layer]:
    """Seeded restatement of tools/init/gen_recurrent_init.py (<recurrent> n_in -> n_hid, matrix
    [n_hid x (n_in + n_hid)] in the file) followed by a gen_mlp_init-style <biasedlinearity>
    n_hid -> n_out + <softmax> (the TRecurrentCu network of BASELINE config 5)."""
    rng = np.random.default_rng(seed)
    k = n_in + n_hid
    Wt = (0.1 * rng.standard_normal((n_hid, k)) if gauss else rng.random((n_hid, k)) / 5.0 - 0.1).astype(np.float32)
    b = ((rng.random(n_hid) / 5.0 - 4.1) if negbias else np.zeros(n_hid)).astype(np.float32)
    out = gen_mlp_init([n_hid, n_out], seed=seed + 1)
    return [Layer("<recurrent>", n_hid, n_in, np.ascontiguousarray(Wt.T), b)] + out


def gen_frontend_transform(dim: int = 23, context: int = 25, n_dct: int = 26, seed: int = 0,
                           normalise: bool = True) -> List[Layer]:
    """A --FEATURETRANSFORM network of the examples/01 "Hamm_dct_norm" structure, built from
    formulas: <expand> to 2*context+1 frames, <transpose> to band-major, a Hamming <window> per
    band, a per-band DCT-II <blocklinearity> (2*context+1 -> n_dct; row k = cos(pi k (j+1/2) / L)),
    then (normalise) a seeded <bias> / <window> pair standing in for the global mean/variance
    normalisation.  Output dim = dim * n_dct."""
    L = 2 * context + 1
    n_sp = dim * L
    n_out = dim * n_dct
    j = np.arange(L)
    hamming = (0.54 - 0.46 * np.cos(2.0 * np.pi * j / (L - 1))).astype(np.float32)
    dct = np.cos(np.pi * np.outer(np.arange(n_dct), j + 0.5) / L).astype(np.float32)   # [n_dct x L]
    layers = [Layer("<expand>", n_sp, dim, extra={"offsets": np.arange(-context, context + 1)}),
              Layer("<transpose>", n_sp, n_sp, extra={"context": L}),
              Layer("<window>", n_sp, n_sp, extra={"window": np.tile(hamming, dim)}),
              Layer("<blocklinearity>", n_out, n_sp, W=np.ascontiguousarray(dct.T))]
    if normalise:
        rng = np.random.default_rng(seed)
        layers.append(Layer("<bias>", n_out, n_out, b=(-rng.standard_normal(n_out)).astype(np.float32)))
        layers.append(Layer("<window>", n_out, n_out,
                            extra={"window": (0.05 + 0.3 * rng.random(n_out)).astype(np.float32)}))
    return layers


def extend_frames(x: np.ndarray, start: int, end: int) -> np.ndarray:
    """--STARTFRMEXT / --ENDFRMEXT: repeat the first / last frame (src/KaldiLib/Features.cc:776-850)."""
    x = np.asarray(x, dtype=np.float32)
    return np.concatenate([np.repeat(x[:1], start, 0), x, np.repeat(x[-1:], end, 0)], axis=0)


def round_trip_text(layers: Sequence[Layer], precision: int = 6) -> List[Layer]:
    """Weights exactly as a reader sees them after a text write at ``precision`` digits."""
    buf = io.StringIO()
    write_nnet(layers, buf, precision)
    return read_nnet(buf.getvalue())


# --------------------------------------------------------------------------------------
# HTK features / MLF labels
# --------------------------------------------------------------------------------------

HTK_USER = 9


def write_htk(path: str, feats: np.ndarray, samp_period: int = 100000, kind: int = HTK_USER) -> None:
    feats = np.asarray(feats, dtype=np.float32)
    n, d = feats.shape
    with open(path, "wb") as f:
        f.write(struct.pack(">iihh", n, samp_period, d * 4, kind))
        f.write(feats.astype(">f4").tobytes())


def read_htk(path: str) -> np.ndarray:
    with open(path, "rb") as f:
        n, period, size, kind = struct.unpack(">iihh", f.read(12))
        data = np.frombuffer(f.read(n * size), dtype=">f4").astype(np.float32)
    return data.reshape(n, size // 4)


def read_htk_header(path: str):
    """(frames, sample period [100 ns], bytes per frame, parameter kind)."""
    with open(path, "rb") as f:
        return struct.unpack(">iihh", f.read(12))


def read_state_map(path: str) -> dict:
    """LabelRepository::ReadOutputLabelMap (src/KaldiLib/Labels.cc:192-212): whitespace-separated
    state tags, id = position."""
    tags = open(path).read().split()
    if len(set(tags)) != len(tags):
        raise ValueError(f"{path}: duplicate state tag")
    return {t: i for i, t in enumerate(tags)}


def read_mlf(path: str) -> dict:
    """An HTK master label file -> {pattern: [(beg, end, tag), ...]} (times in 100 ns units)."""
    out, cur = {}, None
    with open(path) as f:
        for line in f:
            s = line.strip()
            if not s or s.startswith("#"):
                continue
            if s.startswith('"'):
                cur = out.setdefault(s.strip('"'), [])
            elif s == ".":
                cur = None
            elif cur is not None:
                beg, end, tag = s.split()[:3]
                cur.append((int(beg), int(end), tag))
    return out


def mlf_class_ids(segments, n_frames: int, samp_period: int, state_map: dict) -> np.ndarray:
    """LabelRepository::GenDesiredMatrix (src/KaldiLib/Labels.cc:42-186) as class ids: frame
    interval [(beg + P/2) / P, (end + P/2) / P), frames past the feature end dropped, a frame
    labelled twice or never is an error (the reference's row-sum check)."""
    lab = np.full(n_frames, -1, np.int32)
    half = samp_period // 2
    for beg, end, tag in segments:
        if tag not in state_map:
            raise ValueError(f"Unknown state tag: '{tag}'")
        b, e = (beg + half) // samp_period, (end + half) // samp_period
        for t in range(b, min(e, n_frames)):
            if lab[t] != -1:
                raise ValueError(f"Frame already assigned to other state, frame: {t}")
            lab[t] = state_map[tag]
    if (lab < 0).any():
        raise ValueError(f"Desired vector sum isn't 1.0, row: {int(np.argmax(lab < 0))}")
    return lab


def read_corpus(scp: str, mlf: str, states: str, label_dir: str = "*/", label_ext: str = "lab",
                base: Optional[str] = None) -> "Corpus":
    """The FeatureRepository + LabelRepository intake of TNet / TNetCu (-S scp -I mlf -L dir -X ext
    -m states): HTK features in scp order, per-frame class ids from the MLF.  Relative scp paths are
    taken from ``base`` (default: the scp's directory)."""
    base = base or os.path.dirname(os.path.abspath(scp))
    smap = read_state_map(states)
    mlfd = read_mlf(mlf)
    feats, labels = [], []
    for l in open(scp):
        p = l.strip()
        if not p:
            continue
        path = p if os.path.isabs(p) else os.path.join(base, p)
        n, period, _, _ = read_htk_header(path)
        x = read_htk(path)
        key = label_dir.rstrip("/") + "/" + os.path.splitext(os.path.basename(p))[0] + "." + label_ext
        if key not in mlfd:
            raise ValueError(f"Cannot open label MLF record: {key}")
        feats.append(x)
        labels.append(mlf_class_ids(mlfd[key], n, period, smap))
    return Corpus(feats, labels)


def write_mlf(path: str, utts: Sequence[str], labels: Sequence[np.ndarray], state_names: Sequence[str],
              samp_period: int = 100000) -> None:
    """One label segment per run of equal class ids; '*/<utt>.lab' patterns like examples/01."""
    with open(path, "w") as f:
        f.write("#!MLF!#\n")
        for u, lab in zip(utts, labels):
            f.write(f'"*/{u}.lab"\n')
            lab = np.asarray(lab)
            start = 0
            for t in range(1, len(lab) + 1):
                if t == len(lab) or lab[t] != lab[start]:
                    f.write(f"{start * samp_period} {t * samp_period} {state_names[lab[start]]}\n")
                    start = t
            f.write(".\n")


# --------------------------------------------------------------------------------------
# Synthetic corpora
# --------------------------------------------------------------------------------------


@dataclass
class Corpus:
    feats: List[np.ndarray]      # per utterance [T x D] float32
    labels: List[np.ndarray]     # per utterance [T] int32 class ids

    @property
    def frames(self) -> int:
        return int(sum(len(l) for l in self.labels))


def _teacher_labels(x: np.ndarray, teacher: List[np.ndarray], n_cls: int) -> np.ndarray:
    h = x
    for k, W in enumerate(teacher):
        h = h @ W
        if k < len(teacher) - 1:
            h = np.tanh(h)
    return np.argmax(h, axis=1).astype(np.int32)


def synth_corpus(n_utts: int, dim: int, n_cls: int, seed: int = 0, min_len: int = 200, max_len: int = 1500,
                 teacher: bool = True, teacher_hidden: int = 64) -> Corpus:
    """Deterministic synthetic stacked-feature corpus: N(0,1) features, teacher-MLP labels."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(min_len, max_len + 1, size=n_utts)
    trng = np.random.default_rng(seed + 1)
    T = [trng.standard_normal((dim, teacher_hidden)).astype(np.float32) / np.sqrt(dim),
         trng.standard_normal((teacher_hidden, n_cls)).astype(np.float32) / np.sqrt(teacher_hidden) * 4.0]
    feats, labels = [], []
    for n in lens:
        x = rng.standard_normal((int(n), dim)).astype(np.float32)
        if teacher:
            y = _teacher_labels(x, T, n_cls)
        else:
            y = rng.integers(0, n_cls, size=int(n)).astype(np.int32)
        feats.append(x)
        labels.append(y)
    return Corpus(feats, labels)


def write_corpus_htk(corpus: Corpus, outdir: str, n_cls: int) -> dict:
    """Write HTK features, scp, MLF and a state map so the reference TNet can train on it."""
    os.makedirs(os.path.join(outdir, "features"), exist_ok=True)
    names = [f"u{i:05d}" for i in range(len(corpus.feats))]
    scp = os.path.join(outdir, "train.scp")
    with open(scp, "w") as f:
        for n, x in zip(names, corpus.feats):
            p = os.path.join(outdir, "features", n + ".fea")
            write_htk(p, x)
            f.write(p + "\n")
    states = [f"s{k}" for k in range(n_cls)]
    with open(os.path.join(outdir, "states"), "w") as f:
        f.write("\n".join(states) + "\n")
    write_mlf(os.path.join(outdir, "train.mlf"), names, corpus.labels, states)
    return {"scp": scp, "mlf": os.path.join(outdir, "train.mlf"), "states": os.path.join(outdir, "states")}
