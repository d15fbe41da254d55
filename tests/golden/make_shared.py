#!/usr/bin/env python3
"""Regenerate the <sharedlinearity> / <blockarray> fixtures in tests/golden/ from the REFERENCE CPU TNet.

Runs only in the build container (needs /root/reference and oracle/_ref/ref_harness, oracle/_ref/TFeaCat built by
``make -C oracle ref``).  The fixtures are data only: inputs generated here (seeded) and the outputs the
reference's CPU twins (src/TNetLib/SharedLinearity.cc, BlockArray.cc) computed on them.

  shared_steps_first.npz  <sharedlinearity> 48 72 (3 x 24->16), <sigmoid>, <biasedlinearity> 10 48, <softmax>;
                          bunch 16, 4 SGD steps, lr 0.5, wc 0 through ``ref_harness step``.  The shared layer is
                          first, so the CPU Network::Backpropagate never back-propagates through it
                          (Nnet.cc:100-104) and the whole trajectory is pinned.
  shared_steps_stack.npz  shared 3 x (20->12), sigmoid, shared 3 x (12->6), sigmoid, <biasedlinearity> 10 18,
                          softmax; bunch 16, ONE step: the CPU twin's backward accumulates (beta 1,
                          SharedLinearity.cc:35) into a buffer cleared only at allocation, the CUDA code (and this
                          library) uses beta 0 -- they agree on the first step of a fresh process only.
  blockarray_fwd.npz      <blockarray> 17 28 of two blocks ({<biasedlinearity> 7 10, <sigmoid>} and
                          {<sharedlinearity> 10 18 (2 x 9->5), <sigmoid>}), inputs [33 x 28], the forward output
                          of oracle/_ref/TFeaCat, and the .nnet text it read.

Before saving, every stored output is recomputed by the float64 numpy restatement below and must agree within the
pin tolerance of tests/test_gpu_shared.py (rtol 2e-4; atol 2e-6 outputs, 1e-6 parameters).
Reproducibility: MKL_NUM_THREADS=1 MKL_CBWR=COMPATIBLE.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "nnet-asr_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
from golden_io import save_npz_parts  # noqa: E402
from tnet_amd import formats  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref")
ENV = dict(os.environ, MKL_NUM_THREADS="1", MKL_CBWR="COMPATIBLE", OMP_NUM_THREADS="1")
RTOL, ATOL_Y, ATOL_P = 2e-4, 2e-6, 1e-6


# ---------------------------------------------------------------------------- float64 restatement
def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def forward(layers, X):
    """Activations after every layer ([X, a_0, a_1, ...]) in float64."""
    acts = [np.asarray(X, np.float64)]
    for L in layers:
        a = acts[-1]
        if L.tag == "<biasedlinearity>":
            a = a @ L.W.astype(np.float64) + L.b.astype(np.float64)
        elif L.tag == "<sharedlinearity>":
            n = L.extra["n_inst"]
            W, b = L.W.astype(np.float64), L.b.astype(np.float64)
            a = np.concatenate([a[:, i * W.shape[0]:(i + 1) * W.shape[0]] @ W + b for i in range(n)], axis=1)
        elif L.tag == "<sigmoid>":
            a = sigmoid(a)
        elif L.tag == "<softmax>":
            e = np.exp(a - a.max(axis=1, keepdims=True))
            a = e / e.sum(axis=1, keepdims=True)
        elif L.tag == "<blockarray>":
            outs, o = [], 0
            for block in L.extra["blocks"]:
                ni = block[0].n_in
                outs.append(forward(block, a[:, o:o + ni])[-1])
                o += ni
            a = np.concatenate(outs, axis=1)
        else:
            raise ValueError(L.tag)
        acts.append(a)
    return acts


def cpu_step(layers, X, lab, lr):
    """One step with the CPU twins' single-thread semantics (momentum 0, no weight decay, no division by the
    frames): <biasedlinearity> W -= lr X^T E (BiasedLinearity.cc), <sharedlinearity> W -= lr/N sum_i X_i^T E_i
    (SharedLinearity.cc:232-274).  Updates `layers` in place (float64 parameters); returns (Y, E, xent)."""
    acts = forward(layers, X)
    Y = acts[-1]
    T = np.zeros_like(Y)
    T[np.arange(len(lab)), lab] = 1.0
    xent = -np.log(np.maximum(Y[np.arange(len(lab)), lab], np.finfo(np.float32).tiny)).sum()
    E = Y - T
    err = E
    new = {}
    for k in range(len(layers) - 1, -1, -1):
        L, a_in = layers[k], acts[k]
        if L.tag == "<softmax>":
            pass
        elif L.tag == "<sigmoid>":
            err = err * acts[k + 1] * (1.0 - acts[k + 1])
        elif L.tag == "<biasedlinearity>":
            W = L.W.astype(np.float64)
            new[k] = (W - lr * a_in.T @ err, L.b - lr * err.sum(axis=0))
            err = err @ W.T
        elif L.tag == "<sharedlinearity>":
            n = L.extra["n_inst"]
            W = L.W.astype(np.float64)
            ni, no = W.shape
            g = sum(a_in[:, i * ni:(i + 1) * ni].T @ err[:, i * no:(i + 1) * no] for i in range(n))
            gb = sum(err[:, i * no:(i + 1) * no].sum(axis=0) for i in range(n))
            new[k] = (W - lr / n * g, L.b - lr / n * gb)
            err = np.concatenate([err[:, i * no:(i + 1) * no] @ W.T for i in range(n)], axis=1)
    for k, (W, b) in new.items():
        layers[k].W, layers[k].b = W, b
    return Y, E, xent


def param_arrays(layers, prefix):
    out, k = {}, 0
    for L in layers:
        if L.tag in ("<biasedlinearity>", "<sharedlinearity>"):
            out[f"{prefix}W{k}"] = np.asarray(L.W, np.float32)
            out[f"{prefix}b{k}"] = np.asarray(L.b, np.float32)
            k += 1
    return out


def check(name, got, ref, atol):
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=atol, err_msg=f"fixture {name} disagrees with the restatement")


# ---------------------------------------------------------------------------------- fixtures
def run_steps(name, layers, bunch, nsteps, lr, seed):
    rng = np.random.default_rng(seed)
    n_in, n_cls = layers[0].n_in, layers[-1].n_out
    X = rng.standard_normal((bunch * nsteps, n_in)).astype(np.float32)
    lab = rng.integers(0, n_cls, size=bunch * nsteps).astype(np.int32)
    with tempfile.TemporaryDirectory() as td:
        init = os.path.join(td, "init.nnet")
        formats.write_nnet(layers, init, precision=9)
        X.tofile(os.path.join(td, "X.f32"))
        lab.tofile(os.path.join(td, "lab.i32"))
        subprocess.run([os.path.join(REF, "ref_harness"), "step", init, os.path.join(td, "X.f32"),
                        os.path.join(td, "lab.i32"), str(n_in), str(n_cls), str(bunch), str(nsteps), repr(lr),
                        repr(0.0), td], check=True, env=ENV)
        arrs = {"X": X, "labels": lab, "bunch": np.int32(bunch), "lr": np.float32(lr), "wc": np.float32(0.0),
                "nnet": np.array(open(init).read())}
        model = formats.read_nnet(init)
        arrs.update(param_arrays(model, "init_"))
        xent = 0.0
        for s in range(nsteps):
            Y = np.fromfile(os.path.join(td, f"Y_{s}.f32"), np.float32).reshape(bunch, n_cls)
            E = np.fromfile(os.path.join(td, f"E_{s}.f32"), np.float32).reshape(bunch, n_cls)
            after = param_arrays(formats.read_nnet(os.path.join(td, f"nnet_{s}.txt")), f"step{s}_")
            Yr, Er, x = cpu_step(model, X[s * bunch:(s + 1) * bunch], lab[s * bunch:(s + 1) * bunch], lr)
            xent += x
            check(f"{name} Y_{s}", Y, Yr, ATOL_Y)
            check(f"{name} E_{s}", E, Er, ATOL_Y)
            for key, ref in param_arrays(model, f"step{s}_").items():
                check(f"{name} {key}", after[key], ref, ATOL_P)
            arrs[f"Y_{s}"], arrs[f"E_{s}"] = Y, E
            arrs.update(after)
        with open(os.path.join(td, "report.txt")) as f:
            err, frames = f.readline().split()
        np.testing.assert_allclose(float(err), xent, rtol=1e-5)
        arrs["xent_sum"] = np.float64(err)
        arrs["frames"] = np.int64(frames)
    save_npz_parts(os.path.join(HERE, name), arrs)
    print("wrote", name)


def run_blockarray(name, seed):
    rng = np.random.default_rng(seed)
    b1 = formats.gen_mlp_init([10, 7], seed=seed + 1)
    b1[-1] = formats.Layer("<sigmoid>", 7, 7)
    b2 = formats.gen_shared_init(2, 9, 5, seed=seed + 2, negbias=False)
    layers = [formats.Layer("<blockarray>", 17, 28, extra={"blocks": [b1, b2]})]
    X = rng.standard_normal((33, 28)).astype(np.float32)
    with tempfile.TemporaryDirectory() as td:
        net = os.path.join(td, "ba.nnet")
        formats.write_nnet(layers, net, precision=9)
        fea = os.path.join(td, "x.fea")
        formats.write_htk(fea, X)
        scp = os.path.join(td, "x.scp")
        open(scp, "w").write(fea + "\n")
        outdir = os.path.join(td, "out")
        os.makedirs(outdir)
        subprocess.run([os.path.join(REF, "TFeaCat"), "-S", scp, "-H", net, "-l", outdir, "-y", "fea"], check=True,
                       env=ENV, cwd=td)
        Y = formats.read_htk(os.path.join(outdir, "x.fea"))
        text = open(net).read()
    check(name, Y, forward(formats.read_nnet(text), X)[-1], ATOL_Y)
    np.savez_compressed(os.path.join(HERE, name), X=X, Y=Y, nnet=np.array(text))
    print("wrote", name)


def shared_first():
    top = formats.gen_mlp_init([48, 10], seed=32)
    return formats.gen_shared_init(3, 24, 16, seed=31, negbias=False) + top


def shared_stack():
    top = formats.gen_mlp_init([18, 10], seed=43)
    return (formats.gen_shared_init(3, 20, 12, seed=41, negbias=False) +
            formats.gen_shared_init(3, 12, 6, seed=42, negbias=False) + top)


if __name__ == "__main__":
    run_steps("shared_steps_first.npz", shared_first(), bunch=16, nsteps=4, lr=0.5, seed=7)
    run_steps("shared_steps_stack.npz", shared_stack(), bunch=16, nsteps=1, lr=0.5, seed=8)
    run_blockarray("blockarray_fwd.npz", seed=9)
