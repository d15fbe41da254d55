#!/usr/bin/env python3
"""Regenerate the <blocksoftmax> fixtures in tests/golden/ from the REFERENCE CPU TNet.

Runs only in the build container (needs oracle/_ref/ref_harness, built by ``make -C oracle ref``).  The fixtures are
data only: inputs generated here (seeded) and what the reference's CPU BlockSoftmax (src/TNetLib/Activation.cc:55-133)
under its cross-entropy computed on them through ``ref_harness step`` (bunch 16, 4 SGD steps, lr 0.5, wc 0).

  blocksoftmax_steps_mlp.npz     <biasedlinearity> 16 12, <sigmoid>, <biasedlinearity> 10 16, <blocksoftmax> 10 10 of
                                 blocks (3, 5, 2): a sigmoid MLP of <= 256 outputs -- the fused step.
  blocksoftmax_steps_shared.npz  <sharedlinearity> 48 72 (3 x 24->16), <sigmoid>, <biasedlinearity> 11 48,
                                 <blocksoftmax> 11 11 of blocks (1, 6, 4): the generic step.  The shared layer is first,
                                 so the CPU Network::Backpropagate never back-propagates through it (make_shared.py's
                                 note) and the whole trajectory is pinned.

The labels cover every block and every seventh one is -1 (an unlabeled frame: an all-zero target row).  Stored: inputs,
labels, the .nnet text, the parameters before and after every step, every step's output Y_s and the objective's
(unmasked) error E_s = Y - T, the cross-entropy sum, the frames and the correct count of the reference's report.

Before saving, everything is recomputed by the float64 restatement of tests/blocksoftmax_cases.py and must agree within
make_shared.py's pin tolerances (rtol 2e-4; atol 2e-6 outputs, 1e-6 parameters; xent rtol 1e-5), and in every row the
two largest whole-row posteriors of the restatement must differ by more than 2e-3 relative, so that the integer
correct count can be compared exactly (another seed if a row fails).
Reproducibility: MKL_NUM_THREADS=1 MKL_CBWR=COMPATIBLE.
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "nnet-asr_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import blocksoftmax_cases as cases  # noqa: E402
from tnet_amd import formats  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref")
ENV = dict(os.environ, MKL_NUM_THREADS="1", MKL_CBWR="COMPATIBLE", OMP_NUM_THREADS="1")


def check(name, got, ref, atol):
    np.testing.assert_allclose(got, ref, rtol=cases.RTOL, atol=atol,
                               err_msg=f"fixture {name} disagrees with the restatement")


def f32_params(layers, prefix):
    out, k = {}, 0
    for L in layers:
        if L.W is not None:
            out[f"{prefix}W{k}"] = np.asarray(L.W, np.float32)
            out[f"{prefix}b{k}"] = np.asarray(L.b, np.float32)
            k += 1
    return out


def run_steps(name, layers, dims, bunch, nsteps, lr, seed):
    rng = np.random.default_rng(seed)
    n_in, n_cls = layers[0].n_in, layers[-1].n_out
    X = rng.standard_normal((bunch * nsteps, n_in)).astype(np.float32)
    lab = cases.fixture_labels(dims, bunch * nsteps, seed + 100)
    with tempfile.TemporaryDirectory() as td:
        init = os.path.join(td, "init.nnet")
        formats.write_nnet(layers, init, precision=9)
        X.tofile(os.path.join(td, "X.f32"))
        lab.tofile(os.path.join(td, "lab.i32"))
        subprocess.run([os.path.join(REF, "ref_harness"), "step", init, os.path.join(td, "X.f32"),
                        os.path.join(td, "lab.i32"), str(n_in), str(n_cls), str(bunch), str(nsteps), repr(lr),
                        repr(0.0), td], check=True, env=ENV)
        arrs = {"X": X, "labels": lab, "bunch": np.int32(bunch), "lr": np.float32(lr), "wc": np.float32(0.0),
                "dims": np.asarray(dims, np.int32), "nnet": np.array(open(init).read())}
        model = formats.read_nnet(init)
        assert model[-1].extra["dims"] == list(dims)
        arrs.update(f32_params(model, "init_"))
        net = cases.Net(model)
        xent, correct = 0.0, 0
        for s in range(nsteps):
            Y = np.fromfile(os.path.join(td, f"Y_{s}.f32"), np.float32).reshape(bunch, n_cls)
            E = np.fromfile(os.path.join(td, f"E_{s}.f32"), np.float32).reshape(bunch, n_cls)
            after = f32_params(formats.read_nnet(os.path.join(td, f"nnet_{s}.txt")), f"step{s}_")
            Yr, Er, x, c = net.step(X[s * bunch:(s + 1) * bunch], lab[s * bunch:(s + 1) * bunch], lr)
            assert cases.margin_ok(Yr).all(), f"{name}: step {s}: two posteriors of a row too close; pick another seed"
            xent += x
            correct += c
            check(f"{name} Y_{s}", Y, Yr, cases.ATOL_Y)
            check(f"{name} E_{s}", E, Er, cases.ATOL_Y)
            for key, ref in net.params(f"step{s}_").items():
                check(f"{name} {key}", after[key], ref, cases.ATOL_P)
            arrs[f"Y_{s}"], arrs[f"E_{s}"] = Y, E
            arrs.update(after)
        with open(os.path.join(td, "report.txt")) as f:
            err, frames = f.readline().split()
            report = f.read()
        np.testing.assert_allclose(float(err), xent, rtol=cases.XENT_RTOL)
        # "Xent:... frames:F err/frm:... correct[P%]": the count is P% of the frames, an integer
        pct = float(re.search(r"correct\[([-+0-9.eE]+)%\]", report).group(1))
        ref_correct = int(round(pct * int(frames) / 100.0))
        assert abs(ref_correct - pct * int(frames) / 100.0) < 1e-3 * int(frames), report
        assert ref_correct == correct, (ref_correct, correct, report)
        arrs["xent_sum"] = np.float64(err)
        arrs["frames"] = np.int64(frames)
        arrs["correct"] = np.int64(ref_correct)
    np.savez_compressed(os.path.join(HERE, name), **arrs)
    print("wrote", name, "xent", float(err), "frames", frames, "correct", ref_correct, report.strip())


def mlp_net():
    return formats.gen_mlp_init([12, 16, 10], seed=51, negbias=False)[:2] + \
        formats.gen_blocksoftmax_top(16, cases.MLP_DIMS, seed=52)


def shared_net():
    return formats.gen_shared_init(3, 24, 16, seed=61, negbias=False) + \
        formats.gen_blocksoftmax_top(48, cases.SHARED_DIMS, seed=62)


if __name__ == "__main__":
    run_steps(cases.FIXTURES[0], mlp_net(), cases.MLP_DIMS, bunch=16, nsteps=4, lr=0.5, seed=11)
    run_steps(cases.FIXTURES[1], shared_net(), cases.SHARED_DIMS, bunch=16, nsteps=4, lr=0.5, seed=31)
