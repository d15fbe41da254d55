#!/usr/bin/env python3
"""Regenerate the golden fixtures in tests/golden/ from the REFERENCE CPU TNet.

Runs only in the build container (needs /root/reference and the binaries built by
``make -C oracle -f Makefile.ref``: oracle/_ref/TNet and oracle/_ref/ref_harness, the latter being
our own driver linked against the reference TNetLib/KaldiLib objects).  The fixtures are data only:
inputs we generate here (seeded) and the outputs the reference computed on them.

  steps_tiny.npz       24:32:32:10 sigmoid MLP, bunch 16, 4 SGD steps (CPU TNet semantics)
  steps_slice.npz      598:128:135 MLP3-shaped slice, bunch 64, 3 SGD steps, weight decay on
                       (+ steps_slice.part1.npz: tests/golden_io.py)
  shuffle.npz          cache permutations for (seed, n, cache, bunch) -- lrand48 + random_shuffle
  epoch_mlp3.json      one TNet epoch (THREADS=1) on a seeded synthetic 598-dim corpus with the
                       598:1024:135 MLP3: the reference's own Report() line and FPS
Reproducibility: MKL_NUM_THREADS=1 MKL_CBWR=COMPATIBLE.
"""
import json
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
from golden_io import save_npz_parts  # noqa: E402
from tnet_amd import formats  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref")
ENV = dict(os.environ, MKL_NUM_THREADS="1", MKL_CBWR="COMPATIBLE", OMP_NUM_THREADS="1")


def nnet_arrays(layers, prefix):
    out = {}
    k = 0
    for L in layers:
        if L.tag == "<biasedlinearity>":
            out[f"{prefix}W{k}"] = L.W
            out[f"{prefix}b{k}"] = L.b
            k += 1
    return out


def run_steps(name, dims, bunch, nsteps, lr, wc, seed, unlabeled=(), keep_all=True):
    rng = np.random.default_rng(seed)
    n_in, n_cls = dims[0], dims[-1]
    layers = formats.gen_mlp_init(dims, seed=seed + 100)
    nfr = bunch * nsteps
    X = rng.standard_normal((nfr, n_in)).astype(np.float32)
    lab = rng.integers(0, n_cls, size=nfr).astype(np.int32)
    for u in unlabeled:
        lab[u] = -1
    with tempfile.TemporaryDirectory() as td:
        init = os.path.join(td, "init.nnet")
        formats.write_nnet(layers, init, precision=9)
        X.tofile(os.path.join(td, "X.f32"))
        lab.tofile(os.path.join(td, "lab.i32"))
        subprocess.run([os.path.join(REF, "ref_harness"), "step", init, os.path.join(td, "X.f32"),
                        os.path.join(td, "lab.i32"), str(n_in), str(n_cls), str(bunch), str(nsteps),
                        repr(lr), repr(wc), td], check=True, env=ENV)
        arrs = {"X": X, "labels": lab, "dims": np.array(dims, np.int32),
                "bunch": np.int32(bunch), "lr": np.float32(lr), "wc": np.float32(wc)}
        arrs.update(nnet_arrays(formats.read_nnet(init), "init_"))
        for s in range(nsteps):
            arrs[f"Y_{s}"] = np.fromfile(os.path.join(td, f"Y_{s}.f32"), np.float32).reshape(bunch, n_cls)
            arrs[f"E_{s}"] = np.fromfile(os.path.join(td, f"E_{s}.f32"), np.float32).reshape(bunch, n_cls)
            if keep_all or s == nsteps - 1:
                arrs.update(nnet_arrays(formats.read_nnet(os.path.join(td, f"nnet_{s}.txt")), f"step{s}_"))
        with open(os.path.join(td, "report.txt")) as f:
            err, frames = f.readline().split()
            arrs["xent_sum"] = np.float64(err)
            arrs["frames"] = np.int64(frames)
            arrs["report"] = np.array(f.read().strip())
    save_npz_parts(os.path.join(HERE, name), arrs)  # (steps_slice: two parts, each under 1 MiB)
    print("wrote", name)


def run_shuffle():
    cases = [(123, 2000, 1920, 96), (7, 1000, 1000, 100), (1, 4096, 4096, 1024)]
    arrs = {}
    with tempfile.TemporaryDirectory() as td:
        for (seed, n, cache, bunch) in cases:
            p = os.path.join(td, "p.i32")
            subprocess.run([os.path.join(REF, "ref_harness"), "shuffle", str(seed), str(n), str(cache),
                            str(bunch), p], check=True, env=ENV)
            arrs[f"perm_{seed}_{n}_{cache}_{bunch}"] = np.fromfile(p, np.int32)
    np.savez_compressed(os.path.join(HERE, "shuffle.npz"), **arrs)
    print("wrote shuffle.npz")


# The epoch case is parameterised here and re-generated (not stored) by the tests: only the
# reference's reported numbers are fixtures.
EPOCH_MLP3 = dict(n_utts=100, dim=598, n_cls=135, corpus_seed=11, min_len=200, max_len=900,
                  dims=[598, 1024, 135], init_seed=1, bunch=1024, cache=8192, seed=123, lr=0.008,
                  threads=1)


EPOCH_MLP3_B256 = dict(EPOCH_MLP3, bunch=256, cache=4096, lr=0.002)


def run_epoch(cfg, name):
    corpus = formats.synth_corpus(cfg["n_utts"], cfg["dim"], cfg["n_cls"], seed=cfg["corpus_seed"],
                                  min_len=cfg["min_len"], max_len=cfg["max_len"])
    layers = formats.gen_mlp_init(cfg["dims"], seed=cfg["init_seed"])
    with tempfile.TemporaryDirectory() as td:
        files = formats.write_corpus_htk(corpus, td, cfg["n_cls"])
        init = os.path.join(td, "init.nnet")
        formats.write_nnet(layers, init, precision=6)
        out = os.path.join(td, "out.nnet")
        cmd = [os.path.join(REF, "TNet"), "-H", init, "-I", files["mlf"], "-L", "*/", "-X", "lab",
               "-S", files["scp"], "-m", files["states"], "-n", repr(cfg["lr"]),
               f"--TARGETMMF={out}", f"--BUNCHSIZE={cfg['bunch']}", f"--CACHESIZE={cfg['cache']}",
               "--RANDOMIZE=TRUE", f"--SEED={cfg['seed']}", f"--THREADS={cfg['threads']}"]
        p = subprocess.run(cmd, capture_output=True, text=True, env=ENV, cwd=td)
        if p.returncode != 0:
            print(p.stdout, p.stderr)
            raise SystemExit("reference TNet failed")
        m = re.search(r"Xent:(\S+) frames:(\d+) err/frm:(\S+) correct\[(\S+)%\]", p.stdout)
        fps = re.search(r"FPS:\s*([0-9.e+]+)", p.stdout)
        res = dict(cfg, xent=float(m.group(1)), frames=int(m.group(2)), err_per_frm=float(m.group(3)),
                   correct_pct=float(m.group(4)), ref_fps=float(fps.group(1)),
                   corpus_frames=corpus.frames, report=m.group(0))
    with open(os.path.join(HERE, name), "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", name, res["report"])


if __name__ == "__main__":
    run_steps("steps_tiny.npz", [24, 32, 32, 10], bunch=16, nsteps=4, lr=0.05, wc=0.0, seed=5,
              unlabeled=(3, 17))
    run_steps("steps_slice.npz", [598, 128, 135], bunch=64, nsteps=3, lr=0.002, wc=1e-4, seed=6, keep_all=False)
    run_shuffle()
    run_epoch(EPOCH_MLP3, "epoch_mlp3.json")
    run_epoch(EPOCH_MLP3_B256, "epoch_mlp3_b256.json")
