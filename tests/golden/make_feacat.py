#!/usr/bin/env python3
"""Reference outputs of the forward pass in its four output modes (tests/golden/feacat_ref.npz).

Runs only in the build container: drives the reference CPU TFeaCat (oracle/_ref/TFeaCat, built by ``make -C oracle
ref``; TFeaCat.cc:239-254 is TFeaCatCu.cc:244-259 line for line) on UTTS of tests/golden/ex01 -- the three shortest
utterances, so that two can be stored in full, and three ordinary ones -- with the real Hamm_dct_norm transform, frame
extension 25/25, and the seeded 598:64:135 MLP formats.gen_mlp_init(**INIT) written at 6 digits (not stored: the tests
re-generate it).  Modes: none, --LOGPOSTERIOR, --GMMBYPASS, both.

  names                the utterances, in the order run
  <mode>_rows          per utterance: rows of the written file
  <mode>_period/_kind/_size   per utterance: the header's sample period, parameter kind and sample size
  <mode>_sum/_sumsq    per utterance: float64 sum and sum of squares over the FINITE elements
  <mode>_nonfinite     per utterance: elements that are not finite (log of a posterior that underflowed)
  <mode>_Y_<name>      FULL utterances in full (float32)
  file_<mode>_<name>   the raw bytes of RAWFILE's written file in mode RAWMODE (header + big-endian body)

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
from tnet_amd import formats  # noqa: E402

EX = os.path.join(HERE, "ex01")
REF = os.path.join(REPO, "oracle", "_ref")
ENV = dict(os.environ, MKL_NUM_THREADS="1", MKL_CBWR="COMPATIBLE", OMP_NUM_THREADS="1")

INIT = dict(dims=[598, 64, 135], seed=7)
UTTS = ["040", "086", "011", "001", "002", "003"]
FULL = ["040", "086"]
RAWFILE, RAWMODE = "040", "gmmbypass"
MODES = dict(none=[], logposterior=["--LOGPOSTERIOR=TRUE"], gmmbypass=["--GMMBYPASS=TRUE"],
             both=["--GMMBYPASS=TRUE", "--LOGPOSTERIOR=TRUE"])
EXT = 25


def write_init(path):
    formats.write_nnet(formats.gen_mlp_init(INIT["dims"], seed=INIT["seed"]), path, precision=6)


def write_scp(path):
    with open(path, "w") as f:
        f.writelines(os.path.join(EX, "features", n + ".fea") + "\n" for n in UTTS)


def main():
    arrs = {"names": np.array(UTTS)}
    with tempfile.TemporaryDirectory() as td:
        net, scp = os.path.join(td, "init.nnet"), os.path.join(td, "utts.scp")
        write_init(net)
        write_scp(scp)
        for mode, extra in MODES.items():
            out = os.path.join(td, mode)
            os.makedirs(out)
            p = subprocess.run([os.path.join(REF, "TFeaCat"), "-S", scp, "-H", net, "-l", out, "-y", "fea",
                                f"--FEATURETRANSFORM={os.path.join(EX, 'Hamm_dct_norm')}", f"--STARTFRMEXT={EXT}",
                                f"--ENDFRMEXT={EXT}"] + extra, capture_output=True, text=True, env=ENV, cwd=EX)
            if p.returncode != 0:
                raise SystemExit("reference TFeaCat failed: " + p.stdout[-2000:] + p.stderr[-2000:])
            rows, per, kind, size, sums, sqs, bad = [], [], [], [], [], [], []
            for n in UTTS:
                path = os.path.join(out, n + ".fea")
                h = formats.read_htk_header(path)
                y = formats.read_htk(path)
                fin = np.isfinite(y)
                y64 = np.where(fin, y, 0).astype(np.float64)
                rows.append(h[0]); per.append(h[1]); size.append(h[2]); kind.append(h[3])
                sums.append(y64.sum()); sqs.append((y64 ** 2).sum()); bad.append(int((~fin).sum()))
                if n in FULL:
                    arrs[f"{mode}_Y_{n}"] = y
                if n == RAWFILE and mode == RAWMODE:
                    arrs[f"file_{mode}_{n}"] = np.frombuffer(open(path, "rb").read(), np.uint8)
            arrs.update({f"{mode}_rows": np.array(rows, np.int64), f"{mode}_period": np.array(per, np.int64),
                         f"{mode}_kind": np.array(kind, np.int64), f"{mode}_size": np.array(size, np.int64),
                         f"{mode}_sum": np.array(sums), f"{mode}_sumsq": np.array(sqs),
                         f"{mode}_nonfinite": np.array(bad, np.int64)})
            print(mode, rows, bad)
    dst = os.path.join(HERE, "feacat_ref.npz")
    np.savez_compressed(dst, **arrs)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
