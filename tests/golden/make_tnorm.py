#!/usr/bin/env python3
"""Reference statistics for the normalisation pass on examples/01 -> tests/golden/tnorm_ex01.npz.

Runs only in the build container (needs oracle/_ref/TFeaCat, built by ``make -C oracle ref``).  The first four
components of tests/golden/ex01/Hamm_dct_norm (<expand> <transpose> <window> <blocklinearity>: the transform BEFORE
its own normalisation pair) are written to a temporary file and given to the reference CPU TFeaCat as
--FEATURETRANSFORM with an empty network, --STARTFRMEXT=25 --ENDFRMEXT=25, over the 100 utterances of test.scp (the
call of make_ex01.py's feacat()).  Its output -- what TNormCu's loop sees after the trim -- goes through the float64
restatement of TNormCu.cc:262-327 in tests/tnorm_cases.py.  Stored, for both frame-count modes ("ext": the
reference's N including the context rows, "true": the summed rows):
  first, second, abs_sum [598]  float64 sums of y, of the fp32 squares y*y, of |y|
  summed, frames_ext, frames_true
  bias_ext / window_ext, bias_true / window_true [598]
  text_ext, text_true           the norm file TNormCu would write
No reference program text is stored; the transform output itself (55,457 x 598 floats) is not stored either.
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
import tnorm_cases as tc  # noqa: E402
from tnet_amd import formats  # noqa: E402

EX = os.path.join(HERE, "ex01")
REF = os.path.join(REPO, "oracle", "_ref")
ENV = dict(os.environ, MKL_NUM_THREADS="1", MKL_CBWR="COMPATIBLE", OMP_NUM_THREADS="1")
HEAD = 4  # <expand> <transpose> <window> <blocklinearity>


def head_layers():
    return formats.read_nnet(os.path.join(EX, "Hamm_dct_norm"))[:HEAD]


def main():
    scp = os.path.join(EX, "test.scp")
    names = [os.path.splitext(os.path.basename(l.strip()))[0] for l in open(scp) if l.strip()]
    with tempfile.TemporaryDirectory() as td:
        head = os.path.join(td, "head.nnet")
        formats.write_nnet(head_layers(), head, precision=9)   # 9 digits: the float32 values exactly
        empty = os.path.join(td, "empty.nnet")
        open(empty, "w").close()
        outdir = os.path.join(td, "out")
        os.makedirs(outdir)
        p = subprocess.run([os.path.join(REF, "TFeaCat"), "-S", scp, "-H", empty, "-l", outdir, "-y", "fea",
                            f"--FEATURETRANSFORM={head}", f"--STARTFRMEXT={tc.EX01_EXT}", f"--ENDFRMEXT={tc.EX01_EXT}"],
                           capture_output=True, text=True, env=ENV, cwd=EX)
        if p.returncode != 0:
            raise SystemExit("reference TFeaCat failed: " + p.stdout[-2000:] + p.stderr[-2000:])
        accs = {"ext": tc.Accumulator(598, tc.EX01_EXT, tc.EX01_EXT, True),
                "true": tc.Accumulator(598, tc.EX01_EXT, tc.EX01_EXT, False)}
        for n in names:
            y = formats.read_htk(os.path.join(outdir, n + ".fea"))
            for a in accs.values():
                a.add(y)
    a = accs["ext"]
    assert a.summed == tc.EX01_FRAMES and a.frames == tc.EX01_FRAMES_EXT and accs["true"].frames == tc.EX01_FRAMES
    arrs = dict(first=a.first, second=a.second, abs_sum=a.abs_sum, summed=np.int64(a.summed),
                frames_ext=np.int64(a.frames), frames_true=np.int64(accs["true"].frames))
    for mode, acc in accs.items():
        bias, window = tc.finish(acc.first, acc.second, acc.frames)
        arrs[f"bias_{mode}"], arrs[f"window_{mode}"] = bias, window
        arrs[f"text_{mode}"] = np.array(tc.norm_text(bias, window))
    np.savez_compressed(os.path.join(HERE, "tnorm_ex01.npz"), **arrs)
    print("wrote tnorm_ex01.npz", os.path.getsize(os.path.join(HERE, "tnorm_ex01.npz")), "bytes")


if __name__ == "__main__":
    main()
