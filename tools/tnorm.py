#!/usr/bin/env python3
"""tnorm.py -- the TNormCu step of a TNet recipe (src/TNormCu.cc) on this library.

Propagates every utterance of a script file through a feature transform on the GPU, accumulates the per-column
mean and variance of the output (context rows left out) and writes the global normalisation as a <bias> + <window>
pair -- the file tnorm_scheduler.sh `cat`s onto the transform.  Option names are TNormCu's.

  tools/tnorm.py -S train.scp -H hamm_dct.nnet --TARGETMMF=norm.nnet --STARTFRMEXT=25 --ENDFRMEXT=25 \\
      --assemble hamm_dct_norm.nnet
"""
import argparse
import os
import shutil
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QUIRK = ("Frame count: the reference TNormCu divides by the number of frames INCLUDING the STARTFRMEXT + ENDFRMEXT "
         "context frames of every utterance, although only the frames between them are summed (on examples/01 at 25 + 25 "
         "context frames: N = 60,457 for 55,457 summed frames, a mean 0.917 of the true one).  Transforms in use were "
         "made this way, so that is the default; --true-frame-count divides by the summed frames.")


def _bool(s):
    v = str(s).strip().lower()
    if v in ("true", "t", "1", "yes", "on"):
        return True
    if v in ("false", "f", "0", "no", "off"):
        return False
    raise argparse.ArgumentTypeError(f"not a boolean: {s!r}")


def _nonneg(s):
    v = int(s)
    if v < 0:
        raise argparse.ArgumentTypeError("must be >= 0")
    return v


def parser():
    p = argparse.ArgumentParser(prog="tnorm.py", description=__doc__.split("\n\n")[1], epilog=QUIRK,
                                formatter_class=argparse.RawDescriptionHelpFormatter, allow_abbrev=False)
    p.add_argument("-S", "--SCRIPT", dest="script", required=True, metavar="file", help="script file (feature list)")
    p.add_argument("-H", "--SOURCEMMF", dest="mmf", metavar="mmf",
                   help="the feature transform (.nnet) whose output is normalised")
    p.add_argument("--TARGETMMF", dest="targetmmf", required=True, metavar="file",
                   help="output: the <bias> + <window> normalisation")
    p.add_argument("--STARTFRMEXT", dest="startfrmext", type=_nonneg, default=0, metavar="N",
                   help="context frames repeated before every utterance (propagated, not summed)")
    p.add_argument("--ENDFRMEXT", dest="endfrmext", type=_nonneg, default=0, metavar="N",
                   help="context frames repeated after every utterance")
    p.add_argument("--NATURALREADORDER", dest="naturalreadorder", type=_bool, nargs="?", const=True, default=False,
                   metavar="TRUE|FALSE", help="features are in this host's byte order (default: big-endian HTK)")
    p.add_argument("--CMEANDIR", dest="cmeandir", metavar="dir", help="cepstral mean files: directory")
    p.add_argument("--CMEANMASK", dest="cmeanmask", metavar="mask", help="cepstral mean files: name mask (turns CMN on)")
    p.add_argument("--VARSCALEDIR", dest="varscaledir", metavar="dir", help="variance files: directory")
    p.add_argument("--VARSCALEMASK", dest="varscalemask", metavar="mask", help="variance files: name mask (turns CVN on)")
    p.add_argument("--VARSCALEFN", dest="varscalefn", metavar="file", help="global variance file")
    p.add_argument("--true-frame-count", dest="true_frame_count", action="store_true",
                   help="divide by the frames that were summed, not by the reference's count (see below)")
    p.add_argument("--assemble", dest="assemble", metavar="OUT",
                   help="also write the transform followed by the normalisation as one file (cat SOURCEMMF TARGETMMF)")
    p.add_argument("--threads", type=int, default=4, help="feature reader threads")
    p.add_argument("-T", "--TRACE", dest="trace", type=int, default=0, metavar="N", help="trace flags")
    return p


def parse_args(argv=None):
    p = parser()
    a = p.parse_args(argv)
    if not a.mmf:
        p.error("Source MMF must be specified [-H]")
    return a


def assemble(mmf, norm, out):
    """the scheduler's `cat $MMF $NORM > $OUT`"""
    with open(out, "wb") as o:
        for src in (mmf, norm):
            with open(src, "rb") as f:
                shutil.copyfileobj(f, o)


def main(argv=None):
    a = parse_args(argv)
    sys.path.insert(0, os.path.join(REPO, "nnet-asr_amd"))
    import tnet_amd

    t0 = time.time()
    print("===== TNormCu STARTED =====", flush=True)
    transform = tnet_amd.Network(path=a.mmf)
    reader = tnet_amd.FeatureReader(a.script, start_ext=a.startfrmext, end_ext=a.endfrmext,
                                    swap=not a.naturalreadorder, threads=a.threads, cmn_dir=a.cmeandir,
                                    cmn_mask=a.cmeanmask, cvn_dir=a.varscaledir, cvn_mask=a.varscalemask,
                                    cvg_file=a.varscalefn)
    norm = tnet_amd.Normalizer(transform, start_ext=a.startfrmext, end_ext=a.endfrmext,
                               count_ext_frames=not a.true_frame_count)
    norm.add_reader(reader)
    norm.finish()
    norm.write(a.targetmmf)
    if a.assemble:
        assemble(a.mmf, a.targetmmf, a.assemble)
    dt = max(time.time() - t0, 1e-9)
    _, _, frames = norm.stats()
    print(f"\n\n===== TNormCu FINISHED ( {dt:g}s ) [FPS:{frames / dt:g},RT:{1.0 / (frames / dt / 100.0):g}] =====")
    print(norm.report(), end="")
    bad = norm.bad_window_entries()
    if bad:
        print(f"WARNING: {bad} of {norm.dim} window entries are inf / nan (zero or negative variance)", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
