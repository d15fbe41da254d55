#!/usr/bin/env python3
"""tfeacat.py -- the TFeaCatCu step of a TNet recipe (src/TFeaCatCu.cc) on this library.

Propagates every utterance of a script file (and of the feature files named on the command line) through the feature
transform and the network on the GPU and writes the output -- posteriors, log posteriors, the GMMBYPASS form HVite
takes, or bottleneck features -- as one HTK file per utterance: TARGETPARAMDIR/basename.TARGETPARAMEXT, kind USER.
Option names and defaults are TFeaCatCu's.

  tools/tfeacat.py -S test.scp -H final.nnet --FEATURETRANSFORM=hamm_dct_norm.nnet -l out -y fea \\
      --STARTFRMEXT=25 --ENDFRMEXT=25 --GMMBYPASS=TRUE
"""
import argparse
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PACKING = ("Utterances are packed back to back into bunches of --pack-rows rows when no component of the network mixes "
           "rows; a network with an <expand> or a recurrence inside runs one utterance a pass.  Several GPUs: start one "
           "process per GPU with --rank R --world N; rank R takes every N-th utterance from the R-th on (the pass has no "
           "reduction, so that is all there is to it).")


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
    p = argparse.ArgumentParser(prog="tfeacat.py", description=__doc__.split("\n\n")[1], epilog=PACKING,
                                formatter_class=argparse.RawDescriptionHelpFormatter, allow_abbrev=False)
    p.add_argument("files", nargs="*", metavar="feature-file", help="feature files, after those of the script")
    p.add_argument("-S", "--SCRIPT", dest="script", metavar="file", help="script file (feature list)")
    p.add_argument("-H", "--SOURCEMMF", dest="mmf", metavar="mmf", help="the network (.nnet); an empty file: the "
                   "transform's output")
    p.add_argument("--FEATURETRANSFORM", dest="featuretransform", metavar="mmf", help="the feature transform (.nnet)")
    p.add_argument("-l", "--TARGETPARAMDIR", dest="targetparamdir", metavar="dir", help="output directory")
    p.add_argument("-y", "--TARGETPARAMEXT", dest="targetparamext", default="fea", metavar="ext",
                   help="output file extension (default: fea)")
    p.add_argument("--GMMBYPASS", dest="gmmbypass", type=_bool, nargs="?", const=True, default=False,
                   metavar="TRUE|FALSE", help="y <- sqrt(-2 log y): posteriors as features for HVite")
    p.add_argument("--LOGPOSTERIOR", dest="logposterior", type=_bool, nargs="?", const=True, default=False,
                   metavar="TRUE|FALSE", help="y <- log y (after GMMBYPASS when both are set)")
    p.add_argument("--STARTFRMEXT", dest="startfrmext", type=_nonneg, default=0, metavar="N",
                   help="context frames repeated before every utterance (propagated, not written)")
    p.add_argument("--ENDFRMEXT", dest="endfrmext", type=_nonneg, default=0, metavar="N",
                   help="context frames repeated after every utterance")
    p.add_argument("--NATURALREADORDER", dest="naturalreadorder", type=_bool, nargs="?", const=True, default=False,
                   metavar="TRUE|FALSE", help="features are in this host's byte order (default: big-endian HTK); "
                   "the output follows, as in the reference")
    p.add_argument("--CMEANDIR", dest="cmeandir", metavar="dir", help="cepstral mean files: directory")
    p.add_argument("--CMEANMASK", dest="cmeanmask", metavar="mask", help="cepstral mean files: name mask (turns CMN on)")
    p.add_argument("--VARSCALEDIR", dest="varscaledir", metavar="dir", help="variance files: directory")
    p.add_argument("--VARSCALEMASK", dest="varscalemask", metavar="mask", help="variance files: name mask (turns CVN on)")
    p.add_argument("--VARSCALEFN", dest="varscalefn", metavar="file", help="global variance file")
    p.add_argument("--pack-rows", dest="pack_rows", type=_nonneg, default=0, metavar="N",
                   help="rows of a pack (default: the library's)")
    p.add_argument("--rank", type=_nonneg, default=0, metavar="R", help="this process's share of the utterances ...")
    p.add_argument("--world", type=int, default=1, metavar="N", help="... of N processes")
    p.add_argument("--threads", type=int, default=4, help="feature reader threads")
    p.add_argument("-T", "--TRACE", dest="trace", type=int, default=0, metavar="N", help="trace flags")
    return p


def parse_args(argv=None):
    p = parser()
    a = p.parse_args(argv)
    if not a.mmf:
        p.error("Source MMF must be specified [-H]")
    if not a.script and not a.files:
        p.error("No input features specified, try [-S SCP] or positional argument")
    if a.world < 1 or not 0 <= a.rank < a.world:
        p.error(f"--rank {a.rank} outside --world {a.world}")
    return a


def records(script, files):
    """the feature list in the reference's order: the files of the command line, then the script's lines
    (TFeaCatCu.cc:175-205: AddFile per argument, then AddFileList)"""
    out = list(files)
    if script:
        out += [l.strip() for l in open(script) if l.strip()]
    return out


def main(argv=None):
    a = parse_args(argv)
    sys.path.insert(0, os.path.join(REPO, "nnet-asr_amd"))
    import tnet_amd

    t0 = time.time()
    recs = tnet_amd.shard_utterances(records(a.script, a.files), a.rank, a.world)
    if a.trace & 1:
        print(f"Reading network: {a.mmf}", flush=True)
    net = tnet_amd.Network(path=a.mmf)
    transform = tnet_amd.Network(path=a.featuretransform) if a.featuretransform else None
    fwd = tnet_amd.Forwarder(net, transform, start_ext=a.startfrmext, end_ext=a.endfrmext,
                             log_posterior=a.logposterior, gmm_bypass=a.gmmbypass, pack_rows=a.pack_rows or None)
    fwd.set_output(a.targetparamdir, a.targetparamext, swap=not a.naturalreadorder)
    with tempfile.TemporaryDirectory() as td:
        scp = os.path.join(td, "shard.scp")
        with open(scp, "w") as f:
            f.writelines(r + "\n" for r in recs)
        if recs:
            reader = tnet_amd.FeatureReader(scp, start_ext=a.startfrmext, end_ext=a.endfrmext,
                                            swap=not a.naturalreadorder, threads=a.threads, cmn_dir=a.cmeandir,
                                            cmn_mask=a.cmeanmask, cvn_dir=a.varscaledir, cvn_mask=a.varscalemask,
                                            cvg_file=a.varscalefn)
            fwd.add_reader(reader)
        fwd.finish()
    if a.trace & 1:
        s = fwd.stats()
        dt = max(time.time() - t0, 1e-9)
        print(f"TFeaCat finished: {dt:g}s  [{s['utterances']} utterances, {s['frames']} frames, {s['packs']} network "
              f"passes, {'packed' if s['packed'] else 'one utterance a pass'}, {s['frames'] / dt:g} frames/s]")
    return 0


if __name__ == "__main__":
    sys.exit(main())
