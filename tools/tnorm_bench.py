#!/usr/bin/env python3
"""The normalisation pass (tnet_amd.Normalizer, TNormCu's loop): its reduction kernel and the whole pass.

Kernel: tnet_col_moments on one matrix next to tnetF_add_col_sum on the same matrix -- the column-sum kernel reads
the same bytes once and is the yardstick.  Timing (the method of tools/sparse_bench.py): device events
around `iters` back-to-back calls on the library stream, after a warm-up of both; the two alternate for `rounds` rounds
and the median, minimum and maximum per-call time of each are reported.

Whole pass: frames/s over the examples/01 corpus (tests/golden/ex01, held in host memory with the recipe's 25 + 25
context frames, the first four components of its Hamm_dct_norm as the transform) through Normalizer.add + finish,
beside a baseline written here from existing calls that does what the reference does (TNormCu.cc:233-290): per
utterance Network.propagate, copy the output back, accumulate x and x*x on the host (numpy, float64).  Host clock
around each pass, alternating, median of `rounds`.

usage: python tools/tnorm_bench.py [--out profiles/tnorm.json] [--iters 200] [--rounds 7]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nnet-asr_amd"))
import numpy as np  # noqa: E402

import tnet_amd  # noqa: E402
from tnet_amd import DeviceArray, Network, Normalizer, formats  # noqa: E402
from tnet_amd._lib import check, header_constant, lib  # noqa: E402

SHAPES = [(136, 598), (1024, 598), (5000, 1173)]
VARIANTS = ("col_moments", "add_col_sum")
EX = os.path.join(REPO, "tests", "golden", "ex01")
EXT = 25


def S():
    return lib().tnet_stream()


def timed(fn, iters):
    check(lib().tnet_timer_start())
    for _ in range(iters):
        fn()
    ms = C.c_float()
    check(lib().tnet_timer_stop(C.byref(ms)))
    return 1e3 * ms.value / iters  # us per call


def build(rows, cols):
    rng = np.random.default_rng(0)
    L = lib()
    X = DeviceArray.from_numpy(rng.standard_normal((rows, cols)).astype(np.float32))
    words = int(L.tnet_col_moments_words(cols))
    acc = DeviceArray(1, words, np.float64, stride=words)
    vec = DeviceArray(1, cols)
    ws_floats = max(int(L.tnet_col_sum_workspace(X.dim)) // 4, 1)
    ws = DeviceArray(1, ws_floats, stride=ws_floats)

    def col_moments():
        check(L.tnet_col_moments(X.ptr, X.dim, acc.ptr, 0, S()))

    def add_col_sum():
        check(L.tnetF_add_col_sum(1.0, X.ptr, 0.0, vec.ptr, X.dim, ws.ptr, S()))

    return {"col_moments": col_moments, "add_col_sum": add_col_sum}, (X, acc, vec, ws)


def kernel_bench(iters, rounds):
    results = []
    for rows, cols in SHAPES:
        fns, keep = build(rows, cols)
        for name in VARIANTS:  # warm-up: code objects, clocks
            timed(fns[name], 20)
        t = {name: [] for name in VARIANTS}
        for _ in range(rounds):
            for name in VARIANTS:
                t[name].append(timed(fns[name], iters))
        nbytes = 4.0 * rows * cols
        rec = {"rows": rows, "cols": cols, "bytes": int(nbytes),
               "load_form": "16-byte" if cols % 4 == 0 else "scalar",
               "workgroups": -(-cols // (256 if cols % 4 == 0 else 64)) *
               min(-(-rows // header_constant("TNET_COL_MOMENTS_ROWS")), header_constant("TNET_COL_MOMENTS_SLOTS"))}
        for name in VARIANTS:
            rec[name + "_us"] = round(float(np.median(t[name])), 2)
            rec[name + "_us_min_max"] = [round(min(t[name]), 2), round(max(t[name]), 2)]
        rec["col_moments_over_add_col_sum"] = round(rec["col_moments_us"] / rec["add_col_sum_us"], 3)
        rec["col_moments_gbytes_per_s"] = round(nbytes / rec["col_moments_us"] / 1e3, 1)
        print(json.dumps(rec), flush=True)
        results.append(rec)
        tnet_amd.synchronize()
        del fns, keep
    return results


def pass_bench(rounds):
    c = formats.read_corpus(os.path.join(EX, "test.scp"), os.path.join(EX, "test_3s.mlf"),
                            os.path.join(EX, "mono_state_phn_set_135_phn"))
    corpus = [formats.extend_frames(x, EXT, EXT) for x in c.feats]
    frames = sum(x.shape[0] for x in c.feats)
    head = formats.read_nnet(os.path.join(EX, "Hamm_dct_norm"))[:4]
    net = Network.from_layers(head, precision=9)

    def device_pass():
        nz = Normalizer(net, start_ext=EXT, end_ext=EXT)
        for xe in corpus:
            nz.add(xe)
        nz.finish()
        return nz.stats()

    def copy_back_pass():
        first, second = np.zeros(net.n_out), np.zeros(net.n_out)
        n = 0
        for xe in corpus:
            y = net.propagate(DeviceArray.from_numpy(xe)).numpy()[EXT:-EXT]
            first += y.astype(np.float64).sum(0)
            second += (y * y).astype(np.float64).sum(0)
            n += xe.shape[0]
        return first, second, n

    passes = {"device": device_pass, "copy_back": copy_back_pass}
    out = {name: fn() for name, fn in passes.items()}  # warm-up, and the two must agree
    assert out["device"][2] == out["copy_back"][2]
    assert np.allclose(out["device"][0], out["copy_back"][0], rtol=1e-9, atol=1e-6)
    t = {name: [] for name in passes}
    for _ in range(rounds):
        for name, fn in passes.items():
            tnet_amd.synchronize()
            t0 = time.perf_counter()
            fn()
            tnet_amd.synchronize()
            t[name].append(frames / (time.perf_counter() - t0))
    res = {name: {"frames_per_s": round(float(np.median(v))), "min_max": [round(min(v)), round(max(v))]}
           for name, v in t.items()}
    res["utterances"], res["frames"] = len(corpus), frames
    res["device_over_copy_back"] = round(res["device"]["frames_per_s"] / res["copy_back"]["frames_per_s"], 3)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tnorm.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    results = kernel_bench(a.iters, a.rounds)
    whole = pass_bench(a.rounds)
    doc = {"what": "tnet_col_moments vs tnetF_add_col_sum on the same matrix (the yardstick: the same bytes read once); "
                   "device-event time per call in us, median of `rounds` alternating windows of `iters` calls each "
                   "(min / max beside it).  pass: frames/s of the whole normalisation pass over the examples/01 "
                   "corpus in host memory (Normalizer.add + finish: sums on the device) beside the reference's shape "
                   "of the job from existing calls (Network.propagate, copy back, numpy float64 accumulation per "
                   "utterance); host clock, median of `rounds` alternating passes",
           "iters": a.iters, "rounds": a.rounds, "version": lib().tnet_version().decode(),
           "slab_rows": header_constant("TNET_COL_MOMENTS_ROWS"), "slots": header_constant("TNET_COL_MOMENTS_SLOTS"),
           "results": results, "pass": whole}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
