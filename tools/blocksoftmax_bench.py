#!/usr/bin/env python3
"""<blocksoftmax>: the fused objective tnet_block_softmax_xent next to the three calls it replaces
(tnetF_block_softmax -> tnet_softmax_xent with Z = NULL -> tnet_block_softmax_bwd) and to the plain
tnet_softmax_xent on a matrix of the same shape -- the plain kernel moves the same bytes (Z read, E written) and is
the yardstick.

Timing (the method of tools/sparse_bench.py): device events around `iters` back-to-back calls on the
library stream, after a warm-up of every variant; the variants alternate for `rounds` rounds and the median, minimum
and maximum per-call time of each are reported.  `bytes` is what one call has to move: Z once, E once, the labels.

The whole step: frames/s of 440 -> 2048 x 4 -> 4000 with a 4 x 1000 <blocksoftmax> top against the same net with
<softmax>, bunch 1024, through Trainer.replay (host clock around `steps` steps after a warm-up, alternating).

usage: python tools/blocksoftmax_bench.py [--out profiles/blocksoftmax.json] [--iters 200] [--rounds 7]"""
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
from tnet_amd import DeviceArray, Network, Objective, Trainer, formats  # noqa: E402
from tnet_amd._lib import check, lib  # noqa: E402

SHAPES = {"4x1000": (1000,) * 4, "2x2000": (2000,) * 2, "24x135": (135,) * 24, "135+4000": (135, 4000)}
BUNCHES = [1024, 256]
VARIANTS = ("fused", "chain", "plain")


def S():
    return lib().tnet_stream()


def timed(fn, iters):
    check(lib().tnet_timer_start())
    for _ in range(iters):
        fn()
    ms = C.c_float()
    check(lib().tnet_timer_stop(C.byref(ms)))
    return 1e3 * ms.value / iters  # us per call


def build(rows, dims):
    rng = np.random.default_rng(0)
    N, B, L = sum(dims), len(dims), lib()
    Z = DeviceArray.from_numpy((rng.standard_normal((rows, N)) * 3).astype(np.float32))
    lab = DeviceArray.vector(rng.integers(0, N, size=rows).astype(np.int32))
    off = DeviceArray.vector(np.concatenate([[0], np.cumsum(dims)]).astype(np.int32))
    Y, E = DeviceArray(rows, N), DeviceArray(rows, N)
    stats = DeviceArray(1, 1024, np.float64, stride=1024)
    inv = DeviceArray.vector(np.zeros(1, np.int32))

    def fused():
        check(L.tnet_block_softmax_xent(Z.ptr, Z.dim, off.ptr, B, lab.ptr, None, 0, E.ptr, E.stride, stats.ptr, S()))

    def chain():
        check(L.tnetF_block_softmax(Y.ptr, Z.ptr, Z.dim, off.ptr, B, S()))
        check(L.tnet_softmax_xent(None, Y.dim, lab.ptr, Y.ptr, Y.stride, E.ptr, E.stride, stats.ptr, S()))
        check(L.tnet_block_softmax_bwd(E.ptr, E.dim, off.ptr, B, E.ptr, E.stride, inv.ptr, S()))

    def plain():
        check(L.tnet_softmax_xent(Z.ptr, Z.dim, lab.ptr, None, 0, E.ptr, E.stride, stats.ptr, S()))

    return {"fused": fused, "chain": chain, "plain": plain}, (Z, lab, off, Y, E, stats, inv)


def step_rate(top, steps, rounds):
    """frames/s of the whole step for each top layer, alternating"""
    dims, B = [440, 2048, 2048, 2048, 2048, 4000], 1024
    runs = {}
    for name in top:
        layers = formats.gen_mlp_init(dims, seed=1)
        if name == "blocksoftmax":
            layers[-1] = formats.Layer("<blocksoftmax>", 4000, 4000, extra={"dims": [1000] * 4})
        net = Network.from_layers(layers)
        net.set_learn_rate(0.008)
        net.set_grad_div_frm(True)
        obj = Objective()
        tr = Trainer(net, obj, bunchsize=B, cachesize=8 * B, seed=1, randomize=True)
        rng = np.random.default_rng(2)
        X = rng.standard_normal((8 * B, dims[0])).astype(np.float32)
        lab = rng.integers(0, dims[-1], size=8 * B).astype(np.int32)
        took = lib().tnet_trainer_prefill(tr.h, X.ctypes.data, X.shape[0], X.shape[1], X.shape[1], lab.ctypes.data)
        assert took == 8 * B, took
        tr.replay(20)
        tnet_amd.synchronize()
        runs[name] = (tr, net, obj)
    t = {name: [] for name in top}
    for _ in range(rounds):
        for name in top:
            tr = runs[name][0]
            t0 = time.perf_counter()
            tr.replay(steps)
            tnet_amd.synchronize()
            t[name].append(B * steps / (time.perf_counter() - t0))
    return {name: {"frames_per_s": round(float(np.median(v))), "min_max": [round(min(v)), round(max(v))]}
            for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "blocksoftmax.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    a = ap.parse_args()
    results = []
    for shape, dims in SHAPES.items():
        for rows in BUNCHES:
            fns, keep = build(rows, dims)
            for name in VARIANTS:  # warm-up: code objects, clocks
                timed(fns[name], 20)
            t = {name: [] for name in VARIANTS}
            for _ in range(a.rounds):
                for name in VARIANTS:
                    t[name].append(timed(fns[name], a.iters))
            nbytes = 8.0 * rows * sum(dims) + 4.0 * rows
            rec = {"shape": shape, "bunch": rows, "cols": sum(dims), "blocks": len(dims), "bytes": int(nbytes)}
            for name in VARIANTS:
                rec[name + "_us"] = round(float(np.median(t[name])), 2)
                rec[name + "_us_min_max"] = [round(min(t[name]), 2), round(max(t[name]), 2)]
            rec["fused_over_plain"] = round(rec["fused_us"] / rec["plain_us"], 3)
            rec["chain_over_fused"] = round(rec["chain_us"] / rec["fused_us"], 3)
            rec["fused_gbytes_per_s"] = round(nbytes / rec["fused_us"] / 1e3, 1)
            print(json.dumps(rec), flush=True)
            results.append(rec)
            tnet_amd.synchronize()
            del fns, keep
    step = step_rate(("softmax", "blocksoftmax"), a.steps, a.rounds)
    step["blocksoftmax_over_softmax"] = round(step["blocksoftmax"]["frames_per_s"] / step["softmax"]["frames_per_s"], 4)
    print(json.dumps(step), flush=True)
    doc = {"what": "tnet_block_softmax_xent (fused) vs tnetF_block_softmax + tnet_softmax_xent(Z = NULL) + "
                   "tnet_block_softmax_bwd (chain) vs tnet_softmax_xent on the same matrix (plain); device-event time "
                   "per call in us, median of `rounds` alternating windows of `iters` calls each (min / max beside "
                   "it).  step: frames/s of 440-2048x4-4000 at bunch 1024 through Trainer.replay, <softmax> top vs a "
                   "4 x 1000 <blocksoftmax> top, median of `rounds` alternating windows of `steps` steps",
           "iters": a.iters, "rounds": a.rounds, "steps": a.steps, "version": lib().tnet_version().decode(),
           "results": results, "step": step}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
