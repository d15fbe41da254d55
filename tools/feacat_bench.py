#!/usr/bin/env python3
"""The forward pass (tnet_amd.Forwarder, TFeaCatCu's loop): its fused output kernel and the whole pass.

Kernel: tnet_softmax_emit (LOGPOSTERIOR, big-endian) beside the calls it replaces on the same pre-softmax matrix --
tnetF_softmax + tnetF_apply_log + a device copy of the rows (what CopyRows moves) -- as device-event time per call
(`iters` back-to-back calls after a warm-up, the two alternating for `rounds` rounds; median, min, max).  The part of
the replaced job that is not a kernel is timed with the host clock, each side ending in its synchronous copy: the fused
side copies rows x C dense words; the replaced side copies the padded rows x stride matrix and swaps [:, :C] on the
host (numpy).

Whole pass, frames/s from host memory to written HTK files (LOGPOSTERIOR except (c), big-endian), host clock around a pass ending
in finish(), the variants alternating, median of `rounds`:
  packed     Forwarder, utterances packed into bunches of pack_rows rows
  unpacked   Forwarder with pack_rows = -1: one utterance a pass, context rows through the network, same kernels/sink
  host       the reference's shape of the job from existing calls: per utterance Network.propagate (transform, net),
             copy back, numpy trim + log + byte swap, formats.write_htk
  memory     packed, results kept in memory instead of files (what the writers cost)
over (a) examples/01 (tests/golden/ex01, the real Hamm_dct_norm, ext 25/25, a seeded 598:1024:135 MLP), (b) a
440:2048x4:4000 net and (c) a 440:2048x2:40 bottleneck net (no softmax: the unfused emit) on seeded synthetic utterances
of 200-1500 frames with 15 + 15 context rows.  The default pack_rows comes from the sweep over {1024 .. 8192} on (a), (b).
A pass over examples/01 lasts under 20 ms, too short for a host clock and dominated by the pass's set-up (its pinned
buffers), so every corpus goes through `--repeat` (4) times over in one pass.

usage: python tools/feacat_bench.py [--out profiles/feacat.json] [--iters 200] [--rounds 5] [--repeat 4]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nnet-asr_amd"))
import numpy as np  # noqa: E402

import tnet_amd  # noqa: E402
from tnet_amd import DeviceArray, Forwarder, Network, formats  # noqa: E402
from tnet_amd._lib import check, lib  # noqa: E402

SHAPES = [(64, 135), (1024, 135), (1024, 4000)]
EX = os.path.join(REPO, "tests", "golden", "ex01")
LOGPOSTERIOR = 2
SWEEP = (1024, 2048, 4096, 8192)


def S():
    return lib().tnet_stream()


def timed(fn, iters):
    check(lib().tnet_timer_start())
    for _ in range(iters):
        fn()
    ms = C.c_float()
    check(lib().tnet_timer_stop(C.byref(ms)))
    return 1e3 * ms.value / iters  # us per call


def _stat(v, nd=2):
    return {"median": round(float(np.median(v)), nd), "min_max": [round(min(v), nd), round(max(v), nd)]}


def kernel_bench(iters, rounds):
    L = lib()
    results = []
    for rows, cols in SHAPES:
        rng = np.random.default_rng(0)
        Z = DeviceArray.from_numpy((3 * rng.standard_normal((rows, cols))).astype(np.float32))
        Y, T = DeviceArray(rows, cols), DeviceArray(rows, cols)
        dense = DeviceArray(1, rows * cols, np.uint32, stride=rows * cols)
        one = (C.c_int * 1)
        src, dst, n = one(0), one(0), one(rows)
        host_dense = np.empty(rows * cols, np.uint32)
        host_pad = np.empty((rows, Y.stride), np.float32)

        def fused():
            check(L.tnet_softmax_emit(Z.ptr, Z.dim, src, dst, n, 1, LOGPOSTERIOR, 1, dense.ptr, S()))

        def replaced():
            check(L.tnetF_softmax(Y.ptr, Z.ptr, Z.dim, S()))
            check(L.tnetF_apply_log(Y.ptr, Y.dim, S()))
            check(L.tnet_memcpy_d2d(T.ptr, Y.ptr, rows * Y.stride * 4))

        def fused_to_host():
            fused()
            check(L.tnet_memcpy_d2h(host_dense.ctypes.data, dense.ptr, host_dense.nbytes))

        def replaced_to_host():
            replaced()
            check(L.tnet_memcpy_d2h(host_pad.ctypes.data, T.ptr, host_pad.nbytes))
            return host_pad[:, :cols].astype(">f4")

        def host_us(fn, reps):
            tnet_amd.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            return 1e6 * (time.perf_counter() - t0) / reps

        for fn in (fused, replaced):
            timed(fn, 20)
        fused_to_host(), replaced_to_host()
        # the two agree: the fused words are the replaced job's, within the log's last place
        a = host_dense.byteswap().view(np.float32).reshape(rows, cols)
        b = replaced_to_host().astype(np.float32)
        assert np.allclose(a, b, rtol=1e-5, atol=1e-5), "fused and replaced outputs differ"
        t = {"fused": [], "replaced": [], "fused_to_host": [], "replaced_to_host": []}
        reps = max(5, iters // 20)
        for _ in range(rounds):
            t["fused"].append(timed(fused, iters))
            t["replaced"].append(timed(replaced, iters))
            t["fused_to_host"].append(host_us(fused_to_host, reps))
            t["replaced_to_host"].append(host_us(replaced_to_host, reps))
        rec = {"rows": rows, "cols": cols, "stride": Y.stride, "read_bytes": 4 * rows * cols,
               "written_bytes": 4 * rows * cols}
        for k, v in t.items():
            rec[k + "_us"] = _stat(v)
        rec["kernels_replaced_over_fused"] = round(rec["replaced_us"]["median"] / rec["fused_us"]["median"], 3)
        rec["to_host_replaced_over_fused"] = round(rec["replaced_to_host_us"]["median"] /
                                                   rec["fused_to_host_us"]["median"], 3)
        rec["fused_gbytes_per_s"] = round(8.0 * rows * cols / rec["fused_us"]["median"] / 1e3, 1)
        print(json.dumps(rec), flush=True)
        results.append(rec)
        tnet_amd.synchronize()
    return results


def _passes(net, transform, corpus, ext, outdir, logp):
    """the variants as callables: each runs the whole pass over `corpus` (host arrays incl. the context rows)"""
    names = [f"u{k:04d}" for k in range(len(corpus))]

    def forwarder(pack_rows, files=True):
        def run():
            fwd = Forwarder(net, transform, start_ext=ext, end_ext=ext, log_posterior=logp, pack_rows=pack_rows)
            if files:
                fwd.set_output(outdir, "fea")
            for name, x in zip(names, corpus):
                fwd.add(x, name=name)
            fwd.finish()
            return fwd.stats()
        return run

    def host():
        for name, x in zip(names, corpus):
            d = DeviceArray.from_numpy(x)
            if transform is not None:
                d = transform.propagate(d)
            y = net.propagate(d).numpy()[ext:x.shape[0] - ext]
            if logp:
                with np.errstate(all="ignore"):
                    y = np.log(y.astype(np.float64)).astype(np.float32)
            formats.write_htk(os.path.join(outdir, name + ".fea"), y, 100000, formats.HTK_USER)
        return None

    return forwarder, host


def _rate(fn, frames):
    tnet_amd.synchronize()
    t0 = time.perf_counter()
    fn()
    tnet_amd.synchronize()
    return frames / (time.perf_counter() - t0)


def pass_bench(name, net, transform, corpus, ext, rounds, sweep, logp=True):
    frames = sum(x.shape[0] - 2 * ext for x in corpus)
    n_out = net.n_out
    res = {"name": name, "utterances": len(corpus), "frames": frames, "n_out": n_out, "ext": ext,
           "mode": "LOGPOSTERIOR" if logp else "none",
           "output_bytes_per_pass": 4 * n_out * frames}
    with tempfile.TemporaryDirectory() as outdir:
        forwarder, host = _passes(net, transform, corpus, ext, outdir, logp)
        variants = {"packed": forwarder(None), "unpacked": forwarder(-1), "host": host,
                    "memory": forwarder(None, files=False)}
        for fn in variants.values():  # warm-up: allocations, code objects, the page cache of the output files
            fn()
        # the variants write the same files: compare the first and the longest utterance of packed and host
        order = np.argsort([x.shape[0] for x in corpus])
        check_utts = (0, int(order[-1]))
        variants["host"]()
        a = [formats.read_htk(os.path.join(outdir, f"u{k:04d}.fea")) for k in check_utts]
        variants["packed"]()
        b = [formats.read_htk(os.path.join(outdir, f"u{k:04d}.fea")) for k in check_utts]
        for x, y in zip(a, b):
            assert x.shape == y.shape and np.allclose(x, y, rtol=1e-3, atol=1e-3), "packed and host passes differ"
        t = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():
                t[k].append(_rate(fn, frames))
        for k, v in t.items():
            res[k] = {"frames_per_s": round(float(np.median(v))), "min_max": [round(min(v)), round(max(v))]}
        res["packed_stats"] = variants["packed"]()
        res["unpacked_stats"] = variants["unpacked"]()
        for a, b in (("packed", "unpacked"), ("packed", "host"), ("memory", "packed")):
            res[f"{a}_over_{b}"] = round(res[a]["frames_per_s"] / res[b]["frames_per_s"], 3)
        res["packed_file_gbytes_per_s"] = round(res["packed"]["frames_per_s"] * 4e-9 * n_out, 3)
        res["memory_d2h_gbytes_per_s"] = round(res["memory"]["frames_per_s"] * 4e-9 * n_out, 3)
        if sweep:
            sw = {}
            fns = {p: forwarder(p) for p in SWEEP}
            for fn in fns.values():
                fn()
            ts = {p: [] for p in SWEEP}
            for _ in range(rounds):
                for p, fn in fns.items():
                    ts[p].append(_rate(fn, frames))
            for p, v in ts.items():
                sw[str(p)] = {"frames_per_s": round(float(np.median(v))), "min_max": [round(min(v)), round(max(v))]}
            res["pack_rows_sweep"] = sw
    print(json.dumps(res), flush=True)
    return res


def ex01_case():
    c = formats.read_corpus(os.path.join(EX, "test.scp"), os.path.join(EX, "test_3s.mlf"),
                            os.path.join(EX, "mono_state_phn_set_135_phn"))
    corpus = [formats.extend_frames(x, 25, 25) for x in c.feats]
    transform = Network(path=os.path.join(EX, "Hamm_dct_norm"))
    net = Network.from_layers(formats.gen_mlp_init([598, 1024, 135], seed=1), precision=6)
    return net, transform, corpus, 25


def seeded_net(dims, softmax, rng):
    """(<biasedlinearity> <sigmoid>)* <biasedlinearity> [<softmax>] with seeded weights: the text carries zeros (21 M
    formatted floats would take longer than the measurement), the weights go in through set_params"""
    parts = []
    for li, (n_in, n_out) in enumerate(zip(dims[:-1], dims[1:])):
        last = li == len(dims) - 2
        parts.append(f"<biasedlinearity> {n_out} {n_in}\nm {n_out} {n_in}\n" + ("0 " * n_in + "\n") * n_out +
                     f"v {n_out}  " + "0 " * n_out + "\n\n")
        if not last or softmax:
            parts.append(f"{'<softmax>' if last else '<sigmoid>'} {n_out} {n_out}\n")
    net = Network(text="".join(parts))
    for i, (tag, n_in, n_out) in enumerate(net.components()):
        if tag == "<biasedlinearity>":
            net.set_params(i, (0.1 * rng.standard_normal((n_in, n_out))).astype(np.float32),
                           (-2.0 * rng.random(n_out)).astype(np.float32))
    return net


def synthetic_case(dims, softmax, utts=24, ext=15, seed=0):
    rng = np.random.default_rng(seed)
    net = seeded_net(dims, softmax, rng)  # without a softmax: a bottleneck stage ends in its linearity
    corpus = [rng.standard_normal((int(n) + 2 * ext, dims[0])).astype(np.float32)
              for n in rng.integers(200, 1501, utts)]
    return net, None, corpus, ext


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "feacat.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--utts", type=int, default=24, help="synthetic utterances per case")
    ap.add_argument("--repeat", type=int, default=4, help="every corpus this many times over in one pass")
    ap.add_argument("--cases", default="kernel,ex01,4000,bottleneck", help="comma-separated subset to run")
    a = ap.parse_args()
    cases = set(a.cases.split(","))
    doc = {"what": "tnet_softmax_emit (LOGPOSTERIOR, big-endian) vs tnetF_softmax + tnetF_apply_log + a device copy of "
                   "the rows: device-event us per call, median of `rounds` alternating windows of `iters` calls "
                   "(min / max beside it); *_to_host_us: host clock, each side ending in its synchronous copy (dense "
                   "rows x C words; padded rows x stride + a numpy byte swap).  passes: frames/s from host memory to "
                   "written files, host clock around a pass ending in finish(), variants alternating, median of "
                   "`rounds`; memory: the packed pass with the results kept in memory",
           "iters": a.iters, "rounds": a.rounds, "version": lib().tnet_version().decode(),
           "default_pack_rows": 4096}
    doc["repeat"], doc["passes"] = a.repeat, []
    if "kernel" in cases:
        doc["kernel"] = kernel_bench(a.iters, a.rounds)
    if "ex01" in cases:
        net, tr, corpus, ext = ex01_case()
        doc["passes"].append(pass_bench("examples/01 598:1024:135 + Hamm_dct_norm", net, tr, corpus * a.repeat, ext,
                                        a.rounds, True))
    if "4000" in cases:
        net, tr, corpus, ext = synthetic_case([440, 2048, 2048, 2048, 2048, 4000], True, a.utts)
        doc["passes"].append(pass_bench("440:2048x4:4000", net, tr, corpus * a.repeat, ext, a.rounds, True))
    if "bottleneck" in cases:
        net, tr, corpus, ext = synthetic_case([440, 2048, 2048, 40], False, a.utts)
        doc["passes"].append(pass_bench("440:2048x2:40 bottleneck (linear output)", net, tr, corpus * a.repeat, ext,
                                        a.rounds, False, logp=False))
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
