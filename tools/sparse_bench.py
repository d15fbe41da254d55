#!/usr/bin/env python3
"""<sparselinearity> update: tnet_sparse_update in both forms (the single launch whose GEMM epilogue applies the
update, and the sliced form: K slices + a combine launch), each at both tile sizes, next to the straightforward port
of CuSparseLinearity::Update (cuSparseLinearity.cc:28-63) built only from entry points the library had before it:

  tnet_affine_update (corrW = X^T E + mmt*corrW ; W += scale*corrW, l2 0), tnetF_add_scaled (accu += corrW),
  tnetF_apply_mask (a float mask), tnetF_apply_l1, tnetF_add_scaled (W += l2*W), tnet_bias_update

"entry" is tnet_sparse_update as it ships (form 0: the automatic choice); the forced variants go through
tnet_sparse_update_form.

Timing: device events around `iters` back-to-back calls on the library stream, after a warm-up of every variant; the
variants alternate for `rounds` rounds and the median, minimum and maximum per-call time of each are reported, so
the spread of a variant is visible beside the differences between them.  FLOP = 2 * bunch * n_in * n_out; the
fraction is of the 157.3 TFLOP/s dense fp32 MFMA peak.  `min_bytes` is what one update has to move at least: X and E
once, W, corrW and accu read and written once, the bit mask once.

usage: python tools/sparse_bench.py [--out profiles/sparse_linearity.json] [--iters 200] [--rounds 7]"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nnet-asr_amd"))
import numpy as np  # noqa: E402

import tnet_amd  # noqa: E402
from tnet_amd import DeviceArray  # noqa: E402
from tnet_amd._lib import check, lib  # noqa: E402

PEAK = 157.3
# (1024x2048: 512 tiles of 64x64, between the 224 of 440x2048 and the 1024 of 2048x2048 -- it places the threshold
# between the two forms)
LAYERS = [(2048, 2048), (1024, 2048), (440, 2048), (1024, 135)]
BUNCHES = [1024, 256]
DENSITIES = [1.0, 0.1]
# name -> tnet_sparse_update_form argument (| 0x20: 128x128 tiles instead of 64x64)
FORMS = {"single64": 0x01, "single128": 0x21, "sliced64": 0x02, "sliced128": 0x22, "entry": 0}


def S():
    return lib().tnet_stream()


def timed(fn, iters):
    check(lib().tnet_timer_start())
    for _ in range(iters):
        fn()
    ms = C.c_float()
    check(lib().tnet_timer_stop(C.byref(ms)))
    return 1e3 * ms.value / iters  # us per call


def build(rows, n_in, n_out, density):
    rng = np.random.default_rng(0)
    f = lambda *s, scale=1.0: (rng.standard_normal(s) * scale).astype(np.float32)  # noqa: E731
    L = lib()
    mask = (rng.random((n_in, n_out)) < density).astype(np.float32)
    X, E = DeviceArray.from_numpy(f(rows, n_in)), DeviceArray.from_numpy(f(rows, n_out, scale=0.01))
    W0 = f(n_in, n_out, scale=0.1) * mask
    scale, mmt, l1c, l2 = -1e-6, 0.5, 1e-7, -1e-6
    # ---- the fused entry point
    W, Cw, A = DeviceArray.from_numpy(W0), DeviceArray(n_in, n_out), DeviceArray(n_in, n_out)
    b, cb, b2, cb2 = (DeviceArray.vector(f(n_out)) for _ in range(4))
    Mf = DeviceArray.from_numpy(mask)
    ldmask = (n_out + 31) // 32
    bits = DeviceArray(n_in, ldmask, np.uint32, stride=ldmask)
    check(L.tnet_sparse_mask_pack(Mf.ptr, Mf.dim, bits.ptr, ldmask, S()))

    def fused():
        check(L.tnet_sparse_update(X.ptr, X.dim, E.ptr, E.dim, W.ptr, W.dim, Cw.ptr, Cw.stride, A.ptr, A.stride,
                                   bits.ptr, ldmask, b.ptr, cb.ptr, scale, mmt, l1c, l2, S()))

    # ---- the chain of the library's older entry points, on buffers of its own
    W2, C2, A2 = DeviceArray.from_numpy(W0), DeviceArray(n_in, n_out), DeviceArray(n_in, n_out)
    ws = DeviceArray(1, max(L.tnet_col_sum_workspace(E.dim) // 4, 4))

    def chain():
        check(L.tnet_affine_update(X.ptr, X.dim, E.ptr, E.dim, W2.ptr, W2.dim, C2.ptr, C2.stride, scale, mmt, 0.0, S()))
        check(L.tnetF_add_scaled(1.0, C2.ptr, C2.stride, 1.0, A2.ptr, A2.dim, S()))
        check(L.tnetF_apply_mask(W2.ptr, Mf.ptr, W2.dim, Mf.dim, S()))
        check(L.tnetF_apply_l1(W2.ptr, l1c, W2.dim, S()))
        check(L.tnetF_add_scaled(l2, W2.ptr, W2.stride, 1.0, W2.ptr, W2.dim, S()))
        check(L.tnet_bias_update(E.ptr, E.dim, b2.ptr, cb2.ptr, None, scale, mmt, ws.ptr, S()))

    keep = (X, E, W, Cw, A, b, cb, b2, cb2, Mf, bits, W2, C2, A2, ws)
    return fused, chain, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sparse_linearity.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    L = lib()
    results = []
    for n_in, n_out in LAYERS:
        for rows in BUNCHES:
            for density in DENSITIES:
                fused, chain, keep = build(rows, n_in, n_out, density)
                names = list(FORMS) + ["chain"]

                def run(name, iters):
                    if name == "chain":
                        return timed(chain, iters)
                    was = L.tnet_sparse_update_form(FORMS[name])
                    try:
                        return timed(fused, iters)
                    finally:
                        L.tnet_sparse_update_form(was)

                for name in names:  # warm-up: code objects, workspaces, clocks
                    run(name, 20)
                t = {name: [] for name in names}
                for _ in range(a.rounds):
                    for name in names:
                        t[name].append(run(name, a.iters))
                flop = 2.0 * rows * n_in * n_out
                min_bytes = 4.0 * (rows * (n_in + n_out) + 6 * n_in * n_out) + n_in * n_out / 8.0
                rec = {"layer": f"{n_in}x{n_out}", "bunch": rows, "density": density, "min_bytes": int(min_bytes)}
                for name in names:
                    med = float(np.median(t[name]))
                    rec[name + "_us"] = round(med, 2)
                    rec[name + "_us_min_max"] = [round(min(t[name]), 2), round(max(t[name]), 2)]
                med_chain = rec["chain_us"]
                for name in FORMS:
                    rec[name + "_speedup_vs_chain"] = round(med_chain / rec[name + "_us"], 3)
                rec["entry_tflops"] = round(flop / rec["entry_us"] / 1e6, 2)
                rec["entry_frac_of_fp32_mfma_peak"] = round(flop / rec["entry_us"] / 1e6 / PEAK, 4)
                rec["entry_gbytes_per_s_of_min_bytes"] = round(min_bytes / rec["entry_us"] / 1e3, 1)
                print(json.dumps(rec), flush=True)
                results.append(rec)
                tnet_amd.synchronize()
                del fused, chain, keep
    doc = {"what": "tnet_sparse_update (single launch with the update in the GEMM epilogue / K slices + combine "
                   "launch, 64x64 and 128x128 tiles, and the entry point's automatic choice) vs the chain "
                   "tnet_affine_update + tnetF_add_scaled + tnetF_apply_mask + tnetF_apply_l1 + tnetF_add_scaled + "
                   "tnet_bias_update; device-event time per call in us, median of `rounds` alternating windows of "
                   "`iters` calls each (min / max beside it); FLOP = 2 * bunch * n_in * n_out",
           "peak_tflops_fp32_mfma": PEAK, "iters": a.iters, "rounds": a.rounds,
           "version": L.tnet_version().decode(), "results": results}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
