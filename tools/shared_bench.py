#!/usr/bin/env python3
"""<sharedlinearity> kernels: the instance-batched entry points (tnet_shared_fwd / _bwd / _update, one launch per
direction over all N instances) next to the straightforward port of cuSharedLinearity.cc built only from entry
points the library had before them:

  forward   tnetF_add_scaled_row (the expanded bias, built once outside the timed window) + N tnet_sgemm('N','N',
            beta 1) on column windows
  backward  N tnet_sgemm('N','T', beta 0) on column windows
  update    N tnet_sgemm('T','N', beta = momentum for the first, 1 after) into the correction buffer,
            tnetF_add_col_sum over E and over the [N x out] view of that sum, and tnet_sgd_update for W and b

tnet_sgemm needs 16-byte aligned operands, so where `in` is no multiple of 4 (39) the loop first gathers X into a
layout with every window padded to a multiple of 4 columns (tnetF_rearrange, one launch) and, backward, scatters
the padded result back the same way; both launches are inside the loop's timed window.

Timing: device events around `iters` back-to-back calls on the library stream, after a warm-up of both variants;
the two variants alternate for `rounds` rounds and the median, minimum and maximum per-call time of each are
reported, so the spread of a variant is visible beside the difference between the two.  FLOP = 2 * rows * N * in *
out per direction; the fraction is of the 157.3 TFLOP/s dense fp32 MFMA peak.

usage: python tools/shared_bench.py [--out profiles/shared_linearity.json] [--iters 200] [--rounds 7]"""
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
from tnet_amd._lib import MatrixDim, check, lib  # noqa: E402

PEAK = 157.3
SHAPES = [(1024, 5, 440, 1024), (1024, 5, 1024, 80), (256, 11, 39, 128)]  # (bunch, N, in, out)


def S():
    return lib().tnet_stream()


def timed(fn, iters):
    check(lib().tnet_timer_start())
    for _ in range(iters):
        fn()
    ms = C.c_float()
    check(lib().tnet_timer_stop(C.byref(ms)))
    return 1e3 * ms.value / iters  # us per call


def off(d, cols):
    return d.ptr + 4 * cols


def build(rows, n, n_in, n_out):
    rng = np.random.default_rng(0)
    f = lambda *s, scale=1.0: (rng.standard_normal(s) * scale).astype(np.float32)  # noqa: E731
    X, E = DeviceArray.from_numpy(f(rows, n * n_in)), DeviceArray.from_numpy(f(rows, n * n_out, scale=0.01))
    W, Cw = DeviceArray.from_numpy(f(n_in, n_out, scale=0.1)), DeviceArray(n_in, n_out)
    W2, Cw2 = DeviceArray.from_numpy(W.numpy()), DeviceArray(n_in, n_out)
    b, cb, b2, cb2 = (DeviceArray.vector(f(n_out)) for _ in range(4))
    Y, Eo = DeviceArray(rows, n * n_out), DeviceArray(rows, n * n_in)
    scale, mmt, l2 = -1e-6, 0.5, -1e-6
    L = lib()

    def new_fwd():
        check(L.tnet_shared_fwd(X.ptr, X.dim, W.ptr, W.dim, b.ptr, n, Y.ptr, Y.dim, S()))

    def new_bwd():
        check(L.tnet_shared_bwd(E.ptr, E.dim, W.ptr, W.dim, n, Eo.ptr, Eo.dim, S()))

    def new_upd():
        check(L.tnet_shared_update(X.ptr, X.dim, E.ptr, E.dim, n, W.ptr, W.dim, Cw.ptr, Cw.stride, b.ptr, cb.ptr,
                                   scale, mmt, l2, S()))

    # ---- the per-instance loop
    pin = (n_in + 3) & ~3  # window pitch of the padded copy of X / Eo (== n_in where the windows are aligned)
    padded = pin != n_in
    Xp = Eop = to_pad = from_pad = None
    if padded:
        Xp, Eop = DeviceArray(rows, n * pin), DeviceArray(rows, n * pin)
        idx = np.concatenate([np.minimum(np.arange(pin), n_in - 1) + i * n_in for i in range(n)]).astype(np.int32)
        to_pad = DeviceArray.vector(idx)
        from_pad = DeviceArray.vector(np.concatenate([np.arange(n_in) + i * pin for i in range(n)]).astype(np.int32))
    bexp = DeviceArray.vector(np.tile(b.numpy().reshape(-1), n))
    bsum = DeviceArray(1, n * n_out, stride=n * n_out)
    ws = DeviceArray(1, max(L.tnet_col_sum_workspace(E.dim) // 4, 4))
    dsum = MatrixDim(n, n_out, n_out)

    def x_windows():
        if padded:
            check(L.tnetF_rearrange(Xp.ptr, X.ptr, to_pad.ptr, Xp.dim, X.dim, S()))
            return Xp, pin
        return X, n_in

    def loop_fwd():
        Xs, pitch = x_windows()
        check(L.tnetF_add_scaled_row(1.0, bexp.ptr, 0.0, Y.ptr, Y.dim, S()))
        for i in range(n):
            check(L.tnet_sgemm(b"N", b"N", rows, n_out, n_in, 1.0, off(Xs, i * pitch), Xs.stride, W2.ptr, W2.stride,
                               1.0, off(Y, i * n_out), Y.stride, S()))

    def loop_bwd():
        dst = Eop if padded else Eo
        for i in range(n):
            check(L.tnet_sgemm(b"N", b"T", rows, n_in, n_out, 1.0, off(E, i * n_out), E.stride, W2.ptr, W2.stride, 0.0,
                               off(dst, i * pin), dst.stride, S()))
        if padded:
            check(L.tnetF_rearrange(Eo.ptr, Eop.ptr, from_pad.ptr, Eo.dim, Eop.dim, S()))

    def loop_upd():
        Xs, pitch = x_windows()
        for i in range(n):
            check(L.tnet_sgemm(b"T", b"N", n_in, n_out, rows, 1.0, off(Xs, i * pitch), Xs.stride, off(E, i * n_out),
                               E.stride, mmt if i == 0 else 1.0, Cw2.ptr, Cw2.stride, S()))
        check(L.tnetF_add_col_sum(1.0, E.ptr, 0.0, bsum.ptr, E.dim, ws.ptr, S()))
        check(L.tnetF_add_col_sum(1.0, bsum.ptr, mmt, cb2.ptr, dsum, ws.ptr, S()))
        check(L.tnet_sgd_update(W2.ptr, Cw2.ptr, None, n_in * W2.stride, scale, 0.0, l2, S()))
        check(L.tnet_sgd_update(b2.ptr, cb2.ptr, None, n_out, scale, 0.0, 0.0, S()))

    keep = (X, E, W, Cw, W2, Cw2, b, cb, b2, cb2, Y, Eo, Xp, Eop, to_pad, from_pad, bexp, bsum, ws)
    return {"fwd": (new_fwd, loop_fwd), "bwd": (new_bwd, loop_bwd), "update": (new_upd, loop_upd)}, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shared_linearity.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    results = []
    for rows, n, n_in, n_out in SHAPES:
        variants, keep = build(rows, n, n_in, n_out)
        flop = 2.0 * rows * n * n_in * n_out
        for direction, (new, loop) in variants.items():
            for fn in (new, loop):  # warm-up: code objects, workspaces, clocks
                timed(fn, 20)
            t_new, t_loop = [], []
            for _ in range(a.rounds):
                t_new.append(timed(new, a.iters))
                t_loop.append(timed(loop, a.iters))
            med_new, med_loop = float(np.median(t_new)), float(np.median(t_loop))
            rec = {"bunch": rows, "n_inst": n, "in": n_in, "out": n_out, "direction": direction,
                   "batched_us": round(med_new, 2), "batched_us_min_max": [round(min(t_new), 2), round(max(t_new), 2)],
                   "loop_us": round(med_loop, 2), "loop_us_min_max": [round(min(t_loop), 2), round(max(t_loop), 2)],
                   "speedup": round(med_loop / med_new, 3),
                   "batched_tflops": round(flop / med_new / 1e6, 2),
                   "batched_frac_of_fp32_mfma_peak": round(flop / med_new / 1e6 / PEAK, 4),
                   "loop_tflops": round(flop / med_loop / 1e6, 2),
                   "loop_frac_of_fp32_mfma_peak": round(flop / med_loop / 1e6 / PEAK, 4)}
            print(json.dumps(rec), flush=True)
            results.append(rec)
        tnet_amd.synchronize()
        del variants, keep
    doc = {"what": "tnet_shared_fwd / _bwd / _update (one launch per direction over all instances) vs the "
                   "per-instance loop built from tnet_sgemm / tnetF_add_scaled_row / tnetF_add_col_sum / "
                   "tnet_sgd_update; device-event time per call in us, median of `rounds` alternating windows of "
                   "`iters` calls each (min / max beside it); FLOP = 2 * bunch * N * in * out",
           "peak_tflops_fp32_mfma": PEAK, "iters": a.iters, "rounds": a.rounds, "version": lib().tnet_version().decode(),
           "results": results}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
