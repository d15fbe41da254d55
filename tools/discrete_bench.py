#!/usr/bin/env python3
"""<discretelinearity> kernels: the grouped entry points (tnet_discrete_fwd / _bwd / _update, one launch per
direction over all blocks) next to the straightforward port of cuDiscreteLinearity.cc built only from entry points
the library had before them:

  forward   tnetF_add_scaled_row (the bias) + one tnet_sgemm('N','N', beta 1) per block on its column stripes
  backward  one tnet_sgemm('N','T', beta 0) per block
  update    one tnet_sgemm('T','N', beta = momentum) per block into its correction buffer and one tnet_sgd_update
            per block, tnetF_add_col_sum over E (beta = momentum) and tnet_sgd_update for the bias

tnet_sgemm needs 16-byte aligned operands, so where a stripe origin is off 16 bytes (in_k = 39) the loop first
gathers X into a layout with every stripe padded to a multiple of 4 columns (tnetF_rearrange, one launch) and,
backward, scatters the padded result back the same way; both launches are inside the loop's timed window.

Where tnet_discrete_bwd routes a shape to its own per-block loop (gemm_discrete.hip loop_class), the table's
"grouped" column is still the grouped launch, measured with the routing switched off
(tnet_discrete_loop_routing(0)), and "entry_us" is the entry point as it ships.

Timing: device events around `iters` back-to-back calls on the library stream, after a warm-up of both variants;
the two variants alternate for `rounds` rounds and the median, minimum and maximum per-call time of each are
reported, so the spread of a variant is visible beside the difference between the two.  FLOP = 2 * rows *
sum(in_k * out_k) per direction; the fraction is of the 157.3 TFLOP/s dense fp32 MFMA peak.

usage: python tools/discrete_bench.py [--out profiles/discrete_linearity.json] [--iters 200] [--rounds 7]"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nnet-asr_amd"))
import numpy as np  # noqa: E402

import tnet_amd  # noqa: E402
from tnet_amd import DeviceArray, DiscretePlan  # noqa: E402
from tnet_amd._lib import check, lib  # noqa: E402

PEAK = 157.3
LAYERS = {"23x(16->32)": [(16, 32)] * 23,
          "ragged(39,120,281)->(64,256,704)": [(39, 64), (120, 256), (281, 704)],
          "4x(512->512)": [(512, 512)] * 4}
BUNCHES = [1024, 256]


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


def build(rows, blocks):
    rng = np.random.default_rng(0)
    f = lambda *s, scale=1.0: (rng.standard_normal(s) * scale).astype(np.float32)  # noqa: E731
    nb = len(blocks)
    ins, outs = [b[0] for b in blocks], [b[1] for b in blocks]
    n_in, n_out = sum(ins), sum(outs)
    io, oo = np.concatenate([[0], np.cumsum(ins)]), np.concatenate([[0], np.cumsum(outs)])
    plan = DiscretePlan(blocks)
    X, E = DeviceArray.from_numpy(f(rows, n_in)), DeviceArray.from_numpy(f(rows, n_out, scale=0.01))
    Ws = [f(a, b, scale=0.1) for a, b in blocks]
    Wp, Cp = DeviceArray.vector(plan.pack(Ws)), DeviceArray.vector(np.zeros(plan.floats, np.float32))
    b, cb, b2, cb2 = (DeviceArray.vector(f(n_out)) for _ in range(4))
    Y, Eo = DeviceArray(rows, n_out), DeviceArray(rows, n_in)
    scale, mmt, l2 = -1e-6, 0.5, -1e-6
    L = lib()

    def new_fwd():
        check(L.tnet_discrete_fwd(X.ptr, X.dim, Wp.ptr, plan.ptr, b.ptr, Y.ptr, Y.dim, S()))

    def new_bwd():
        check(L.tnet_discrete_bwd(E.ptr, E.dim, Wp.ptr, plan.ptr, Eo.ptr, Eo.dim, S()))

    def new_upd():
        check(L.tnet_discrete_update(X.ptr, X.dim, E.ptr, E.dim, plan.ptr, Wp.ptr, Cp.ptr, b.ptr, cb.ptr, scale, mmt,
                                     l2, S()))

    # ---- the per-block loop: one matrix and one correction buffer per block
    W2 = [DeviceArray.from_numpy(W) for W in Ws]
    C2 = [DeviceArray(a, b_) for a, b_ in blocks]
    # stripes of X / Eo: where an origin is off 16 bytes, a copy with every stripe padded to a multiple of 4 columns
    pins = [(a + 3) & ~3 for a in ins]
    pio = np.concatenate([[0], np.cumsum(pins)])
    padded = any(int(o) & 3 for o in io[:-1])
    Xp = Eop = to_pad = from_pad = None
    if padded:
        Xp, Eop = DeviceArray(rows, int(pio[-1])), DeviceArray(rows, int(pio[-1]))
        idx = np.concatenate([np.minimum(np.arange(p), a - 1) + o for p, a, o in zip(pins, ins, io[:-1])])
        to_pad = DeviceArray.vector(idx.astype(np.int32))
        idx = np.concatenate([np.arange(a) + o for a, o in zip(ins, pio[:-1])])
        from_pad = DeviceArray.vector(idx.astype(np.int32))
    if any(int(o) & 3 for o in oo[:-1]):
        raise SystemExit("the loop baseline handles unaligned input stripes only")
    ws = DeviceArray(1, max(L.tnet_col_sum_workspace(E.dim) // 4, 4))

    def x_stripes():
        if padded:
            check(L.tnetF_rearrange(Xp.ptr, X.ptr, to_pad.ptr, Xp.dim, X.dim, S()))
            return Xp, pio
        return X, io

    def loop_fwd():
        Xs, xo = x_stripes()
        check(L.tnetF_add_scaled_row(1.0, b2.ptr, 0.0, Y.ptr, Y.dim, S()))
        for k in range(nb):
            check(L.tnet_sgemm(b"N", b"N", rows, outs[k], ins[k], 1.0, off(Xs, int(xo[k])), Xs.stride, W2[k].ptr,
                               W2[k].stride, 1.0, off(Y, int(oo[k])), Y.stride, S()))

    def loop_bwd():
        dst, do = (Eop, pio) if padded else (Eo, io)
        for k in range(nb):
            check(L.tnet_sgemm(b"N", b"T", rows, ins[k], outs[k], 1.0, off(E, int(oo[k])), E.stride, W2[k].ptr,
                               W2[k].stride, 0.0, off(dst, int(do[k])), dst.stride, S()))
        if padded:
            check(L.tnetF_rearrange(Eo.ptr, Eop.ptr, from_pad.ptr, Eo.dim, Eop.dim, S()))

    def loop_upd():
        Xs, xo = x_stripes()
        for k in range(nb):
            check(L.tnet_sgemm(b"T", b"N", ins[k], outs[k], rows, 1.0, off(Xs, int(xo[k])), Xs.stride,
                               off(E, int(oo[k])), E.stride, mmt, C2[k].ptr, C2[k].stride, S()))
        for k in range(nb):
            check(L.tnet_sgd_update(W2[k].ptr, C2[k].ptr, None, ins[k] * W2[k].stride, scale, 0.0, l2, S()))
        check(L.tnetF_add_col_sum(1.0, E.ptr, mmt, cb2.ptr, E.dim, ws.ptr, S()))
        check(L.tnet_sgd_update(b2.ptr, cb2.ptr, None, n_out, scale, 0.0, 0.0, S()))

    keep = (plan, X, E, Wp, Cp, b, cb, b2, cb2, Y, Eo, W2, C2, Xp, Eop, to_pad, from_pad, ws)
    return {"fwd": (new_fwd, loop_fwd), "bwd": (new_bwd, loop_bwd), "update": (new_upd, loop_upd)}, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "discrete_linearity.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    results = []
    for name, blocks in LAYERS.items():
        for rows in BUNCHES:
            variants, keep = build(rows, blocks)
            flop = 2.0 * rows * sum(i * o for i, o in blocks)
            for direction, (new, loop) in variants.items():
                for fn in (new, loop):  # warm-up: code objects, workspaces, clocks
                    timed(fn, 20)
                t_new, t_loop, t_entry = [], [], []
                for _ in range(a.rounds):
                    lib().tnet_discrete_loop_routing(0)
                    t_new.append(timed(new, a.iters))
                    lib().tnet_discrete_loop_routing(1)
                    t_loop.append(timed(loop, a.iters))
                    t_entry.append(timed(new, a.iters))
                med_new, med_loop = float(np.median(t_new)), float(np.median(t_loop))
                med_entry = float(np.median(t_entry))
                rec = {"layer": name, "bunch": rows, "blocks": len(blocks), "direction": direction,
                       "grouped_us": round(med_new, 2),
                       "grouped_us_min_max": [round(min(t_new), 2), round(max(t_new), 2)],
                       "loop_us": round(med_loop, 2), "loop_us_min_max": [round(min(t_loop), 2), round(max(t_loop), 2)],
                       "speedup": round(med_loop / med_new, 3),
                       "entry_us": round(med_entry, 2),
                       "entry_us_min_max": [round(min(t_entry), 2), round(max(t_entry), 2)],
                       "entry_speedup": round(med_loop / med_entry, 3),
                       "grouped_tflops": round(flop / med_new / 1e6, 2),
                       "grouped_frac_of_fp32_mfma_peak": round(flop / med_new / 1e6 / PEAK, 4),
                       "loop_tflops": round(flop / med_loop / 1e6, 2),
                       "loop_frac_of_fp32_mfma_peak": round(flop / med_loop / 1e6 / PEAK, 4)}
                print(json.dumps(rec), flush=True)
                results.append(rec)
            tnet_amd.synchronize()
            del variants, keep
    doc = {"what": "tnet_discrete_fwd / _bwd / _update (one grouped launch per direction over all blocks) vs "
                   " the per-block loop built from tnet_sgemm / tnetF_add_scaled_row / "
                   "tnetF_add_col_sum / tnet_sgd_update; device-event time per call in us, median of `rounds` "
                   "alternating windows of `iters` calls each (min / max beside it); FLOP = 2 * bunch * "
                   "sum(in_k * out_k)",
           "routing": "tnet_discrete_bwd runs its own per-block loop (tnet_sgemm per block into a 4-column-padded "
                      "copy of Eo in the kept workspace + one tnetF_rearrange; directly into Eo where the stripes are "
                      "aligned) where bunch >= 512, the grouped 64-tile grid has fewer than 256 workgroups, the "
                      "deepest out_k is at least 200 per block and the E stripes are 16-byte aligned; grouped_us is "
                      "the grouped launch with that routing off, entry_us the entry point as it ships",
           "peak_tflops_fp32_mfma": PEAK, "iters": a.iters, "rounds": a.rounds,
           "version": lib().tnet_version().decode(), "results": results}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
