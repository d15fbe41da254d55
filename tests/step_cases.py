"""Cases shared by tests/test_gpu_step_branches.py, tests/step_modes_worker.py and tests/test_step_cases_cpu.py: one
sigmoid MLP per branch of the fused SGD step's scheduler (CuNetwork::TrainBunch, csrc/host/cunetwork.cpp:376-749),
its SGD constants, its bunches, the float64 restatement of its steps (stack_cases.Oracle: nothing is restated here a
second time) and, per step, the multiset of launch tags the scheduler must report through tnet_kernel_timing_report.
numpy only: nothing here touches the GPU.

The tags are written down by hand from the gate expressions quoted beside each case (G.* below); no code here mirrors
the library's planner.  `transpose:KxN` (CuBiasedLinearity::ShadowForBwd rebuilding a stale transposed shadow) is no
scheduling decision of the step and is left out of the comparison (IGNORED_TAGS); every other tag counts.  A count is
the number of GEMMs, not of launches: a two-GEMM launch reports 2 under its one tag (KTScope's count, culayers.cpp:213,
248, 285: `other ? 2 : 1`).

The gates (csrc/kernels/gemm_f32.hip unless another file is named; tiles are ceil-divided; the MI355X has 256 CUs)
  G.fused-top   cunetwork.cpp:456   last && fuse_top && !block_top && n_out <= TNET_AFFINE_SOFTMAX_MAX_N (256)
                :3033               tnet_affine_softmax_xent declines dW.cols > kSxMaxN
  G.ride        cunetwork.cpp:521-526  top_colsum && !fused_top: top_bwd = nl > 1 && top != stopper && the layer below
                                    is trained; slabs_ride && top_bwd: the slab sums ride on the top backward, else a
                                    `colsum:N` launch of their own
                :3276               bwd_colsum_slabs declines ceil(rows/64) * ceil(n_in/128) < 200: then
                                    cunetwork.cpp:607 launches `colsum:N` inside the `gemm_bwd` scope
  G.bwd-colsum  cunetwork.cpp:583   the backward of layer l writes column sums iff layer l-1 is trained; :625 else the
                                    plain tnet_affine_bwd.  Both report `gemm_bwd:KxN`
  G.stopper     cunetwork.cpp:576   no backward for the stopper or layer 0
  G.upd+bwd     cunetwork.cpp:590, culayers.cpp:213; launch_pair_a_bwd :2849-2864: g_pair, the update planned
                                    m128x128k64s2 unsplit (plan_gemm :2710-2711: ceil(M/128) ceil(N/256) < 240 and
                                    ceil(M/128) ceil(N/128) >= 240), ceil(rows/64) ceil(n_in_below/128) >= 200,
                                    px_exact<64,128> of the backward (:2428: rows % 64 == 0, n_in % 128 == 0)
  G.wide        :2852, launch_pair_wide_bwd_t :2821-2833: the update planned m128x256k32s3 (ceil(M/128) ceil(N/256)
                                    >= 240), the backward from the transposed shadow with K/64 whole and even
  G.upd+upd     cunetwork.cpp:642-653, launch_upd_pair :2908-2918: the stopper (or layer 0) and a held-back update
                                    above it, both 64x64 grids together within the CUs:
                                    ceil(M1/64) ceil(N1/64) + ceil(M2/64) ceil(N2/64) <= 256
  G.gather      cunetwork.cpp:643, tnet_affine_update_bias_gather :3562-3582: as G.upd+upd plus >= 8 CUs left over;
                                    trainer.cpp:86: only while the cache holds a bunch ahead
  G.grad+bwd    cunetwork.cpp:586,663; launch_pair_a_bwd<EPI_STORE_BG>: G.upd+bwd's conditions from W (no shadow in
                                    the data-parallel step, cunetwork.cpp:419)
  G.crossval    cunetwork.cpp:501   !train returns after the objective

Small cases run steps of 32, 19, 64 and 1 rows (stack_cases.ROWS); large ones 2 steps of B rows.  The large cases'
rates are 8 times stack_cases.consts' (4 times without GradDivFrm): their tolerance is 2 ulp(W) + 1e-4 of the block's
largest move, and at the plain rate -- a tenth of it under momentum 0.9 -- the two float32 roundings of W per step
alone take half of that (measured shares at the plain rate: 0.46 to 0.55).

Measured by tests/test_step_cases_cpu.py (it prints them; copied here)
  float32 headroom     fused-top-cap 0.0383, three-call-top 0.0456, one-layer-fused 0.0181, one-layer-wide 0.0542,
                       top-frozen 0.0137, middle-frozen 0.015, stopper-middle 0.0178, only-top 0.0146, only-top-wide
                       0.0493, crossval 0.0121, keep-output-on 0.0271, keep-output-off 0.0271, keep-output-wide-on
                       0.0348, keep-output-wide-off 0.0348, colsum-declined 0.074, top-split 0.2, pair-narrow 0.112,
                       pair-narrow-ring 0.0448, pair-wide 0.117, pair-closed 0.113, mlp3 0.103, gather-tail-small
                       0.0142, gather-tail-mlp3 0.111, dp-pair-narrow 0.112, dp-mlp3 0.111
  (bound 0.25: the restatement in float32 numpy against float64, worst deviation / tolerance over every exposed
  output, parameter and the objective sum)
  C oracle             fused-top-cap 0.0068, three-call-top 0.00089, one-layer-fused 0.00939, one-layer-wide 0.00152,
                       keep-output-on 0.00148, keep-output-off 0.00148, keep-output-wide-on 0.00455, keep-output-wide-
                       off 0.00455, colsum-declined 0.000883, top-split 0.000947, pair-narrow 0.112, pair-narrow-ring
                       0.0443, pair-wide 0.115, pair-closed 0.113, mlp3 0.103, gather-tail-small 0.00134, gather-tail-
                       mlp3 0.111, dp-pair-narrow 0.112, dp-mlp3 0.111
  (oracle.MLP.step, a float32 program, against the restatement in shares of the same tolerance; bound 0.25)
  C oracle, double     oracle.MLP(dtype=float64).step -- the same C source built with double storage -- against the
                       restatement, worst |oracle - restatement| / max|restatement| per parameter block: 1.4e-16
                       (one-layer-wide) to 1.3e-15 (pair-wide) over the 19 uniform-rate cases (bound 1e-12); with its
                       usual float32 storage the oracle is 1.0e-7 to 3.0e-7 away, float32 rounding
  sensitivity          fused-top-cap post-update-backward 562, three-call-top post-update-backward 2.35e+03, top-
                       frozen post-update-backward 41.8, top-frozen frozen-updated 2.94e+05, middle-frozen post-
                       update-backward 317, middle-frozen frozen-updated 2.72e+04, stopper-middle post-update-backward
                       508, stopper-middle frozen-updated 5.52e+03, stopper-middle factor-ignored 4.49e+04, only-top
                       frozen-updated 5.32e+03, only-top-wide frozen-updated 1.42e+04, crossval frozen-updated
                       2.94e+05, keep-output-on post-update-backward 2.46e+03, keep-output-off post-update-backward
                       2.46e+03, keep-output-wide-on post-update-backward 571, keep-output-wide-off post-update-
                       backward 571, colsum-declined post-update-backward 76.9, top-split post-update-backward 27,
                       pair-narrow post-update-backward 9.04e+03, pair-narrow-ring post-update-backward 7.33e+04,
                       pair-wide post-update-backward 2.44e+03, pair-closed post-update-backward 8.76e+03, mlp3 post-
                       update-backward 1.55e+03, gather-tail-small post-update-backward 68.8, gather-tail-mlp3 post-
                       update-backward 1.68e+03, dp-pair-narrow post-update-backward 9.04e+03, dp-mlp3 post-update-
                       backward 1.68e+03
  (bound >= 10: a deliberately wrong restatement against the right one, in tolerances.  Only the variants that can
  differ from the right restatement are run for a case (wrong_applies): a factor cannot be ignored where none is set,
  nothing is frozen where every factor is 1, and the backward order cannot matter without a trained layer above
  another trained layer's backward.  one-layer-fused and one-layer-wide therefore have NO sensitivity figure: with
  one layer at factor 1 none of the three wrong restatements differs from the right one)
"""
import functools
from collections import Counter, namedtuple

import numpy as np

import stack_cases as sc
from tnet_amd import formats

IGNORED_TAGS = ("transpose:",)
LARGE_RTOL_MOVE = 1e-4                 # large cases: |W - W_ref| <= 2 ulp(W) + 1e-4 max|W_ref - W_init| per block
OBJ_RTOL = 1e-5
INIT_SEED, DATA_SEED = 190, 191

Case = namedtuple("Case", "name dims rows consts factors train keep runner large lr_scale tags")


def _case(name, dims, tags, rows=sc.ROWS, consts=1, factors=None, train=True, keep=True, runner="net", large=False,
          lr_scale=1.0):
    return Case(name, tuple(dims), tuple(rows), sc.CONSTS[consts], factors, train, keep, runner, large, lr_scale, tags)


def _fwd3(top):
    """the forward of 23 -> 48 -> 40 -> top: the <= 256-class fused top (G.fused-top) or the three calls"""
    t = {"gemm_fwd:23x48": 1, "gemm_fwd:48x40": 1}
    if top <= 256:
        t[f"gemm_fwd+softmax:40x{top}"] = 1
    else:
        t.update({f"gemm_fwd:40x{top}": 1, f"softmax_xent:{top}": 1})
    return t


def _all_trained3(top):
    """23 -> 48 -> 40 -> top with every layer trained at these small sizes: the top backward with column sums
    (G.bwd-colsum), G.upd+bwd declined (40 x top plans no 128x128 grid) so the top update alone, layer 1's backward,
    then layers 1 and 0 as one launch (G.upd+upd: 1 + 1 tiles).  A wide top's slab sums: G.ride wants the ride
    (top_bwd) and the backward declines it (1 * 1 tiles < 200): `colsum:top`"""
    t = _fwd3(top)
    t.update({f"gemm_bwd:40x{top}": 1, f"gemm_upd:40x{top}": 1, "gemm_bwd:48x40": 1, "gemm_upd+upd:48x40+23x48": 2})
    if top > 256:
        t[f"colsum:{top}"] = 1
    return t


SMALL = [
    # G.fused-top at the cap exactly
    _case("fused-top-cap", [23, 48, 40, 256], _all_trained3(256), consts=1),
    # one class past it
    _case("three-call-top", [23, 48, 40, 257], _all_trained3(257), consts=0),
    # nl == 1: G.stopper leaves no backward; the update is the held-back one flushed after the loop
    # (cunetwork.cpp:722)
    _case("one-layer-fused", [23, 12], {"gemm_fwd+softmax:23x12": 1, "gemm_upd:23x12": 1}, consts=3),
    # ... and with a wide top G.ride's top_bwd is false (nl == 1): the slab sums' own launch
    _case("one-layer-wide", [23, 300], {"gemm_fwd:23x300": 1, "softmax_xent:300": 1, "colsum:300": 1,
                                        "gemm_upd:23x300": 1}, consts=2),
    # top_colsum false (cunetwork.cpp:439): no slab sums; both backwards with column sums (the layers below are
    # trained); no top update; G.upd+upd for layers 1 and 0
    _case("top-frozen", [23, 48, 40, 12], dict(_fwd3(12), **{"gemm_bwd:40x12": 1, "gemm_bwd:48x40": 1,
                                                             "gemm_upd+upd:48x40+23x48": 2}),
          consts=1, factors="1,1,0"),
    # the top backward hands its error to a frozen layer: plain tnet_affine_bwd (G.bwd-colsum, same tag); the held-back
    # top update finds G.upd+bwd closed and goes alone; layer 1's backward with column sums; layer 0 (the stopper)
    # has no held-back partner: alone
    _case("middle-frozen", [23, 48, 40, 12], dict(_fwd3(12), **{"gemm_bwd:40x12": 1, "gemm_upd:40x12": 1,
                                                                "gemm_bwd:48x40": 1, "gemm_upd:23x48": 1}),
          consts=3, factors="1,0,1"),
    # the stopper is layer 1: one backward (the top's), G.upd+upd for the top and layer 1 (1 + 1 tiles)
    _case("stopper-middle", [23, 48, 40, 12], dict(_fwd3(12), **{"gemm_bwd:40x12": 1, "gemm_upd+upd:40x12+48x40": 2}),
          consts=1, factors="0,1,0.5"),
    # the top is the stopper: no backward at all
    _case("only-top", [23, 48, 40, 12], dict(_fwd3(12), **{"gemm_upd:40x12": 1}), consts=2, factors="0,0,1"),
    # ... and G.ride's top_bwd is false (top == stopper): `colsum:300`
    _case("only-top-wide", [23, 48, 40, 300], dict(_fwd3(300), **{"colsum:300": 1, "gemm_upd:40x300": 1}),
          consts=1, factors="0,0,1"),
    # G.crossval
    _case("crossval", [23, 48, 40, 12], _fwd3(12), consts=1, train=False),
    _case("keep-output-on", [23, 48, 40, 12], _all_trained3(12), consts=0, keep=True),
    _case("keep-output-off", [23, 48, 40, 12], _all_trained3(12), consts=0, keep=False),
    _case("keep-output-wide-on", [23, 48, 40, 300], _all_trained3(300), consts=3, keep=True),
    _case("keep-output-wide-off", [23, 48, 40, 300], _all_trained3(300), consts=3, keep=False),
    # A refusal from a column-sum kernel (reduce.hip:259: tnet_colsum_slab_sums declines more than 256 slabs, i.e. more
    # than 8192 rows): 8224 rows under a wide top.  G.ride wants the ride and the backward declines it (129 * 1 tiles
    # < 200), the slab sums' own launch declines too and reports nothing (its scope is cancelled), so err_colsum is
    # false for the trained top layer: CuBiasedLinearity::UpdateFrom inside the fused step (cunetwork.cpp:708),
    # `bias_update:300` + `gemm_upd:40x300`.  The backwards still write their 257 slabs each
    _case("colsum-declined", [23, 48, 40, 300],
          {"gemm_fwd:23x48": 1, "gemm_fwd:48x40": 1, "gemm_fwd:40x300": 1, "softmax_xent:300": 1, "gemm_bwd:40x300": 1,
           "bias_update:300": 1, "gemm_upd:40x300": 1, "gemm_bwd:48x40": 1, "gemm_upd+upd:48x40+23x48": 2},
          rows=(8224, 8224), consts=1, lr_scale=16.0),   # (the mean gradient of 8224 rows is small)
    # the K = 512 top of at most 256 classes at 64 rows (top_rows.hip's K-slice kernel, TNET_TOP_SPLIT): the tags
    # are the fused top's either way; G.upd+upd: 1 * 8 + 1 tiles
    _case("top-split", [23, 48, 512, 135],
          {"gemm_fwd:23x48": 1, "gemm_fwd:48x512": 1, "gemm_fwd+softmax:512x135": 1, "gemm_bwd:512x135": 1,
           "gemm_upd:512x135": 1, "gemm_bwd:48x512": 1, "gemm_upd+upd:48x512+23x48": 2}, rows=(64, 64), consts=1),
]


def _large3(d, pair, ride=True):
    """d0 -> d1 -> d2 -> d3 (d3 > 256) with every layer trained at 960 or 1024 rows: three forwards and the softmax;
    the top backward carries the slab sums (G.ride: ceil(rows/64) * ceil(d2/128) >= 200 for every d2 used here, so no
    `colsum`); the top update with layer 1's backward as one launch where `pair`; G.upd+upd closed for layers 1 and 0
    (ceil(d1/64) ceil(d2/64) alone is far past 256): one update each"""
    d0, d1, d2, d3 = d
    t = {f"gemm_fwd:{d0}x{d1}": 1, f"gemm_fwd:{d1}x{d2}": 1, f"gemm_fwd:{d2}x{d3}": 1, f"softmax_xent:{d3}": 1,
         f"gemm_bwd:{d2}x{d3}": 1, f"gemm_upd:{d1}x{d2}": 1, f"gemm_upd:{d0}x{d1}": 1}
    if not ride:
        t[f"colsum:{d3}"] = 1
    if pair:
        t[f"gemm_upd+bwd:{d2}x{d3}+{d1}x{d2}"] = 2
    else:
        t.update({f"gemm_upd:{d2}x{d3}": 1, f"gemm_bwd:{d1}x{d2}": 1})
    return t


PAIR_NARROW = [128, 1664, 2048, 1920]
PAIR_RING = [128, 1664, 1984, 1920]
PAIR_WIDE = [128, 2048, 2048, 3840]
MLP3 = [598, 1024, 135]
# MLP3 at 1024 rows: the fused top; its backward (column sums); G.upd+upd: 16 * 3 + 10 * 16 = 208 tiles <= 256
MLP3_TAGS = {"gemm_fwd:598x1024": 1, "gemm_fwd+softmax:1024x135": 1, "gemm_bwd:1024x135": 1,
             "gemm_upd+upd:1024x135+598x1024": 2}

LARGE = [
    # G.upd+bwd: top update 2048 x 1920: 16 * 8 = 128 < 240, 16 * 15 = 240 >= 240: m128x128; layer 1's backward
    # 1024 x 1664: 16 * 13 = 208 >= 200 tiles, 1024 % 64 == 0, 1664 % 128 == 0, from layer 1's transposed shadow
    # (K/64 = 32: the direct form).  G.ride: 16 * 16 = 256 >= 200
    _case("pair-narrow", PAIR_NARROW, _large3(PAIR_NARROW, True), rows=(1024, 1024), consts=1, large=True, lr_scale=8.0),
    # the same with K = 1984: K/64 = 31 is odd (launch_pair_a_bwd :2876: bt = 2, the ring) and 1984 % 128 != 0
    # (px_exact<128,128> of the update false); top update 16 * 15 = 240 tiles still
    _case("pair-narrow-ring", PAIR_RING, _large3(PAIR_RING, True), rows=(1024, 1024), consts=0, large=True, lr_scale=4.0),
    # G.wide: top update 2048 x 3840: 16 * 15 = 240 tiles of 128x256; layer 1's backward 1024 x 2048 over K = 2048
    _case("pair-wide", PAIR_WIDE, _large3(PAIR_WIDE, True), rows=(1024, 1024), consts=3, large=True, lr_scale=8.0),
    # 960 rows: layer 1's backward 15 * 13 = 195 < 200 tiles: G.upd+bwd closed; G.ride still open (15 * 16 = 240)
    _case("pair-closed", PAIR_NARROW, _large3(PAIR_NARROW, False), rows=(960, 960), consts=1, large=True, lr_scale=8.0),
    _case("mlp3", MLP3, MLP3_TAGS, rows=(1024, 1024), consts=1, large=True, lr_scale=8.0),
]

CASES = {c.name: c for c in SMALL + LARGE}
assert len(CASES) == len(SMALL) + len(LARGE)


# ---- the Trainer cases: a 4-bunch cache, filled once by one utterance and shuffled (the gather exists only for a
# shuffled cache: cucache.h:53); bunch s is the rows oracle.epoch_schedule names, the reference's own lrand48 shuffle.
# Tags over the whole drain (the trainer runs it in one call): the first bunch's `gather` (cucache.cpp:348), per step
# the net's tags, and the step's last launch with the next bunch's gather on every step but the last (G.gather)
def _drain(per_step, last, last_gather, n=4):
    t = Counter({"gather": 1})
    for s in range(n):
        t.update(per_step)
        t[last_gather if s < n - 1 else last] += 2
    return dict(t)


_SMALL_STEP = dict(_fwd3(12), **{"gemm_bwd:40x12": 1, "gemm_upd:40x12": 1, "gemm_bwd:48x40": 1})
_MLP3_STEP = {"gemm_fwd:598x1024": 1, "gemm_fwd+softmax:1024x135": 1, "gemm_bwd:1024x135": 1}
TRAINER = {
    # G.gather: 1 + 1 tiles, 254 CUs left
    "gather-tail-small": _case("gather-tail-small", [23, 48, 40, 12],
                               _drain(_SMALL_STEP, "gemm_upd+upd:48x40+23x48", "gemm_upd+upd+gather:48x40+23x48"),
                               rows=(64,) * 4, consts=1, runner="trainer"),
    # G.gather: 48 + 160 = 208 tiles, 48 CUs left
    "gather-tail-mlp3": _case("gather-tail-mlp3", MLP3,
                              _drain(_MLP3_STEP, "gemm_upd+upd:1024x135+598x1024",
                                     "gemm_upd+upd+gather:1024x135+598x1024"),
                              rows=(1024,) * 4, consts=1, runner="trainer", large=True, lr_scale=8.0),
}
# TNET_GATHER_TAIL=0 (trainer.cpp:84): every bunch by the cache's own `gather`, every step's last launch the plain pair
TRAINER_NO_TAIL = {
    "gather-tail-small": dict(Counter(_drain(_SMALL_STEP, "gemm_upd+upd:48x40+23x48", "gemm_upd+upd:48x40+23x48"))
                              + Counter({"gather": 3})),
    "gather-tail-mlp3": dict(Counter(_drain(_MLP3_STEP, "gemm_upd+upd:1024x135+598x1024",
                                            "gemm_upd+upd:1024x135+598x1024")) + Counter({"gather": 3})),
}

# ---- data parallel on a one-rank RCCL communicator (the restatement is the local step's: one rank's rows are the
# global rows).  No shadows (cunetwork.cpp:419); an apply on the exchange's stream reports no tag (culayers.cpp:433),
# the step's last layer is applied on the compute stream (cunetwork.cpp:550): `sgd_apply:KxN`
_DP_NARROW = {"gemm_fwd:128x1664": 1, "gemm_fwd:1664x2048": 1, "gemm_fwd:2048x1920": 1, "softmax_xent:1920": 1,
              "gemm_bwd:2048x1920": 1, "gemm_grad:1664x2048": 1, "gemm_grad:128x1664": 1}
_DP_MLP3_LAST = {"gemm_grad:1024x135": 1, "gemm_grad:598x1024": 1}     # the fill's last step: no bunch ahead


def _dp_drain(gather_step, last_step, n=4):
    t = Counter({"gather": 1})
    for s in range(n):
        t.update(_MLP3_STEP)
        t.update(gather_step if s < n - 1 else last_step)
    return dict(t)


DP = {
    # G.grad+bwd: pair-narrow's shapes; the per-layer submission (three reductions, cunetwork.cpp:698-699)
    "dp-pair-narrow": _case("dp-pair-narrow", PAIR_NARROW,
                            dict(_DP_NARROW, **{"gemm_grad+bwd:2048x1920+1664x2048": 2, "sgd_apply:128x1664": 1}),
                            rows=(1024, 1024), consts=1, runner="dp", large=True, lr_scale=8.0),
    # MLP3 through the trainer: the top gradient is held back (cunetwork.cpp:663) and rides with layer 0's and the
    # next bunch's gather (cunetwork.cpp:670, tnet_affine_grad_bias_gather :3781-3800: 160 + 48 tiles, 48 CUs left);
    # both gradients then go out as one inline group (cunetwork.cpp:693) and one apply (culayers.cpp:455)
    "dp-mlp3": _case("dp-mlp3", MLP3,
                     _dp_drain({"gemm_grad+grad+gather:598x1024+1024x135": 2, "sgd_apply:2layers": 1},
                               dict(_DP_MLP3_LAST, **{"sgd_apply:598x1024": 1})),
                     rows=(1024,) * 4, consts=1, runner="dp-trainer", large=True, lr_scale=8.0),
}
ALL_CASES = dict(CASES, **TRAINER, **DP)

# ---- the RBM trainer under its switches: (V, H, bunch); compared with oracle.RBM as
# tests/test_gpu_rbm.py::test_rbm_trainer_epoch_matches_oracle does
RBM = {"rbm-33x70": (33, 70, 17), "rbm-440x256": (440, 256, 64)}
RBM_SEED, RBM_LR, RBM_MMT, RBM_WC = 321, 0.01, 0.5, 0.0002


# ---- the recurrent trainer's per-frame chain recorded in graph segments shorter than the utterance
# (TNET_RNN_GRAPH_FRAMES, curecurrent.cpp:320-348).  A length is recorded on its second sighting and replayed from the
# third (tests/test_gpu_rnn.py::test_rnn_graph_replay_matches_eager), so lengths repeat; constants as
# tests/rnn_modes_worker.py.  Compared with oracle.RNN at tests/test_gpu_rnn.py::test_rnn_strict_parity_mode's
# tolerances
RNN = {"rnn-graph": (40, 64, 135, 4, (30, 30, 30, 21, 30, 21))}
RNN_LR, RNN_MMT, RNN_WC = 0.02, 0.5, 1e-4
NOT_MLP = tuple(RBM) + tuple(RNN)


def rnn_corpus(name):
    n_in, H, S, bptt, lens = RNN[name]
    rng = np.random.default_rng(17)
    layers = formats.gen_recurrent_init(n_in, H, S, seed=11)
    feats = [rng.standard_normal((T, n_in)).astype(np.float32) for T in lens]
    labels = [rng.integers(0, S, T).astype(np.int32) for T in lens]
    return layers, feats, labels, bptt


def rbm_corpus(name):
    V, H, B = RBM[name]
    rng = np.random.default_rng(5)
    feats = [rng.standard_normal((int(n), V)).astype(np.float32) for n in rng.integers(40, 200, size=12)]
    layer = formats.round_trip_text(formats.gen_rbm_init(V, H, seed=6, vis_type="gauss", hid_type="bern"), 9)[0]
    return layer, feats, B, 8 * B


# ---- the switch matrix (tests/test_gpu_step_branches.py runs one child process per setting): the cases a setting
# runs and the tags it changes; a case not named in `tags` keeps its table
def _without_pairs(t):
    """TNET_GEMM_PAIR=0 (g_pair: launch_pair_a_bwd :2849, launch_upd_pair :2908, the gather's pair :3564): every
    two-GEMM launch falls back to its two calls"""
    out = Counter()
    for tag, n in t.items():
        kind, _, shapes = tag.partition(":")
        if kind == "gemm_upd+bwd":
            up, dn = shapes.split("+") if "+" in shapes else (shapes, shapes)
            out[f"gemm_upd:{up}"] += n // 2
            out[f"gemm_bwd:{dn}"] += n // 2
        elif kind == "gemm_upd+upd":
            a, b = shapes.split("+")
            out[f"gemm_upd:{a}"] += n // 2
            out[f"gemm_upd:{b}"] += n // 2
        else:
            out[tag] += n
    return dict(out)


Setting = namedtuple("Setting", "env cases tags bit_equal_default note")
PAIR_CASES = ("pair-narrow", "pair-wide", "mlp3")
SETTINGS = {s.env: s for s in [
    Setting("", ("fused-top-cap", "stopper-middle", "top-split") + PAIR_CASES + tuple(TRAINER) + tuple(DP)
            + NOT_MLP, {}, (), "the default"),
    # cunetwork.cpp:455: the three calls; the slab sums then want the ride (G.ride) and are declined at 1 * 1 tiles
    Setting("TNET_FUSED_TOP=0", ("fused-top-cap",),
            {"fused-top-cap": {"gemm_fwd:23x48": 1, "gemm_fwd:48x40": 1, "gemm_fwd:40x256": 1, "softmax_xent:256": 1,
                               "colsum:256": 1, "gemm_bwd:40x256": 1, "gemm_upd:40x256": 1, "gemm_bwd:48x40": 1,
                               "gemm_upd+upd:48x40+23x48": 2}}, (), ""),
    # cunetwork.cpp:511: the slab sums' own launch before the loop
    Setting("TNET_TOP_SLABS_RIDE=0", ("pair-narrow",),
            {"pair-narrow": dict(_large3(PAIR_NARROW, True), **{"colsum:1920": 1})}, (), ""),
    Setting("TNET_GEMM_PAIR=0", ("stopper-middle",) + PAIR_CASES,
            {n: _without_pairs(ALL_CASES[n].tags) for n in ("stopper-middle",) + PAIR_CASES}, ("pair-narrow",),
            "DESIGN 5, update + backward pairs in one launch (gemm16_pair_kernel): 'Bit-identical to the two calls "
            "(test_affine_update_bwd_pair)'.  No such sentence covers the two-update pair or the 128x256 pair"),
    # launch_pair_wide_bwd_t :2820: only the 128x256 pair goes; pair-narrow keeps its pair
    Setting("TNET_PAIR_WIDE=0", ("pair-narrow", "pair-wide"), {"pair-wide": _large3(PAIR_WIDE, False)},
            ("pair-narrow",), "the switch is read in launch_pair_wide_bwd_t alone: pair-narrow runs the default's launches"),
    # upd_mixed_ok :3473 wants the first update planned m128x128: MLP3's 1024 x 135 is not, so nothing changes
    Setting("TNET_UPD_MIXED=0", ("gather-tail-mlp3",), {}, (), "no change expected: MLP3 never takes the mixed form"),
    # trainer.cpp:84.  The gather copies rows (gather.h); the update halves of gemm16_upd_gather_kernel are
    # gemm16_upd_pair_kernel's tiles: no arithmetic differs, so the trained result is bit-identical
    Setting("TNET_GATHER_TAIL=0", tuple(TRAINER), TRAINER_NO_TAIL, tuple(TRAINER), ""),
    # top_split_ok :2354: the 32x64 split-K tiles instead of top_rows.hip's K slices; same tags
    Setting("TNET_TOP_SPLIT=0", ("top-split",), {}, (), ""),
    Setting("TNET_UPD64_DIRECT=0", PAIR_CASES, {}, (), ""),
    # g_direct :2413.  0: the ring forms; launch_pair_wide_bwd_t :2821 wants g_direct == 4, so 0, 1 and 3 close
    # the wide pair; pair-narrow's pair stays (its halves fall back to the ring inside the launch)
    Setting("TNET_GEMM_DIRECT=0", PAIR_CASES, {"pair-wide": _large3(PAIR_WIDE, False)}, ("mlp3", "pair-narrow"),
            "DESIGN 5, the direct form: 'Same MFMA operands in the same order as the ring form: bit-identical outputs "
            "(test_direct_form_bit_identical_to_ring; the whole GPU suite passes with either form)'.  pair-wide is "
            "left out: its pair closes, and no sentence claims the 128x256 pair equal to its two calls"),
    Setting("TNET_GEMM_DIRECT=1", PAIR_CASES, {"pair-wide": _large3(PAIR_WIDE, False)}, ("mlp3", "pair-narrow"),
            "DESIGN 5, the direct form: 'Same MFMA operands in the same order as the ring form: bit-identical outputs "
            "(test_direct_form_bit_identical_to_ring; the whole GPU suite passes with either form)'.  pair-wide is "
            "left out: its pair closes, and no sentence claims the 128x256 pair equal to its two calls"),
    Setting("TNET_GEMM_DIRECT=3", PAIR_CASES, {"pair-wide": _large3(PAIR_WIDE, False)}, ("mlp3", "pair-narrow"),
            "DESIGN 5, the direct form: 'Same MFMA operands in the same order as the ring form: bit-identical outputs "
            "(test_direct_form_bit_identical_to_ring; the whole GPU suite passes with either form)'.  pair-wide is "
            "left out: its pair closes, and no sentence claims the 128x256 pair equal to its two calls"),
    Setting("TNET_GEMM_KC=0", PAIR_CASES, {}, PAIR_CASES,
            "gemm_f32.hip:1216-1221, the c<D> forms with a k-contiguous operand: 'the same values in the same registers, so "
            "bit-identical to the ring and to the a<D> forms'"),
    Setting("TNET_GEMM_KC=2", PAIR_CASES, {}, PAIR_CASES,
            "gemm_f32.hip:1216-1221, the c<D> forms with a k-contiguous operand: 'the same values in the same registers, so "
            "bit-identical to the ring and to the a<D> forms'"),
    # px_exact :2428 is false everywhere with g_pre0 == 0: G.upd+bwd and G.wide close
    Setting("TNET_GEMM_PRE0=0", PAIR_CASES, {"pair-narrow": _large3(PAIR_NARROW, False),
                                             "pair-wide": _large3(PAIR_WIDE, False)}, (), ""),
    Setting("TNET_GEMM_EARLY=0", PAIR_CASES, {}, (), ""),
    Setting("TNET_GEMM_WT=0", PAIR_CASES, {}, (), ""),
    Setting("TNET_GEMM_GROUP=1", PAIR_CASES, {}, (), ""),
    Setting("TNET_GEMM_GROUP=3", PAIR_CASES, {}, (), ""),
    Setting("TNET_GEMM_SPLIT2=1", PAIR_CASES, {}, (), ""),
    # cunetwork.cpp:374,663: no gradient is held back: every gradient and backward alone; MLP3's layer 0 alone takes
    # the gather (plan_gemm gives 598 x 1024 the 64x64 grid, 160 tiles), and with the top already submitted the group
    # is not inline: the per-layer apply
    Setting("TNET_DP_PAIR=0", tuple(DP),
            {"dp-pair-narrow": dict(_DP_NARROW, **{"gemm_grad:2048x1920": 1, "gemm_bwd:1664x2048": 1,
                                                   "sgd_apply:128x1664": 1}),
             "dp-mlp3": _dp_drain({"gemm_grad:1024x135": 1, "gemm_grad+gather:598x1024": 1, "sgd_apply:598x1024": 1},
                                  dict(_DP_MLP3_LAST, **{"sgd_apply:598x1024": 1}))}, (), ""),
    # The next five change streams, events and the apply's grid only (cunetwork.cpp:543-547, trainer.cpp:482-490,
    # 642-650, 665-667, elementwise.hip:378-381): parameters bit-identical to the default child's
    # the last layer's apply on the exchange's stream too: no `sgd_apply` tag on the per-layer path
    Setting("TNET_DP_LAST_APPLY_STREAM=1", tuple(DP),
            {"dp-pair-narrow": dict(_DP_NARROW, **{"gemm_grad+bwd:2048x1920+1664x2048": 2}),
             "dp-mlp3": _dp_drain({"gemm_grad+grad+gather:598x1024+1024x135": 2, "sgd_apply:2layers": 1},
                                  _DP_MLP3_LAST)}, tuple(DP), ""),
    # every apply on the compute stream after its reduction: one `sgd_apply` per trained layer
    Setting("TNET_DP_APPLY_STREAM=0", tuple(DP),
            {"dp-pair-narrow": dict(_DP_NARROW, **{"gemm_grad+bwd:2048x1920+1664x2048": 2, "sgd_apply:2048x1920": 1,
                                                   "sgd_apply:1664x2048": 1, "sgd_apply:128x1664": 1}),
             "dp-mlp3": _dp_drain({"gemm_grad+grad+gather:598x1024+1024x135": 2, "sgd_apply:2layers": 1},
                                  dict(_DP_MLP3_LAST, **{"sgd_apply:1024x135": 1, "sgd_apply:598x1024": 1}))},
            tuple(DP), ""),
    Setting("TNET_DP_EVENT_FENCE=1", tuple(DP), {}, tuple(DP), ""),
    Setting("TNET_DP_WAITALL_COMM=1", tuple(DP), {}, tuple(DP), ""),
    Setting("TNET_SGD_BLOCKS=1", tuple(DP), {}, tuple(DP), ""),
    Setting("TNET_SGD_BLOCKS=7", tuple(DP), {}, tuple(DP), ""),
    # curbm.cpp:238: either sampling form; trainer.cpp:84's twin in the RBM trainer
    Setting("TNET_RBM_FUSED_SAMPLE=0", tuple(RBM), {}, (), ""),
    Setting("TNET_RBM_FUSED_SAMPLE=1", tuple(RBM), {}, (), ""),
    # 30- and 21-frame utterances in segments of 7: five and three graphs each.  "record segment by segment ... the
    # host state the frames advance moves exactly as in an eager run" (curecurrent.cpp:325), and replay is
    # bit-identical to eager (test_rnn_graph_replay_matches_eager): bit-identical to the default's single graph
    Setting("TNET_RNN_GRAPH_FRAMES=7", tuple(RNN), {}, tuple(RNN), ""),
]}
SETTINGS["TNET_GATHER_TAIL=0"] = SETTINGS["TNET_GATHER_TAIL=0"]._replace(
    cases=SETTINGS["TNET_GATHER_TAIL=0"].cases + tuple(RBM))


def setting_tags(setting, name):
    return SETTINGS[setting].tags.get(name, ALL_CASES[name].tags)


# ---- networks, constants, data
def layers(case):
    """zero biases below the top (negbias=False), as stack_cases.layers: with the --negbias draw little gradient
    would reach the lower layers"""
    return formats.gen_mlp_init(list(case.dims), seed=INIT_SEED, negbias=False)


def consts(case):
    """stack_cases.consts' rule (the rate shrinks with the first bunch's rows without GradDivFrm) times the case's
    lr_scale"""
    k = sc.consts(case.consts, case.rows[0])
    k["lr"] *= case.lr_scale
    k["l1"] = 0.0
    return k


@functools.lru_cache(maxsize=None)
def _data(dims, rows):
    rng = np.random.default_rng(DATA_SEED)
    return tuple((rng.standard_normal((r, dims[0])).astype(np.float32), rng.integers(0, dims[-1], r).astype(np.int32))
                 for r in rows)


TRAINER_SEED = 7


def corpus(case):
    """a Trainer case's one utterance: the bunches' rows in the order they were drawn"""
    d = _data(case.dims, case.rows)
    return np.concatenate([X for X, _ in d]), np.concatenate([lab for _, lab in d])


def data(case):
    """the bunches in training order; a Trainer case's are the shuffled cache's (oracle.epoch_schedule)"""
    if not case.runner.endswith("trainer"):
        return list(_data(case.dims, case.rows))
    import oracle as orc
    X, lab = corpus(case)
    sched = orc.epoch_schedule([len(lab)], len(lab), case.rows[0], TRAINER_SEED)
    assert sched.shape == (len(case.rows), case.rows[0]) and len(np.unique(sched)) == sched.size
    return [(X[b], lab[b]) for b in sched]


def n_layers(case):
    return len(case.dims) - 1


def exposed_outputs(case):
    """the component outputs a fused step leaves readable (Network.output) and the tests compare: every <sigmoid>'s,
    the top layer's logits and, when kept, the <softmax>'s.  (The lower linear layers write straight into their
    <sigmoid>'s buffer.)  A large case's logits are not compared: as in tests/test_gpu_fullsize.py the top layer is
    compared through Y alone (sums of 1024 to 2048 float32 products that cancel to Z near 0 cannot meet an elementwise
    atol of 2e-6, and no other tolerance is the project's)"""
    nl = n_layers(case)
    out = [2 * l + 1 for l in range(nl - 1)] + ([] if case.large else [2 * (nl - 1)])
    return out + [2 * nl - 1] if case.keep else out


# ---- the restatement, and three deliberately wrong ones
class PostUpdateBackward(sc.Oracle):
    """wrong: each layer's error handed down through its POST-update weights"""

    def _backward(self, acts, err, k, rates, stopper):
        for i in range(len(self.C) - 1, -1, -1):
            c, e_in = self.C[i], err
            if rates[i] is not None and rates[i] > 0:
                self._update(c, acts[i], e_in, rates[i], k)
            if i != stopper:
                err = self._backpropagate(c, e_in, acts[i + 1])
            if i == stopper:
                break


class FrozenUpdated(sc.Oracle):
    """wrong: a frozen layer (factor 0; under cross-validation every layer) trained at the plain rate, the error
    carried down to it past the stopper"""

    def learn_rates(self, lr, factors):
        rates, _ = super().learn_rates(lr, factors)
        return [lr if r == 0 else r for r in rates], 0

    def step(self, X, lab, k, factors=None, train=True):
        return super().step(X, lab, k, factors, True)


class FactorIgnored(sc.Oracle):
    """wrong: every trained layer at the plain rate, whatever its factor"""

    def learn_rates(self, lr, factors):
        rates, stopper = super().learn_rates(lr, factors)
        return [lr if r else r for r in rates], stopper


WRONG = {"post-update-backward": PostUpdateBackward, "frozen-updated": FrozenUpdated, "factor-ignored": FactorIgnored}


def wrong_applies(case, variant):
    """post-update-backward: a trained layer above another trained layer's backward, i.e. at least two layers at or
    above the stopper, the upper one trained, under training; frozen-updated: a factor 0 or cross-validation;
    factor-ignored: a factor that is neither 0 nor 1"""
    f = sc.parse_factors(case.factors) or [1.0] * n_layers(case)
    if variant == "post-update-backward":
        stopper = next(i for i, x in enumerate(f) if x > 0)
        return case.train and any(x > 0 for x in f[stopper + 1:])
    if variant == "frozen-updated":
        return not case.train or 0.0 in f
    return case.train and any(x not in (0.0, 1.0) for x in f)


def run_oracle(case, cls=sc.Oracle, dtype=np.float64):
    """per step (outputs of every component, state after the step, correct count so far), and the oracle"""
    ref = cls(layers(case), dtype)
    f = sc.parse_factors(case.factors)
    k = consts(case)
    steps, correct = [], 0
    for X, lab in data(case):
        acts = ref.step(X, lab, k, f, case.train)
        correct += int((acts[-1].argmax(axis=1) == lab).sum())
        steps.append((acts[1:], {key: np.array(v, copy=True) for key, v in ref.state().items()}, correct))
    return steps, ref


@functools.lru_cache(maxsize=None)
def _reference(dims, rows, consts, factors, train, lr_scale, shuffled):
    return run_oracle(Case("", dims, rows, consts, factors, train, True, "trainer" if shuffled else "net", False,
                           lr_scale, {}))


def reference(case):
    """the float64 restatement of the case, computed once per process (cases that differ only in how they are run
    share it) and left unchanged"""
    return _reference(case.dims, case.rows, case.consts, case.factors, case.train, case.lr_scale,
                      case.runner.endswith("trainer"))


def initial_state(case):
    return sc.Oracle(layers(case)).state()


trajectory = sc.trajectory            # the restatement over any layers, constants and bunches (tests/test_gpu_train.py)


# ---- the comparison (one rule for the CPU headroom / sensitivity figures and for the GPU tests)
def param_tolerance(case, key, ref, init):
    """small: the project's network-level tolerance; large: 2 ulp(W) + 1e-4 max|W_ref - W_init| per block
    (tests/test_gpu_fullsize.py)"""
    if not case.large:
        return sc.ATOL + sc.RTOL * np.abs(ref)
    return 2 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + LARGE_RTOL_MOVE * np.abs(ref - init).max()


def output_tolerance(ref, case=None, i=None):
    """the project's network-level tolerance"""
    return sc.ATOL + sc.RTOL * np.abs(ref)


def worst_share(case, got_steps, got_xent, want_steps=None, want_xent=None, detail=None):
    """worst |got - want| / tolerance over every exposed output and every parameter of every step, and the
    objective's sum against rtol 1e-5; got_steps as run_oracle's"""
    if want_steps is None:
        want_steps, ref = reference(case)
        want_xent = ref.xent
    init = initial_state(case)
    worst = 0.0
    for (go, gs, _), (wo, ws, _) in zip(got_steps, want_steps):
        for i in exposed_outputs(case):
            r = float((np.abs(go[i] - wo[i]) / output_tolerance(wo[i], case, i)).max())
            worst = max(worst, r)
            if detail is not None:
                detail[f"out{i}"] = max(detail.get(f"out{i}", 0.0), r)
        for key, w in ws.items():
            r = float((np.abs(gs[key] - w) / param_tolerance(case, key, w, init[key])).max())
            worst = max(worst, r)
            if detail is not None:
                detail[key] = max(detail.get(key, 0.0), r)
    r = abs(got_xent - want_xent) / (OBJ_RTOL * abs(want_xent))
    if detail is not None:
        detail["xent"] = r
    return max(worst, r)


def parse_report(text):
    """{tag: count} of a tnet_kernel_timing_report, without the ignored tags and the `@runs:` summary"""
    out = {}
    for line in text.splitlines():
        if not line.strip() or line.startswith("@"):
            continue
        tag, n = line.split()[:2]
        if not tag.startswith(IGNORED_TAGS):
            out[tag] = out.get(tag, 0) + int(n)
    return out
