"""Data-parallel training of <sharedlinearity>, <discretelinearity> and <sparselinearity>: the gradient-only kernels
(tnet_shared_grad, tnet_discrete_grad, tnet_sparse_grad), the range apply of the sparse layer (tnet_sparse_apply),
the three classes'
ComputeGradient / ApplyGradient under CuNetwork's generic data-parallel step, with one rank and with two and three
rank processes over the host transport (tests/dp_layers_worker.py), and the Trainer join protocol.

Tolerances
  gradient kernels     the bounds of the matching update's tests (tests/test_gpu_shared.py, test_gpu_discrete.py):
                       |G - ref| <= 2e-5 * (|X|^T |E|) + 1e-6 against float64 numpy (sparse: test_gpu_sparse.py's
                       2e-5 * (|X|^T |E|) + 2e-7 * |G_ref| + 1e-7); bias gradient rtol 1e-5 with the absolute floor
                       1e-5 on the sum.  Two runs: the same bits.
  tnet_sparse_apply    given the same fp32 G the kernel and the float64 restatement differ by the roundings of a
                       handful of fp32 operations (eps = 2^-24 each) on terms no larger than |W|, |scale|*(|G| +
                       mmt*|corrW|) and l1c; mask, soft threshold and decay are 1-Lipschitz.  Bound: 8 eps of that
                       magnitude (4 eps for corrW and accu on theirs).  Range splits: bit-equal to the full range.
  one rank, split step against the fused step of the same library: tests/test_gpu_dp.py
                       test_dp_rccl_world1_equals_local_update's rtol 1e-5 / atol 1e-7
  ranks against the global bunch (fused step and float64 restatement): tests/test_gpu_dp.py's rtol 2e-4 / atol 1e-6;
                       replicas across ranks: bit-equal
All kernel operands are views inside NaN-poisoned allocations (tests/kernel_views.py): what lies around a view must
come back untouched.
"""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dp_layers_cases as cases  # noqa: E402
from kernel_views import POISON, PoisonView, assert_frame_untouched, assert_unchanged  # noqa: E402
from tnet_amd import Comm, DeviceArray, DiscretePlan, Network, Objective  # noqa: E402
from tnet_amd._lib import MatrixDim, check, lib  # noqa: E402

ERR_ARG = -1
EPS = 2.0 ** -24
# the entry points take strides that are multiples of 4 only; `shifted` is the least they allow, a base 4 bytes past
# a 16-byte boundary: X and E then go through the masked scalar loads
LAYOUTS = ("tight", "offset", "shifted")


def S():
    return lib().tnet_stream()


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


# ====================================================================================== gradient kernels
# tnet_shared_grad cuts the reduction into n_inst * kslices slices, kslices = ceil(rows / chunk) with chunks of whole
# 32-row slabs (gemm_shared.hip plan_update): one slice in all -- the direct store from the accumulators -- needs one
# instance and rows <= 32.  (rows, n_inst, in, out):
SHARED_SHAPES = [(20, 1, 20, 12),    # one slice: the epilogue-hook store, no workspace
                 (31, 3, 20, 12),    # one slice per instance, rows below a slab
                 (70, 3, 20, 12),    # three row chunks per instance (9 slices), the last one 6 rows
                 (45, 2, 37, 50),    # window origins off 16 bytes: the masked scalar loads
                 (70, 2, 72, 136)]   # several tiles per slice with ragged edges


def shared_ref(X, E, n, n_in, n_out):
    X, E = X.astype(np.float64), E.astype(np.float64)
    xs = [X[:, i * n_in:(i + 1) * n_in] for i in range(n)]
    es = [E[:, i * n_out:(i + 1) * n_out] for i in range(n)]
    g = sum(x.T @ e for x, e in zip(xs, es))
    mag = sum(np.abs(x).T @ np.abs(e) for x, e in zip(xs, es))
    return g, mag, sum(e.sum(axis=0) for e in es)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,n,n_in,n_out", SHARED_SHAPES)
def test_shared_grad(rows, n, n_in, n_out, layout):
    X, E = rnd((rows, n * n_in), 1), rnd((rows, n * n_out), 2, 0.01)
    vX, vE = PoisonView(X, layout), PoisonView(E, layout)
    g, mag, gb = shared_ref(X, E, n, n_in, n_out)
    outs = []
    for _ in range(2):
        vG, vB = PoisonView.empty(n_in, n_out, layout), PoisonView.empty_vector(n_out, layout)
        check(lib().tnet_shared_grad(vX.ptr, vX.dim, vE.ptr, vE.dim, n, vG.ptr, vG.dim, vB.ptr, S()), "shared_grad")
        assert_frame_untouched(vG, "G")
        assert_frame_untouched(vB, "gradB")
        outs.append((vG.numpy(), vB.numpy().reshape(-1)))
    assert_unchanged(vX, vX.initial, "X")
    assert_unchanged(vE, vE.initial, "E")
    G, B = outs[0]
    err = np.abs(G - g)
    print("shared_grad max err / bound:", float((err / (2e-5 * mag + 1e-6)).max()))
    assert np.all(err <= 2e-5 * mag + 1e-6)            # (an unwritten element is still NaN and fails here)
    np.testing.assert_allclose(B, gb, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(outs[1][0], G)       # no atomics: the same bits
    np.testing.assert_array_equal(outs[1][1], B)


def test_shared_grad_zero_rows_stores_zeros():
    n, n_in, n_out = 3, 20, 12
    dX, dE = DeviceArray(1, n * n_in), DeviceArray(1, n * n_out)
    vG, vB = PoisonView.empty(n_in, n_out, "offset"), PoisonView.empty_vector(n_out, "offset")
    check(lib().tnet_shared_grad(dX.ptr, MatrixDim(0, n * n_in, dX.stride), dE.ptr, MatrixDim(0, n * n_out, dE.stride),
                                 n, vG.ptr, vG.dim, vB.ptr, S()), "shared_grad")
    assert not vG.numpy().any() and not vB.numpy().any()
    assert_frame_untouched(vG, "G")


# tnet_discrete_grad: every block has the depth `rows`, cut into ceil(rows / chunk) slices; one slice (rows <= 32)
# stores the packed gradient from the accumulators.  Ragged blocks, stripe origins off 16 bytes.
BLOCKS = list(zip(cases.DISCRETE["dims_in"], cases.DISCRETE["dims_out"]))
DISCRETE_ROWS = [20, 70, 100]   # one slice; three slices, the last of 6 rows; four


def discrete_ref(X, E, blocks):
    X, E = X.astype(np.float64), E.astype(np.float64)
    io = np.concatenate([[0], np.cumsum([b[0] for b in blocks])])
    oo = np.concatenate([[0], np.cumsum([b[1] for b in blocks])])
    gs, mags = [], []
    for k in range(len(blocks)):
        x, e = X[:, io[k]:io[k + 1]], E[:, oo[k]:oo[k + 1]]
        gs.append(x.T @ e)
        mags.append(np.abs(x).T @ np.abs(e))
    return gs, mags, E.sum(axis=0)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows", DISCRETE_ROWS)
def test_discrete_grad(rows, layout):
    plan = DiscretePlan(BLOCKS)
    n_in, n_out = sum(b[0] for b in BLOCKS), sum(b[1] for b in BLOCKS)
    X, E = rnd((rows, n_in), 3), rnd((rows, n_out), 4, 0.01)
    vX, vE = PoisonView(X, layout), PoisonView(E, layout)
    gs, mags, gb = discrete_ref(X, E, BLOCKS)
    outs = []
    for _ in range(2):
        vG, vB = PoisonView.empty_vector(plan.floats, layout), PoisonView.empty_vector(n_out, layout)
        check(lib().tnet_discrete_grad(vX.ptr, vX.dim, vE.ptr, vE.dim, plan.ptr, vG.ptr, vB.ptr, S()), "discrete_grad")
        assert_frame_untouched(vG, "Gp")
        assert_frame_untouched(vB, "gradB")
        packed = vG.numpy().reshape(-1)
        # the stride padding inside the packed buffer is never written
        assert np.all(plan.padding(packed).view(np.uint32) == POISON)
        outs.append((packed, vB.numpy().reshape(-1)))
    assert_unchanged(vX, vX.initial, "X")
    assert_unchanged(vE, vE.initial, "E")
    for G, g, mag in zip(plan.unpack(outs[0][0]), gs, mags):
        err = np.abs(G - g)
        print("discrete_grad max err / bound:", float((err / (2e-5 * mag + 1e-6)).max()))
        assert np.all(err <= 2e-5 * mag + 1e-6)
    np.testing.assert_allclose(outs[0][1], gb, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(outs[1][0].view(np.uint32), outs[0][0].view(np.uint32))
    np.testing.assert_array_equal(outs[1][1], outs[0][1])


# ====================================================================================== tnet_sparse_apply
SP_ROWS, SP_COLS = cases.SPARSE["n_in"], cases.SPARSE["n_out"]   # 37 x 70: three mask words per row, the last partial


def pack_bits(mask, ldmask):
    rows, cols = mask.shape
    words = np.zeros((rows, ldmask), np.uint32)
    r, c = np.nonzero(mask)
    np.bitwise_or.at(words, (r, c >> 5), np.uint32(1) << (c & 31).astype(np.uint32))
    return words


def apply_ref(G, W, corr, accu, mask, scale, mmt, l1c, l2):
    """CuSparseLinearity::Update's per-element arithmetic (cuSparseLinearity.cc:28-63) on a given gradient"""
    G, W, corr, accu = (a.astype(np.float64) for a in (G, W, corr, accu))
    c = G + mmt * corr
    w = W + scale * c
    a = accu + c
    w = np.where(mask != 0, w, 0.0)
    if l1c > 0:
        w = np.where(np.abs(w) < l1c, 0.0, np.where(w > 0, w - l1c, w + l1c))
    if l2 != 0:
        w = w + l2 * w
    return w, c, a


# tnet_sparse_grad takes tnet_sparse_update's forms: the sliced one is the automatic choice for a layer this small
# (ceil(rows / chunk) slices of whole 32-row slabs), the single launch -- G stored from the accumulators -- is forced
# through the form knob (1), as tests/test_gpu_sparse.py forces it.  Bound: that file's for corrW with a zero
# momentum buffer, 2e-5 * (|X|^T |E|) + 2e-7 * |G_ref| + 1e-7.
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("form", [0, 1], ids=["sliced", "single"])
@pytest.mark.parametrize("rows", [20, 70, 100])   # one slice; three, the last of 6 rows; four
def test_sparse_grad(rows, form, layout):
    X, E = rnd((rows, SP_ROWS), 5), rnd((rows, SP_COLS), 6, 0.01)
    vX, vE = PoisonView(X, layout), PoisonView(E, layout)
    g = X.astype(np.float64).T @ E.astype(np.float64)
    mag = np.abs(X).astype(np.float64).T @ np.abs(E).astype(np.float64)
    outs = []
    was = lib().tnet_sparse_update_form(form)
    try:
        for _ in range(2):
            vG, vB = PoisonView.empty(SP_ROWS, SP_COLS, layout), PoisonView.empty_vector(SP_COLS, layout)
            check(lib().tnet_sparse_grad(vX.ptr, vX.dim, vE.ptr, vE.dim, vG.ptr, vG.dim, vB.ptr, S()), "sparse_grad")
            assert_frame_untouched(vG, "G")
            assert_frame_untouched(vB, "gradB")
            outs.append((vG.numpy(), vB.numpy().reshape(-1)))
    finally:
        lib().tnet_sparse_update_form(was)
    assert_unchanged(vX, vX.initial, "X")
    assert_unchanged(vE, vE.initial, "E")
    tol = 2e-5 * mag + 2e-7 * np.abs(g) + 1e-7
    print("sparse_grad max err / bound:", float((np.abs(outs[0][0] - g) / tol).max()))
    assert np.all(np.abs(outs[0][0] - g) <= tol)
    np.testing.assert_allclose(outs[0][1], E.astype(np.float64).sum(axis=0), rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(outs[1][0], outs[0][0])
    np.testing.assert_array_equal(outs[1][1], outs[0][1])


def sparse_inputs(zero_grad=False):
    mask = (np.random.default_rng(20).random((SP_ROWS, SP_COLS)) < cases.SPARSE["density"]).astype(np.float32)
    W = rnd((SP_ROWS, SP_COLS), 21, 0.1) * mask
    G = np.zeros((SP_ROWS, SP_COLS), np.float32) if zero_grad else rnd((SP_ROWS, SP_COLS), 22, 0.5)
    corr, accu = rnd((SP_ROWS, SP_COLS), 23, 0.2), rnd((SP_ROWS, SP_COLS), 24, 0.3)
    return G, W, corr, accu, mask


CONST = dict(scale=float(np.float32(-0.05)), mmt=0.5, l1c=float(np.float32(0.01)), l2=float(np.float32(-1e-3)))


def run_apply(layout, cuts, G, W, corr, accu, mask):
    """the call over [0, rows*stride) split at `cuts`; W and G in different layouts (strides of their own)"""
    g_layout = "offset" if layout == "tight" else "tight"
    vW, vC, vA = PoisonView(W, layout), PoisonView(corr, g_layout), PoisonView(accu, layout)
    vG = PoisonView(G, g_layout)
    ldmask = (SP_COLS + 31) // 32
    vM = PoisonView(pack_bits(mask, ldmask), layout, dtype=np.uint32)
    edges = [0] + list(cuts) + [SP_ROWS * vW.stride]
    for lo, hi in zip(edges[:-1], edges[1:]):
        check(lib().tnet_sparse_apply(vW.ptr, vW.dim, vG.ptr, vG.stride, vC.ptr, vC.stride, vA.ptr, vA.stride, vM.ptr,
                                      vM.stride, lo, hi, CONST["scale"], CONST["mmt"], CONST["l1c"], CONST["l2"], S()),
              "sparse_apply")
    for v, what in ((vW, "W"), (vC, "corrW"), (vA, "accu")):
        assert_frame_untouched(v, what)
    assert_unchanged(vG, vG.initial, "G")
    assert_unchanged(vM, vM.initial, "bits")
    return vW.numpy(), vC.numpy(), vA.numpy(), vW.stride


@pytest.mark.parametrize("zero_grad", [False, True], ids=["grad", "zero-grad"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sparse_apply_full_and_split_ranges(layout, zero_grad):
    """zero-grad: the call of a step without rows -- momentum, mask, L1 and L2 still apply"""
    G, W, corr, accu, mask = sparse_inputs(zero_grad)
    full = run_apply(layout, [], G, W, corr, accu, mask)
    stride = full[3]
    w, c, a = apply_ref(G, W, corr, accu, mask, **CONST)
    mag_c = np.abs(G).astype(np.float64) + CONST["mmt"] * np.abs(corr)
    tol_w = 8 * EPS * (np.abs(W) + abs(CONST["scale"]) * mag_c + CONST["l1c"])
    print("sparse_apply W max err / tol:", float((np.abs(full[0] - w) / tol_w).max()))
    assert np.all(np.abs(full[0] - w) <= tol_w)
    assert np.all(np.abs(full[1] - c) <= 4 * EPS * mag_c)
    assert np.all(np.abs(full[2] - a) <= 4 * EPS * (np.abs(accu) + mag_c))
    assert np.all(full[0][mask == 0] == 0.0)
    assert (full[0][mask == 1] == 0.0).any() and (full[0] != 0).any()      # the soft threshold took some, not all
    if zero_grad:
        assert not np.array_equal(full[0], W) and np.array_equal(full[1], (0.5 * corr).astype(np.float32))
    # cuts inside a mask word of row 0 (column 45), inside row 1 (column 33) and in a row's padding
    for cuts in ([stride + 33], [45, stride + 33], [45, 3 * stride - 1]):
        split = run_apply(layout, cuts, G, W, corr, accu, mask)
        for k, what in enumerate(("W", "corrW", "accu")):
            np.testing.assert_array_equal(split[k], full[k], err_msg=f"{what} cuts {cuts}")


# ====================================================================================== argument checks
def test_argument_errors_return_err_arg():
    """refused before any launch.  Every operand is a real device buffer large enough for the good call, so a check
    that failed to refuse would still touch only memory this test owns"""
    L, s = lib(), S()
    n = 8
    # ---- tnet_shared_grad: X [8 x 16], E [8 x 16], 2 instances of 8 -> 8
    X, E, G = DeviceArray(n, 2 * n), DeviceArray(n, 2 * n), DeviceArray(n, n)
    gb = DeviceArray(1, 64)
    dA, dG = MatrixDim(n, 2 * n, 64), MatrixDim(n, n, 64)

    def sg(x=X.ptr, dx=dA, e=E.ptr, de=dA, inst=2, g=G.ptr, dg=dG, b=gb.ptr):
        return L.tnet_shared_grad(x, dx, e, de, inst, g, dg, b, s)

    assert sg() == 0
    for k in ("x", "e", "g", "b"):
        assert sg(**{k: None}) == ERR_ARG, k
    assert sg(inst=0) == ERR_ARG and sg(inst=3) == ERR_ARG
    assert sg(dx=MatrixDim(n, 2 * n - 1, 64)) == ERR_ARG and sg(de=MatrixDim(n, 2 * n + 1, 64)) == ERR_ARG
    assert sg(de=MatrixDim(n - 1, 2 * n, 64)) == ERR_ARG and sg(dg=MatrixDim(n, n - 1, 64)) == ERR_ARG
    assert sg(dx=MatrixDim(n, 2 * n, 62)) == ERR_ARG and sg(de=MatrixDim(n, 2 * n, 62)) == ERR_ARG
    assert sg(dg=MatrixDim(n, n, 62)) == ERR_ARG and sg(dg=MatrixDim(n, n, 4)) == ERR_ARG
    assert sg(g=X.ptr) == ERR_ARG and sg(g=E.ptr + 64) == ERR_ARG and sg(b=X.ptr) == ERR_ARG
    assert sg(g=G.ptr + 2) == ERR_ARG

    # ---- tnet_discrete_grad: blocks (8, 8) -> (8, 8)
    plan = DiscretePlan([(n, n), (n, n)])
    Gp = DeviceArray(1, plan.floats)

    def dg_(x=X.ptr, dx=dA, e=E.ptr, de=dA, pl=plan.ptr, g=Gp.ptr, b=gb.ptr):
        return L.tnet_discrete_grad(x, dx, e, de, pl, g, b, s)

    assert dg_() == 0
    for k in ("x", "e", "pl", "g", "b"):
        assert dg_(**{k: None}) == ERR_ARG, k
    assert dg_(dx=MatrixDim(n, 2 * n - 1, 64)) == ERR_ARG and dg_(de=MatrixDim(n, 2 * n + 1, 64)) == ERR_ARG
    assert dg_(de=MatrixDim(n - 1, 2 * n, 64)) == ERR_ARG
    assert dg_(dx=MatrixDim(n, 2 * n, 62)) == ERR_ARG and dg_(de=MatrixDim(n, 2 * n, 18)) == ERR_ARG
    assert dg_(g=X.ptr) == ERR_ARG and dg_(g=E.ptr + 64) == ERR_ARG and dg_(b=E.ptr) == ERR_ARG
    assert dg_(b=Gp.ptr + 16) == ERR_ARG and dg_(g=Gp.ptr + 2) == ERR_ARG

    # ---- tnet_sparse_grad: X [8 x 8], E [8 x 8], G [8 x 8]
    W, Gs, Cw, A, M = (DeviceArray(n, n) for _ in range(5))
    good = MatrixDim(n, n, 64)

    def spg(x=W.ptr, dx=good, e=Cw.ptr, de=good, g=Gs.ptr, dg=good, b=gb.ptr):
        return L.tnet_sparse_grad(x, dx, e, de, g, dg, b, s)

    assert spg() == 0
    for k in ("x", "e", "g", "b"):
        assert spg(**{k: None}) == ERR_ARG, k
    assert spg(dx=MatrixDim(n, n - 1, 64)) == ERR_ARG and spg(de=MatrixDim(n, n + 1, 64)) == ERR_ARG
    assert spg(de=MatrixDim(n - 1, n, 64)) == ERR_ARG and spg(dg=MatrixDim(n - 1, n, 64)) == ERR_ARG
    for k in ("dx", "de", "dg"):
        assert spg(**{k: MatrixDim(n, n, 62)}) == ERR_ARG and spg(**{k: MatrixDim(n, n, 4)}) == ERR_ARG, k
    assert spg(g=W.ptr) == ERR_ARG and spg(g=Cw.ptr + 64) == ERR_ARG and spg(b=W.ptr) == ERR_ARG
    assert spg(b=Gs.ptr + 16) == ERR_ARG and spg(g=Gs.ptr + 2) == ERR_ARG

    # ---- tnet_sparse_apply: W [8 x 8] at stride 64

    def ap(w=W.ptr, dw=good, g=Gs.ptr, ldg=64, c=Cw.ptr, ldc=64, a=A.ptr, lda=64, m=M.ptr, ldm=1, lo=0, hi=n * 64):
        return L.tnet_sparse_apply(w, dw, g, ldg, c, ldc, a, lda, m, ldm, lo, hi, -0.1, 0.5, 0.0, 0.0, s)

    assert ap() == 0 and ap(lo=5, hi=5) == 0 and ap(lo=70, hi=n * 64 - 3) == 0
    for k in ("w", "g", "c", "a", "m"):
        assert ap(**{k: None}) == ERR_ARG, k
    assert ap(dw=MatrixDim(n, n, 62)) == ERR_ARG and ap(dw=MatrixDim(n, n, 4)) == ERR_ARG
    for k in ("ldg", "ldc", "lda"):
        assert ap(**{k: 62}) == ERR_ARG and ap(**{k: 4}) == ERR_ARG, k
    assert ap(ldm=0) == ERR_ARG
    assert ap(lo=9, hi=8) == ERR_ARG and ap(hi=n * 64 + 1) == ERR_ARG and ap(lo=-1) == ERR_ARG
    assert ap(g=W.ptr) == ERR_ARG and ap(c=W.ptr + 16) == ERR_ARG and ap(a=Gs.ptr) == ERR_ARG and ap(m=A.ptr) == ERR_ARG
    assert ap(w=W.ptr + 2) == ERR_ARG and ap(m=M.ptr + 1) == ERR_ARG


# ====================================================================================== one rank: split step = fused step
ROWS1 = 48
_COMMS = {}


def one_rank_comm(transport):
    """communicators are kept for the module: "host" (all-reduce over one rank: nothing to add), "rccl", and
    "rccl-shard" (TNET_DP_SHARD=1 is read when the communicator is made)"""
    if transport not in _COMMS:
        if transport == "host":
            _COMMS[transport] = Comm.host(0, 1, lambda a: None)
        else:
            old = os.environ.get("TNET_DP_SHARD")
            os.environ["TNET_DP_SHARD"] = "1" if transport == "rccl-shard" else "0"
            try:
                _COMMS[transport] = Comm(0, 1, Comm.unique_id())
            finally:
                if old is None:
                    del os.environ["TNET_DP_SHARD"]
                else:
                    os.environ["TNET_DP_SHARD"] = old
    return _COMMS[transport]


def train(kind, gdf, rows, comm=None):
    net = Network(text=cases.net_text(kind))
    cases.configure(net, cases.consts(kind, gdf, rows))
    if comm is not None:
        net.set_comm(comm)
    obj = Objective()
    for X, L in cases.bunches(kind, rows, 3):
        net.train_bunch(obj, DeviceArray.from_numpy(X), DeviceArray.vector(L))
    return net, obj


@functools.lru_cache(maxsize=None)
def fused_state(kind, gdf, rows):
    """the fused single-process steps (no communicator: the code as it was), computed once and shared"""
    net, obj = train(kind, gdf, rows)
    st = cases.state(net, kind)
    for v in st.values():
        v.setflags(write=False)
    return st, obj.stats()


# the sparse layer does not take the sharded apply (refused: test_refusals below)
ONE_RANK = [(k, t) for k in cases.KINDS for t in ("host", "rccl", "rccl-shard") if not (k == "sparse" and t == "rccl-shard")]


@pytest.mark.parametrize("gdf", [True, False], ids=["graddivfrm", "nodiv"])
@pytest.mark.parametrize("kind,transport", ONE_RANK)
def test_one_rank_split_step_equals_fused_step(kind, transport, gdf):
    """three bunches of 48 rows, momentum 0.5, weight cost and (sparse) L1 on: the split ComputeGradient -> reduce ->
    ApplyGradient step of a one-rank communicator against the fused Update() step; the third step's parameters carry
    the momentum buffers of the first two"""
    want, want_stats = fused_state(kind, gdf, ROWS1)
    net, obj = train(kind, gdf, ROWS1, one_rank_comm(transport))
    got = cases.state(net, kind)
    assert set(got) == set(want)
    for k in want:
        if k in ("mask", "nframes"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        else:
            d = np.abs(got[k].astype(np.float64) - want[k])
            print(f"{kind} {transport} {k}: max |diff| {d.max():.3g}, max diff / tol "
                  f"{(d / (1e-7 + 1e-5 * np.abs(want[k]))).max():.3g}")
            np.testing.assert_allclose(got[k], want[k], rtol=1e-5, atol=1e-7, err_msg=k)
            # the sparse layer's gradient is summed in the fused update's slice order and applied by the same
            # per-element arithmetic: W and accu (the running sum of corrW) come out bit for bit
            if kind == "sparse" and k in ("W0", "accu"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    if kind == "sparse":
        assert got["nframes"][0] == 3 * ROWS1
    np.testing.assert_allclose(obj.stats()[0], want_stats[0], rtol=1e-5)
    assert obj.stats()[1] == want_stats[1] == 3 * ROWS1


# ====================================================================================== rank processes
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_ranks(tmp_path, mode, world, kinds=(), shard="0", timeout=240, all_fail=False):
    """starts `world` worker processes and collects them: each gets communicate(timeout) calls of its own, short
    ones in turn, so that the first rank that exits nonzero (or the deadline) ends the others at once instead of
    leaving them in a collective until their own timeout.  all_fail: every rank is expected to exit nonzero by
    itself.  Returns [(returncode, stderr)] with all_fail, else the ranks' (meta, arrays)."""
    import time
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(world),
               OMP_NUM_THREADS="1", TNET_DP_SHARD=shard, TNET_DP_HOST_INLINE="0")
    outs = [str(tmp_path / f"{mode}_w{world}_s{shard}_r{r}.npz") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp_layers_worker.py"), mode, outs[r], ",".join(kinds)],
                              env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    deadline = time.monotonic() + timeout
    done = {}
    failed = None
    while len(done) < world and failed is None:
        for r, p in enumerate(procs):
            if r in done:
                continue
            try:
                _, e = p.communicate(timeout=0.25)
            except subprocess.TimeoutExpired:
                if time.monotonic() > deadline:
                    failed = f"rank {r} still running after {timeout} s"
                    break
                continue
            done[r] = (p.returncode, e)
            if p.returncode != 0 and not all_fail:
                failed = f"rank {r} exited {p.returncode}:\n{e[-4000:]}"
                break
    if failed is not None:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.communicate()
        pytest.fail(failed)
    if all_fail:
        return [done[r] for r in range(world)]
    res = []
    for o in outs:
        z = np.load(o, allow_pickle=False)
        res.append((json.loads(str(z["meta"])), {k: z[k] for k in z.files if k != "meta"}))
    return res


def of_kind(arrs, kind):
    return {k.split(".", 1)[1]: v for k, v in arrs.items() if k.startswith(kind + ".")}


def assert_state_close(got, want, kind, what):
    for k, w in want.items():
        if k in ("mask", "nframes"):
            np.testing.assert_array_equal(got[k], w, err_msg=f"{what} {kind} {k}")
        else:
            np.testing.assert_allclose(got[k], w, rtol=cases.PARAM_RTOL, atol=cases.PARAM_ATOL,
                                       err_msg=f"{what} {kind} {k}")


@pytest.mark.parametrize("world,shard", [(2, "0"), (2, "1"), (3, "0"), (3, "1")])
def test_ranks_match_the_global_bunch(tmp_path, world, shard):
    """Explicit per-rank slices of three global bunches of 96 rows; in the middle step the last rank joins through
    train_empty.  shard "1": the sharded apply emulated over the host transport (world 3 leaves tails), shared and
    discrete layers only.  World 2 runs with GradDivFrm, world 3 without."""
    kinds = ("shared", "discrete") + (("sparse",) if shard == "0" else ())
    gdf = cases.rank_gdf(world)
    ranks = run_ranks(tmp_path, "ranks", world, kinds, shard)
    for r in range(1, world):   # replicas: bit-equal in every parameter, and in the sparse mask, accu and frame count
        assert set(ranks[r][1]) == set(ranks[0][1])
        for k in ranks[0][1]:
            np.testing.assert_array_equal(ranks[r][1][k], ranks[0][1][k], err_msg=f"rank {r} {k}")
    for kind in kinds:
        got = of_kind(ranks[0][1], kind)
        # the fused single-process step on the concatenated global bunch (no communicator: the code as it was)
        assert_state_close(got, fused_state(kind, gdf, cases.GLOBAL_ROWS)[0], kind, "fused")
        ref = cases.oracle_after(kind, gdf)
        assert_state_close(got, ref.state(), kind, "float64")
        frames = [ranks[r][0][kind]["frames"] for r in range(world)]
        assert sum(frames) == cases.GLOBAL_ROWS * cases.RANK_STEPS and frames[-1] < frames[0]
        if kind == "sparse":
            assert got["nframes"][0] == cases.GLOBAL_ROWS * cases.RANK_STEPS
            # sparse_update_mask after the steps: equal across ranks (above); against the float64 reference apart
            # from the elements whose reference |W| lies within the parameter tolerance of the threshold
            mask_ref, near = ref.update_mask()
            assert near.mean() <= cases.MASK_EXCLUDED_CAP
            assert (mask_ref != ref.mask).any()
            np.testing.assert_array_equal(got["mask_after"][~near], mask_ref[~near])
            assert np.all(got["W_after"][got["mask_after"] == 0] == 0.0)


@pytest.mark.parametrize("kind,shard,msg", [("sparse", "1", "cannot take the sharded apply"),
                                            ("rbm", "0", "does not support a trained <rbm>")])
def test_refusals(tmp_path, kind, shard, msg):
    """a network the data-parallel step cannot train is refused on every rank -- the one with a bunch and the one
    that joins empty -- before the step's first collective: each exits by itself, none waits for another"""
    res = run_ranks(tmp_path, "refuse", 2, (kind,), shard, timeout=120, all_fail=True)
    for r, (code, err) in enumerate(res):
        assert code == 3, f"rank {r} exited {code}:\n{err[-3000:]}"
        assert "REFUSED collectives=0 " in err and msg in err, f"rank {r}:\n{err[-3000:]}"


def test_trainer_uneven_shards_sparse_net(tmp_path):
    """Trainer.set_comm over a synthetic corpus whose utterance shards hold unequal bunch counts, on the sparse net:
    the rank that runs out joins the remaining steps through TrainEmpty with the same collective sequence"""
    ranks = run_ranks(tmp_path, "trainer", 2)
    m0, m1 = ranks[0][0], ranks[1][0]
    assert (m0["steps"], m1["steps"]) == tuple(cases.TRAINER["steps"]) and m0["steps"] != m1["steps"]
    assert m0["steps"] + m0["empty_steps"] == m1["steps"] + m1["empty_steps"]
    for k in ranks[0][1]:
        np.testing.assert_array_equal(ranks[1][1][k], ranks[0][1][k], err_msg=k)
    trained = (m0["steps"] + m1["steps"]) * cases.TRAINER["bunch"]
    assert m0["frames"] + m1["frames"] == trained
    assert ranks[0][1]["sparse.nframes"][0] == trained
    assert np.isfinite(ranks[0][1]["sparse.W0"]).all()
