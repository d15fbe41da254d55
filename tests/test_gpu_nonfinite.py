"""One +inf, -inf or NaN planted inside an input matrix: the output is non-finite exactly in the plant's footprint.

tests/nonfinite_cases.py states the rule, the restatements and the plant sites.  Every test here makes one clean run of
an entry point on PoisonViews (tests/kernel_views.py; the `tight` layout, where a clamped re-read can only land on
matrix elements, and `offset` once per family), then overwrites one element of one input at a time with each of
VALUES, in the same buffers, and checks with assert_footprint that
  * wherever the float64 restatement of the planted call is finite, the result is BIT-IDENTICAL to the clean run
    (no tolerance: an element outside the footprint is computed from the same operands in the same order), and
  * wherever it is not, the result has the restatement's class (+inf, -inf, nan);
  * where the plant changes a value without making it non-finite -- sigmoid(+-inf) is exactly 1 / 0, a softmax row
    with a -inf logit -- the result equals the restatement's (exactly, or within the softmax tests' rtol 2e-5);
  * every output's frame is still poison.
A kernel that multiplies an out-of-range or neighbouring operand by zero instead of dropping it, zeroes one operand of
a K tail only, or adds a neighbouring row, tile or GEMM with weight 0 fails the first check with a NaN outside the
footprint.  The cross-entropy totals are read with tnet_stats_fetch and have the class of the restatement's total: a
frame whose label posterior is NaN makes the total NaN, as in the reference (`if (v < FLT_MIN) v = FLT_MIN`,
cukernels.cu:131-141, keeps a NaN; fmaxf(v, FLT_MIN) did not).

The affine updates' second pass, W = W + l2 * W, turns an infinite W into NaN (inf - inf; with l2 = 0, inf + 0 * inf):
the reference makes that pass unconditionally (cuBiasedLinearity.cc:62-63) and so does the restatement.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import nonfinite_cases as nf  # noqa: E402
from kernel_views import POISON_INPUT, PoisonView, assert_frame_untouched  # noqa: E402
from nonfinite_cases import VALUES, assert_footprint, plant_sites  # noqa: E402
from test_gpu_views import AFFINE_CFGS, VIEW_SHAPES  # noqa: E402
from tnet_amd import DeviceArray  # noqa: E402
from tnet_amd._lib import MatrixDim, check, lib  # noqa: E402

TNET_OK = 0
INF, NINF, NAN = VALUES
SHAPES = VIEW_SHAPES + [(70, 135, 100)]  # K = 100: K % 4 == 0, K % 32 != 0 != K % 64 -- the masked LDS-DMA tail
CFGS = AFFINE_CFGS + ["auto+rsv8", "m64x64k32s4w41+sk8"]
# every shape under every configuration on `tight`; `offset` once per family
CASES = [(s, c, "tight") for s in SHAPES for c in CFGS] + [((70, 135, 100), "auto", "offset")]
CASE_IDS = [f"{s[0]}x{s[1]}x{s[2]}-{c}-{lay}" for s, c, lay in CASES]


def S():
    return lib().tnet_stream()


@pytest.fixture
def gemm_config():
    def use(name):
        check(lib().tnet_gemm_config(name.encode()))
    yield use
    check(lib().tnet_gemm_config(b"auto"))
    check(lib().tnet_gemm_reserve(0))


def word(v):
    return np.array([v], np.float32).view(np.uint32)[0]


class Operands:
    """the views of one entry point's operands, kept for a whole sweep.  `host` holds the clean arrays; a pure output
    (not in host) starts as poison before every launch, an in-place operand as its clean contents (or its plant)."""

    def __init__(self, layout, host, ins, outs, out_shapes, layouts=None):
        self.host, self.ins, self.outs = host, tuple(ins), tuple(outs)
        self.v, self.img = {}, {}
        for k in dict.fromkeys(self.ins + self.outs):
            lay = (layouts or {}).get(k, layout)
            if k in host:
                a = np.asarray(host[k])
                self.v[k] = PoisonView(a, lay, poison=POISON_INPUT) if k not in self.outs else PoisonView(a, lay)
            else:
                sh = out_shapes[k]  # (rows, cols) or (rows, cols, dtype)
                self.v[k] = PoisonView.empty(sh[0], sh[1], lay, *sh[2:])
            self.img[k] = self.v[k].initial
        self.planted = None

    def put(self, k):
        self.v[k].backing.upload(self.img[k].reshape(1, -1))

    def plant(self, k, r, c, val):
        v = self.v[k]
        img = v.initial.copy()
        img[v._index[r * v.cols + np.asarray(c)]] = word(val)  # c: one column or several
        self.img[k], self.planted = img, k
        self.put(k)

    def restore(self):
        k, self.planted = self.planted, None
        self.img[k] = self.v[k].initial
        self.put(k)

    def launch(self, call, what):
        """reset every output, call, return the outputs' interiors; frames checked"""
        for k in self.outs:
            self.put(k)
        st = call(self.v)
        assert st == TNET_OK, f"{what}: status {st}"
        got = {}
        for k in self.outs:
            v = self.v[k]
            raw = v.raw()
            assert_frame_untouched(v, f"{what}: {k}", raw=raw)
            got[k] = raw[v._index].view(v.dtype).reshape(v.rows, v.cols)
        return got


def check_outputs(got, clean, ref, ref_clean, what, rtol=None, atol=1e-9):
    """assert_footprint on every output; where the restatement stays finite but changes, the result equals it"""
    for k in got:
        r = np.asarray(ref[k], np.float64)
        changed = np.isfinite(r) & (r != np.asarray(ref_clean[k], np.float64))
        assert_footprint(got[k], clean[k], r, f"{what}: {k}", inside=changed)
        if changed.any():
            if rtol is None:
                bad = changed & (got[k] != r)
                assert not bad.any(), f"{what}: {k}: at {np.argwhere(bad)[0]} got {got[k][bad][0]!r}, " \
                                      f"the restatement gives {r[bad][0]!r} exactly"
            else:
                np.testing.assert_allclose(got[k][changed], r[changed], rtol=rtol, atol=atol, err_msg=f"{what}: {k}")
                zero = changed & (r == 0)  # a -inf logit's posterior, sigmoid(-inf), a zeroed block: exactly 0
                assert (got[k][zero] == 0).all(), f"{what}: {k}: not exactly 0 at {np.argwhere(zero & (got[k] != 0))[0]}"


def sweep(fam, d, call, layout, layouts=None):
    """one clean run, then every plant site x value of every operand of the family"""
    ref_clean = fam.ref(d, nf.matmul_fast)
    ops = Operands(layout, d, fam.ins, fam.outs, {k: v.shape for k, v in ref_clean.items()}, layouts)
    clean = ops.launch(call, fam.name + ": clean")
    for k, a in clean.items():
        assert np.isfinite(a).all() and np.isfinite(ref_clean[k]).all(), f"{fam.name}: clean {k} is not finite"
    n = 0
    for op, (k_axis, _) in fam.ops.items():
        a = np.asarray(d[op])
        for site, r, c in plant_sites(a.shape[0], a.shape[1], k_axis):
            for val in VALUES:
                what = f"{fam.name}: {val} in {op}[{r}, {c}] ({site})"
                ops.plant(op, r, c, val)
                got = ops.launch(call, what)
                dp = dict(d)
                dp[op] = nf.planted(a, r, c, val)
                check_outputs(got, clean, fam.ref(dp, nf.matmul_fast), ref_clean, what)
                n += 1
        ops.restore()
    # and the buffers are clean again: the last run reproduces the first bit for bit
    again = ops.launch(call, fam.name + ": clean again")
    for k in clean:
        np.testing.assert_array_equal(again[k].view(np.uint32), clean[k].view(np.uint32))
    return n


def vec(g, n, scale=1.0):
    return (g.standard_normal((1, n)) * scale).astype(np.float32)


def f64(a):
    return np.asarray(a, np.float64)


def quiet(ref):
    def ref_(h):
        with np.errstate(all="ignore"):
            return ref(h)
    return ref_


# ------------------------------------------------------------------------------------------------------------------
# Part A: the GEMM family
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def affine_d(rows, n_in, n_out):
    return nf.with_scales(nf.affine_data(rows, n_in, n_out), rows)


FAMS = {f.name: f for f in nf.gemm_families()}


def gemm_call(fam):
    """the library call of a Family of nonfinite_cases.gemm_families(), over a dict of views"""
    L, p, name = lib(), fam.params, fam.name
    if name.startswith("affine_fwd_t"):
        return lambda v: L.tnet_affine_fwd_t(v["E"].ptr, v["E"].dim, v["W"].ptr, v["W"].dim, v["b_in"].ptr,
                                             v["Yt"].ptr, v["Yt"].dim, p["act"], S())
    if name.startswith("affine_fwd"):
        return lambda v: L.tnet_affine_fwd(v["X"].ptr, v["X"].dim, v["W"].ptr, v["W"].dim, v["b"].ptr, v["Y"].ptr,
                                           v["Y"].dim, p["act"], S())
    if name.startswith("affine_bwd dsig"):
        return lambda v: L.tnet_affine_bwd(v["E"].ptr, v["E"].dim, v["W"].ptr, v["W"].dim, v["Yb"].ptr, v["Yb"].stride,
                                           v["Eo"].ptr, v["Eo"].dim, p["dsig"], S())
    if name == "affine_bwd_colsum":
        return lambda v: L.tnet_affine_bwd_colsum(v["E"].ptr, v["E"].dim, v["W"].ptr, v["W"].dim, v["Yb"].ptr,
                                                  v["Yb"].stride, v["Eo"].ptr, v["Eo"].dim, v["Po"].ptr,
                                                  v["Po"].stride, S())
    if name == "colsum_slab_sums":
        return lambda v: L.tnet_colsum_slab_sums(v["E"].ptr, v["E"].dim, v["Pe"].ptr, v["Pe"].stride, S())
    if name.startswith("affine_update_bias"):
        def call(v):
            C_, Cb = v.get("corr"), v.get("corr_b")
            return L.tnet_affine_update_bias(v["X"].ptr, v["X"].dim, v["Es"].ptr, v["Es"].dim, v["W"].ptr, v["W"].dim,
                                             C_.ptr if C_ else None, C_.stride if C_ else 0, fam_scale(v), p["mmt"],
                                             nf.UPDATE_L2, v["P"].ptr, v["P"].stride, v["b"].ptr, Cb.ptr if Cb else None, S())
        return call
    if name.startswith("affine_update"):
        def call(v):
            C_ = v.get("corr")
            return L.tnet_affine_update(v["X"].ptr, v["X"].dim, v["Es"].ptr, v["Es"].dim, v["W"].ptr, v["W"].dim,
                                        C_.ptr if C_ else None, C_.stride if C_ else 0, fam_scale(v), p["mmt"],
                                        nf.UPDATE_L2, S())
        return call
    if name == "affine_grad":
        return lambda v: L.tnet_affine_grad(v["X"].ptr, v["X"].dim, v["Es"].ptr, v["Es"].dim, v["G"].ptr, v["G"].dim,
                                            S())
    if name == "affine_grad_bias":
        return lambda v: L.tnet_affine_grad_bias(v["X"].ptr, v["X"].dim, v["Es"].ptr, v["Es"].dim, v["G"].ptr,
                                                 v["G"].dim, v["P"].ptr, v["P"].stride, v["gb"].ptr, S())
    if name == "rbm_update":
        return lambda v: L.tnet_rbm_update(v["X"].ptr, v["X"].dim, v["E"].ptr, v["E"].dim, v["W"].ptr, v["W"].dim,
                                           v["corr"].ptr, v["corr"].stride, 0.1 / v["X"].rows, p["mmt"], p["l2"], S())
    if name == "transpose":
        return lambda v: L.tnet_transpose(v["A"].ptr, v["A"].dim, v["At"].ptr, v["At"].stride, S())
    raise KeyError(name)


def fam_scale(v):
    return -0.3 / v["X"].rows  # nonfinite_cases.with_scales


def run_families(names, shape, cfg, layout, gemm_config):
    d = affine_d(*shape)
    gemm_config(cfg)
    for name in names:
        sweep(FAMS[name], d, gemm_call(FAMS[name]), layout)


@pytest.mark.parametrize("shape,cfg,layout", CASES, ids=CASE_IDS)
def test_sgemm_nonfinite(shape, cfg, layout, gemm_config):
    """tnet_sgemm, all four transposes, beta 0 (C starts as poison) and 0.5: a plant in A reaches one row of C, one in
    B one column, one in C its own element"""
    M, N, K = shape
    gemm_config(cfg)
    L = lib()
    for ta in "NT":
        for tb in "NT":
            d = nf.sgemm_data(M, N, K, ta, tb)
            for beta in (0.0, 0.5):
                fam = nf.sgemm_family(ta, tb, beta)
                sweep(fam, d, lambda v, ta=ta, tb=tb, beta=beta, fam=fam: L.tnet_sgemm(
                    ta.encode(), tb.encode(), M, N, K, fam.params["alpha"], v["A"].ptr, v["A"].stride, v["B"].ptr,
                    v["B"].stride, beta, v["C"].ptr, v["C"].stride, S()), layout)


@pytest.mark.parametrize("shape,cfg,layout", CASES, ids=CASE_IDS)
def test_affine_fwd_nonfinite(shape, cfg, layout, gemm_config):
    """tnet_affine_fwd act 0-3 and tnet_affine_fwd_t: X[r, k] reaches row r of Y, W[k, n] and b[n] column n; under a
    sigmoid an infinite pre-activation is exactly 1 / 0 (negated for act 3)"""
    run_families([f"affine_fwd act {a}" for a in range(4)] + [f"affine_fwd_t act {a}" for a in (0, 1)], shape, cfg,
                 layout, gemm_config)


@pytest.mark.parametrize("shape,cfg,layout", CASES, ids=CASE_IDS)
def test_affine_bwd_nonfinite(shape, cfg, layout, gemm_config):
    """tnet_affine_bwd (dsig 0: Ybelow is not part of the formula, a plant there reaches nothing), tnet_affine_bwd_colsum
    (E[r, c] reaches row r of Eo and the slab-sum row of r's slab only; Ybelow[r, i] one element of each) and
    tnet_colsum_slab_sums (one slab sum)"""
    run_families(["affine_bwd dsig 0", "affine_bwd dsig 1", "affine_bwd_colsum", "colsum_slab_sums"], shape, cfg, layout,
                 gemm_config)


@pytest.mark.parametrize("shape,cfg,layout", CASES, ids=CASE_IDS)
def test_affine_update_nonfinite(shape, cfg, layout, gemm_config):
    """tnet_affine_update, _update_bias (mmt 0 and 0.5: W and corrW, b and corr_b), tnet_affine_grad, _grad_bias and
    tnet_rbm_update: X[r, i] reaches row i, E[r, c] column c, a slab sum one bias element"""
    run_families(["affine_update mmt 0.0", "affine_update mmt 0.5", "affine_update_bias mmt 0.0",
                  "affine_update_bias mmt 0.5", "affine_grad", "affine_grad_bias", "rbm_update"], shape, cfg, layout,
                 gemm_config)


@pytest.mark.parametrize("layout", ["tight", "offset", "odd"])
@pytest.mark.parametrize("rows,cols", [(33, 65), (70, 135), (128, 256), (1, 129)])
def test_transpose_nonfinite(rows, cols, layout):
    d = dict(A=nf.affine_data(rows, cols, 4)["A"])
    sweep(FAMS["transpose"], d, gemm_call(FAMS["transpose"]), layout)


@pytest.mark.parametrize("layout", ["tight", "offset"])
@pytest.mark.parametrize("rows,n_in,n_out", SHAPES)
def test_affine_bwd_colsum_t_nonfinite(rows, n_in, n_out, layout):
    """the backward from the transposed shadow (the planner's configuration only: a forced one makes it decline): the
    same footprints as the W form; a plant in Wt[k, i] reaches column i"""
    d = dict(affine_d(rows, n_in, n_out))
    d["Wt"] = np.ascontiguousarray(d["W"].T)
    base = FAMS["affine_bwd_colsum_t"]
    w_axis, w_pred = base.ops["W"]
    fam = nf.Family(base.name, ("E", "Wt", "Yb"), base.outs,
                    lambda dd, mm: base.ref({**dd, "W": np.asarray(dd["Wt"]).T}, mm),
                    {"E": base.ops["E"], "Yb": base.ops["Yb"], "Wt": (0, lambda s, r, c: w_pred(s, c, r))}, **base.params)
    L = lib()
    sweep(fam, d, lambda v: L.tnet_affine_bwd_colsum_t(v["E"].ptr, v["E"].dim, v["Wt"].ptr, v["Wt"].dim, v["Yb"].ptr,
                                                       v["Yb"].stride, v["Eo"].ptr, v["Eo"].dim, v["Po"].ptr,
                                                       v["Po"].stride, S()), layout)


def fetch(stats):
    e, c = C.c_double(0), C.c_double(0)
    check(lib().tnet_stats_fetch(stats.ptr, C.byref(e), C.byref(c), S()))
    return e.value, c.value


def new_stats():
    return DeviceArray(1, 1024, np.float64, stride=1024)


def clear(stats):
    check(lib().tnet_memset(stats.ptr, 0, 1024 * 8))  # on the library's stream, in order with the launches


def check_totals(stats, xent_rows, correct_rows, what, rtol=1e-5):
    """the class of the cross-entropy total (and its value where finite) and `correct`, against the restatement"""
    xent, correct = fetch(stats)
    want = float(np.sum(xent_rows))
    assert nf.classes(np.float64(xent)) == nf.classes(np.float64(want)), \
        f"{what}: cross-entropy total {xent!r}, the restatement gives {want!r}"
    if np.isfinite(want):
        np.testing.assert_allclose(xent, want, rtol=rtol, atol=1e-5, err_msg=what)
    assert int(round(correct)) == int(np.sum(correct_rows)), f"{what}: correct {correct}, restatement {np.sum(correct_rows)}"


@pytest.mark.parametrize("layout", ["tight", "offset"])
@pytest.mark.parametrize("n_out", [7, 135, 256])
@pytest.mark.parametrize("rows,n_in", [(37, 70), (64, 512)])
def test_affine_softmax_xent_nonfinite(rows, n_in, n_out, layout, affine_cfg_all):
    """the fused top layer: a NaN (or an infinity: inf - inf in the softmax, whichever sign reaches Z) planted in
    X[r, k] makes row r of Z, Y and E non-finite and only the colpart row of r's 32-row slab; the cross-entropy total
    is NaN when r is labelled; every other row is bit-identical to the clean run.  A plant in W[k, n] or b[n] reaches
    column n of Z and, through the row sums, all of Y, E and colpart."""
    g = np.random.default_rng(7)
    X = g.standard_normal((rows, n_in)).astype(np.float32)
    W = (g.standard_normal((n_in, n_out)) * 0.1).astype(np.float32)
    b = g.standard_normal((1, n_out)).astype(np.float32)
    lab = g.integers(0, n_out, size=rows).astype(np.int32)
    lab[::7] = -1
    nf.check_conditions(multiplied=[X, W], others=[b])
    host = dict(X=X, W=W, b=b, lab=lab.reshape(1, -1))
    slabs = lib().tnet_colsum_slabs(rows)
    shapes = dict(Z=(rows, n_out), Y=(rows, n_out), E=(rows, n_out), P=(slabs, n_out))
    ops = Operands(layout, host, ("X", "W", "b", "lab"), ("Z", "Y", "E", "P"), shapes)
    stats = new_stats()

    def call(v):
        clear(stats)
        return lib().tnet_affine_softmax_xent(v["X"].ptr, v["X"].dim, v["W"].ptr, v["W"].dim, v["b"].ptr, v["lab"].ptr,
                                              v["Z"].ptr, v["Z"].stride, v["Y"].ptr, v["Y"].stride, v["E"].ptr,
                                              v["E"].stride, stats.ptr, v["P"].ptr, v["P"].stride, S())

    def z_ref(h):
        with np.errstate(all="ignore"):
            return nf.matmul_fast(h["X"], h["W"]) + np.asarray(h["b"], np.float64)

    def rest(Zk):
        """Y, E and the slab sums restated from the kernel's own Z (whose classes z_ref has just vouched for): the
        bounds of test_affine_softmax_xent_views are against that Z too"""
        Y = nf.softmax_ref(Zk)
        E, xe, co = nf.xent_labels_ref(Y, lab)
        return dict(Y=Y, E=E, P=nf.slab_sums_ref(E)), xe, co

    def totals(got, what):
        _, xe, co = nf.xent_labels_ref(got["Y"], lab)  # of the kernel's own posteriors, as the views test does
        check_totals(stats, xe, co, what)

    zc = z_ref(host)
    clean = ops.launch(call, "affine_softmax_xent: clean")
    totals(clean, "affine_softmax_xent: clean")
    rc, _, _ = rest(clean["Z"])
    plants = [("X", r, c) for _, r, c in plant_sites(rows, n_in, 1)]
    plants += [("W", r, c) for _, r, c in plant_sites(n_in, n_out, 0)][:4] + [("b", 0, n_out - 1)]
    for op, r, c in plants:
        for val in VALUES:
            what = f"affine_softmax_xent: {val} in {op}[{r}, {c}]"
            ops.plant(op, r, c, val)
            got = ops.launch(call, what)
            hp = {k: (nf.planted(host[k], r, c, val) if k == op else host[k]) for k in ("X", "W", "b")}
            check_outputs({"Z": got["Z"]}, clean, {"Z": z_ref(hp)}, {"Z": zc}, what)
            rp, xe, co = rest(got["Z"])
            # a row with a -inf logit stays finite and changes: held to the views test's bounds
            check_outputs({"Y": got["Y"]}, clean, rp, rc, what, rtol=2e-5)
            check_outputs({"E": got["E"]}, clean, rp, rc, what, rtol=2e-5, atol=1e-7)
            changed = np.isfinite(rp["P"]) & (rp["P"] != rc["P"])
            assert_footprint(got["P"], clean["P"], rp["P"], what + ": P", inside=changed)
            own = nf.slab_sums_ref(got["E"])
            with np.errstate(all="ignore"):
                tol = 32 * 1.2e-7 * nf.slab_sums_ref(np.abs(got["E"])) + 1e-7
            assert (np.abs(got["P"] - own)[changed] <= tol[changed]).all(), what + ": P against the slab sums of E"
            totals(got, what)
            if op == "X":
                assert np.isnan(got["Y"][r]).all() and not np.isfinite(got["Z"][r]).any(), what
                assert (~np.isfinite(got["P"])).any(axis=1).tolist() == [s == r // 32 for s in range(slabs)], what
                assert np.isnan(fetch(stats)[0]) == (lab[r] >= 0), what
        ops.restore()


@pytest.fixture(params=AFFINE_CFGS)
def affine_cfg_all(request):
    check(lib().tnet_gemm_config(request.param.encode()))
    yield request.param
    check(lib().tnet_gemm_config(b"auto"))


# ---- the pair launches: a plant in one half leaves the other half (and the gathered bunch) bit-identical
def pair_sweep(what, ops, call, halves, untouched=(), big=False):
    """halves: [(Family, {family operand / output name: the pair's name})].  The shapes are the smallest of each entry
    point's own test that it accepts (TNET_OK is asserted: a decline is a failure here), so the planted half is held
    to the predicted footprint of its family -- which tests/test_nonfinite_cpu.py holds to the float64 restatement
    -- instead of a float64 product of that size: outside it bit-identical to the clean run, inside it non-finite
    (NaN for a NaN plant).  Every output of the other half, and `untouched`, is bit-identical to the clean run.
    Sites: the first and the last plant site of each operand; big (2048-wide operands, 16 MB a matrix and launch):
    the last one only.  The K-tail sites of these GEMMs are swept by the single entry points' tests above."""
    clean = ops.launch(call, what + ": clean")
    for k, a in clean.items():
        assert a.dtype.kind != "f" or np.isfinite(a).all(), f"{what}: clean {k} is not finite"
    shapes = {k: a.shape for k, a in clean.items()}
    for fam, names in halves:
        fshapes = {o: shapes[names[o]] for o in fam.outs}
        for op, (k_axis, predict) in fam.ops.items():
            a = ops.host[names[op]]
            sites = plant_sites(a.shape[0], a.shape[1], k_axis)
            for site, r, c in ((sites[-1],) if big else (sites[0], sites[-1])):
                want = {names[o]: m for o, m in predict(fshapes, r, c).items()}
                for val in VALUES:
                    w = f"{what}: {val} in {names[op]}[{r}, {c}] ({site}, the {fam.name} half)"
                    ops.plant(names[op], r, c, val)
                    got = ops.launch(call, w)
                    for k in got:
                        m = want.get(k, np.zeros(shapes[k], bool))
                        same = got[k].view(np.uint32) == clean[k].view(np.uint32)
                        assert same[~m].all(), f"{w}: {k} changed outside the footprint, first at " \
                                               f"{np.argwhere(~same & ~m)[0]}"
                        inside = got[k][m]
                        assert (np.isnan(inside) if np.isnan(val) else ~np.isfinite(inside)).all(), \
                            f"{w}: {k} is finite inside the footprint"
                    for name, fetch_, want_ in untouched:
                        np.testing.assert_array_equal(fetch_(), want_, err_msg=f"{w}: {name}")
            ops.restore()
    return clean


def upd_args(v, sfx, scale, mmt, l2=nf.UPDATE_L2):
    """the argument list of one tnet_affine_update_bias over the views X<sfx>, Es<sfx>, W<sfx>, ..."""
    g = lambda k: v.get(k + sfx)  # noqa: E731
    C_, Cb = g("corr"), g("corr_b")
    return [g("X").ptr, g("X").dim, g("Es").ptr, g("Es").dim, g("W").ptr, g("W").dim, C_.ptr if C_ else None,
            C_.stride if C_ else 0, scale, mmt, l2, g("P").ptr, g("P").stride, g("b").ptr, Cb.ptr if Cb else None]


def bwd_args(v, sfx="2", w="W"):
    g = lambda k: v[k + sfx]  # noqa: E731
    return [g("E").ptr, g("E").dim, g(w).ptr, g(w).dim, g("Yb").ptr, g("Yb").stride, g("Eo").ptr, g("Eo").dim,
            g("Po").ptr, g("Po").stride]


def suffixed(d, keys, sfx):
    return {k + sfx: d[k] for k in keys}


def names_of(fam, sfx):
    return {k: k + sfx for k in set(fam.ins) | set(fam.outs)}


UPD_KEYS = ("X", "Es", "W", "corr", "P", "b", "corr_b")


@pytest.mark.parametrize("mmt", [0.0, 0.5])
@pytest.mark.parametrize("transposed", [False, True])
def test_update_bwd_pair_nonfinite(mmt, transposed):
    """tnet_affine_update_bwd_pair and _pair_t at (1024, 2048, 2048, 2048), the smallest shape of
    test_affine_update_bwd_pair / test_update_bwd_pair_t that the pair kernel accepts: the update of layer l and the
    backward of layer l - 1 in one launch"""
    rows, n_in, n_out, n_below = 1024, 2048, 2048, 2048
    up, bw = affine_d(rows, n_in, n_out), affine_d(rows, n_below, n_in)
    fu = FAMS[f"affine_update_bias mmt {mmt}"]
    fb = FAMS["affine_bwd_colsum"]
    host = suffixed(up, [k for k in UPD_KEYS if k in fu.ins], "")
    host.update(suffixed(bw, ("E", "W", "Yb"), "2"))
    ins = tuple(fu.ins) + ("E2", "Yb2")
    nb = names_of(fb, "2")
    if transposed:
        host["Wt2"] = np.ascontiguousarray(bw["W"].T)
        ins += ("Wt2",)
        w_axis, w_pred = fb.ops["W"]
        fb = nf.Family(fb.name, ("E", "Wt", "Yb"), fb.outs, None,
                       {"E": fb.ops["E"], "Yb": fb.ops["Yb"], "Wt": (0, lambda s, r, c: w_pred(s, c, r))})
        nb = names_of(fb, "2")
    else:
        ins += ("W2",)
    slabs = lib().tnet_colsum_slabs(rows)
    ops = Operands("tight", host, ins, tuple(fu.outs) + ("Eo2", "Po2"), dict(Eo2=(rows, n_below), Po2=(slabs, n_below)))
    L = lib()
    fn = L.tnet_affine_update_bwd_pair_t if transposed else L.tnet_affine_update_bwd_pair
    pair_sweep(f"update_bwd_pair{'_t' if transposed else ''} mmt {mmt}", ops,
               lambda v: fn(*upd_args(v, "", -0.3 / rows, mmt), *bwd_args(v, "2", "Wt" if transposed else "W"), S()),
               [(fu, names_of(fu, "")), (fb, nb)], big=True)


def test_grad_bwd_pair_nonfinite():
    """tnet_affine_grad_bwd_pair at (1024, 2048, 2048, 2048), the smallest shape of test_affine_grad_bwd_pair that
    the pair kernel accepts"""
    rows, n_in, n_out, n_below = 1024, 2048, 2048, 2048
    up, bw = affine_d(rows, n_in, n_out), affine_d(rows, n_below, n_in)
    fg, fb = FAMS["affine_grad_bias"], FAMS["affine_bwd_colsum"]
    host = suffixed(up, ("X", "Es", "P"), "")
    host.update(suffixed(bw, ("E", "W", "Yb"), "2"))
    slabs = lib().tnet_colsum_slabs(rows)
    ops = Operands("tight", host, ("X", "Es", "P", "E2", "W2", "Yb2"), ("G", "gb", "Eo2", "Po2"),
                   dict(G=(n_in, n_out), gb=(1, n_out), Eo2=(rows, n_below), Po2=(slabs, n_below)))
    L = lib()
    pair_sweep("grad_bwd_pair", ops,
               lambda v: L.tnet_affine_grad_bwd_pair(v["X"].ptr, v["X"].dim, v["Es"].ptr, v["Es"].dim, v["G"].ptr,
                                                     v["G"].dim, v["P"].ptr, v["P"].stride, v["gb"].ptr,
                                                     *bwd_args(v, "2"), S()),
               [(fg, names_of(fg, "")), (fb, names_of(fb, "2"))], big=True)


@pytest.mark.parametrize("mmt", [0.0, 0.5])
def test_update_bias_pair_nonfinite(mmt):
    """tnet_affine_update_bias_pair at (1024; 256 x 135, 440 x 256), the smallest accepted shape of its own test"""
    rows = 1024
    a, b = affine_d(rows, 256, 135), affine_d(rows, 440, 256)
    fu = FAMS[f"affine_update_bias mmt {mmt}"]
    keys = [k for k in UPD_KEYS if k in fu.ins]
    host = suffixed(a, keys, "")
    host.update(suffixed(b, keys, "2"))
    io = tuple(fu.outs) + tuple(k + "2" for k in fu.outs)
    ops = Operands("tight", host, tuple(fu.ins) + tuple(k + "2" for k in fu.ins), io, {})
    L = lib()
    pair_sweep(f"update_bias_pair mmt {mmt}", ops,
               lambda v: L.tnet_affine_update_bias_pair(*upd_args(v, "", -0.3 / rows, mmt),
                                                        *upd_args(v, "2", -0.3 / rows, mmt), S()),
               [(fu, names_of(fu, "")), (fu, names_of(fu, "2"))])


def gather_operands(rows, gcols, seed):
    """the next bunch's gather: (input views to keep alive, argument list, [(name, fetch, expected)]) -- y outside the sweep's frame checks (the header lets
    the gather fill y's row padding up to the next multiple of 4 columns)"""
    g = np.random.default_rng(seed)
    cache = g.standard_normal((3000, gcols)).astype(np.float32)
    lab = ((np.arange(3000, dtype=np.int32) * 7) % 4000).astype(np.int32)
    perm = g.permutation(3000).astype(np.int32)[:rows]
    vC = PoisonView(cache, "tight", poison=POISON_INPUT)
    vL, vP = PoisonView.vector(lab, "tight"), PoisonView.vector(perm, "tight")
    vy, vlo = PoisonView.empty(rows, gcols, "tight"), PoisonView.empty(1, rows, "tight", np.int32)
    args = [vy.ptr, vC.ptr, vlo.ptr, vL.ptr, vP.ptr, vy.dim, vC.dim]
    return (vC, vL, vP), args, [("gathered rows", vy.numpy, cache[perm]), ("gathered ids", vlo.numpy, lab[perm][None, :])]


NIL_UPDATE = [None, MatrixDim(0, 0, 0), None, MatrixDim(0, 0, 0), None, MatrixDim(0, 0, 0), None, 0, 0.0, 0.0, 0.0, None,
              0, None, None]
NIL_GRAD = [None, MatrixDim(0, 0, 0), None, MatrixDim(0, 0, 0), None, MatrixDim(0, 0, 0), None, 0, None]


@pytest.mark.parametrize("mmt", [0.0, 0.5])
def test_update_bias_gather_nonfinite(mmt):
    """tnet_affine_update_bias_gather at (256; 440 x 256; 440 gathered columns): the gathered bunch is exact and
    untouched by a plant in the update"""
    rows, n_in, n_out = 256, 440, 256
    d = affine_d(rows, n_in, n_out)
    fu = FAMS[f"affine_update_bias mmt {mmt}"]
    host = suffixed(d, [k for k in UPD_KEYS if k in fu.ins], "")
    ops = Operands("tight", host, fu.ins, fu.outs, {})
    keep, gargs, fetches = gather_operands(1024, n_in, 1300)
    L = lib()

    def call(v):
        return L.tnet_affine_update_bias_gather(*upd_args(v, "", -0.3 / rows, mmt), *NIL_UPDATE, *gargs, S())

    pair_sweep(f"update_bias_gather mmt {mmt}", ops, call, [(fu, names_of(fu, ""))], untouched=fetches)


def test_grad_bias_gather_nonfinite():
    """tnet_affine_grad_bias_gather at (256; 440 x 256; 440 gathered columns)"""
    rows, n_in, n_out = 256, 440, 256
    d = affine_d(rows, n_in, n_out)
    fg = FAMS["affine_grad_bias"]
    ops = Operands("tight", suffixed(d, ("X", "Es", "P"), ""), fg.ins, fg.outs, dict(G=(n_in, n_out), gb=(1, n_out)))
    keep, gargs, fetches = gather_operands(1024, n_in, 1301)
    L = lib()

    def call(v):
        return L.tnet_affine_grad_bias_gather(v["X"].ptr, v["X"].dim, v["Es"].ptr, v["Es"].dim, v["G"].ptr, v["G"].dim,
                                              v["P"].ptr, v["P"].stride, v["gb"].ptr, *NIL_GRAD, *gargs, S())

    pair_sweep("grad_bias_gather", ops, call, [(fg, names_of(fg, ""))], untouched=fetches)


@pytest.mark.parametrize("transposed", [False, True])
def test_bwd_colsum_slabs_nonfinite(transposed):
    """tnet_affine_bwd_colsum_slabs and _slabs_t at (1024, 2048, 2048), the smallest accepted shape of
    test_affine_bwd_colsum_slabs_matches_two_calls: a plant in E[r, c] reaches row r of Eo, the colpart row of r's
    slab, and ONE slab-sum element of colpartE (slab of r, column c)"""
    rows, n_in, n_out = 1024, 2048, 2048
    d = affine_d(rows, n_in, n_out)
    fb = FAMS["affine_bwd_colsum"]
    host = suffixed(d, ("E", "Yb"), "")
    wname = "Wt" if transposed else "W"
    host[wname] = np.ascontiguousarray(d["W"].T) if transposed else d["W"]
    p_e, p_w, p_y = fb.ops["E"][1], fb.ops["W"][1], fb.ops["Yb"][1]
    fam = nf.Family("affine_bwd_colsum_slabs", ("E", wname, "Yb"), ("Eo", "Po", "Pe"), None,
                    {"E": (1, lambda s, r, c: {**p_e(s, r, c), "Pe": nf.elems_of(s["Pe"], (r // 32, c))}),
                     wname: ((0, lambda s, r, c: p_w(s, c, r)) if transposed else (1, p_w)),
                     "Yb": (None, p_y)})
    slabs = lib().tnet_colsum_slabs(rows)
    ops = Operands("tight", host, fam.ins, fam.outs, dict(Eo=(rows, n_in), Po=(slabs, n_in), Pe=(slabs, n_out)))
    L = lib()
    fn = L.tnet_affine_bwd_colsum_slabs_t if transposed else L.tnet_affine_bwd_colsum_slabs
    pair_sweep(fam.name + ("_t" if transposed else ""), ops,
               lambda v: fn(v["E"].ptr, v["E"].dim, v[wname].ptr, v[wname].dim, v["Yb"].ptr, v["Yb"].stride, v["Eo"].ptr,
                            v["Eo"].dim, v["Po"].ptr, v["Po"].stride, v["Pe"].ptr, v["Pe"].stride, S()),
               [(fam, names_of(fam, ""))], big=True)


@pytest.mark.parametrize("layout", ["tight", "offset"])
@pytest.mark.parametrize("form,B", [("stats_update", 17), ("stats_update", 1025), ("update_stats", 17),
                                    ("update_stats_gather", 17)])
def test_rbm_update_stats_nonfinite(form, B, layout):
    """tnet_rbm_stats_update alone, tnet_rbm_update_stats (the CD-1 weight update and the statistics blocks in one
    launch) and its _gather form at (33, 70, 17), the larger accepted shape of test_rbm_update_stats_views;
    tnet_rbm_stats_update -- a kernel of its own (rbm_stats.h), not the column-sum pair of the other column kernels --
    also at B = 1025: 2050 rows, 65 slabs through its cross-slab combine, plants on both sides of a slab edge.  The two
    halves share V and H: Vs[r, i] reaches row i of W / corrW, vb[i], cvb[i] and the reconstruction error, never hb;
    Hs[r, j] column j, hb[j] and chb[j], never vb or the error; the gathered bunch is untouched."""
    V, H = 33, 70
    g = np.random.default_rng(1400 + B)
    host = dict(Vs=g.uniform(0.05, 0.95, (2 * B, V)).astype(np.float32), Hs=g.standard_normal((2 * B, H)).astype(np.float32),
                W=(g.standard_normal((V, H)) * 0.1).astype(np.float32),
                cW=(g.standard_normal((V, H)) * 0.01).astype(np.float32), vb=vec(g, V), cvb=vec(g, V, 0.01),
                hb=vec(g, H), chb=vec(g, H, 0.01))
    nf.check_conditions(multiplied=[host["Vs"], host["Hs"]], others=[host[k] for k in ("W", "cW", "vb", "cvb", "hb", "chb")])
    scale, mmt, l2 = 0.1 / B, 0.5, -0.1 * 2e-4
    stats = new_stats()
    L = lib()
    with_w = form != "stats_update"

    def f32(x):
        return f64(np.asarray(x, np.float32))

    def ref(h):
        Vs, Hs = f64(h["Vs"]), f64(h["Hs"])
        cv = mmt * f64(h["cvb"]) + scale * f32((Vs[:B].sum(axis=0) - Vs[B:].sum(axis=0))[None, :])
        ch = mmt * f64(h["chb"]) + scale * f32(Hs.sum(axis=0, keepdims=True))
        out = {"vb": f64(h["vb"]) + cv, "cvb": cv, "hb": f64(h["hb"]) + ch, "chb": ch}
        if with_w:
            c = mmt * f64(h["cW"]) + scale * nf.matmul_fast(Vs.T, Hs) + l2 * f64(h["W"])
            out.update(W=f64(h["W"]) + c, cW=c)
        d = Vs[B:] - Vs[:B]
        return out, (d * d).sum(axis=1), np.zeros(B)

    io = (("W", "cW") if with_w else ()) + ("vb", "cvb", "hb", "chb")
    fetches = []
    if form == "update_stats_gather":
        keep, gargs, fetches = gather_operands(B, V, 1401)

    def call(v):
        head = [v["Vs"].ptr, v["Vs"].dim, v["Hs"].ptr, v["Hs"].dim]
        tail = [B, v["vb"].ptr, v["cvb"].ptr, v["hb"].ptr, v["chb"].ptr]
        if not with_w:
            return L.tnet_rbm_stats_update(*head, *tail, scale, mmt, stats.ptr, S())
        mid = [v["W"].ptr, v["W"].dim, v["cW"].ptr, v["cW"].stride, scale, mmt, l2]
        if form == "update_stats":
            return L.tnet_rbm_update_stats(*head, *mid, *tail, stats.ptr, S())
        st = L.tnet_rbm_update_stats_gather(*head, *mid, *tail, stats.ptr, *gargs, S())
        for name, fetch_, want in fetches:
            np.testing.assert_array_equal(fetch_(), want, err_msg=f"{form}: {name}")
        return st

    plants = [("Vs", r, c, v) for r, c in ((0, 0), (B, 5), (2 * B - 1, V - 1), (B - 1, 32)) for v in VALUES]
    plants += [("Hs", r, c, v) for r, c in ((0, 0), (B, 5), (2 * B - 1, H - 1), (B - 1, 64)) for v in VALUES]
    plants += [("cvb", 0, 3, NAN), ("chb", 0, H - 1, NAN), ("vb", 0, 0, INF), ("hb", 0, 1, NINF)]
    if B > 32:  # the last row of a slab and the first of the next, in either phase, and the last slab (2 rows)
        plants += [(k, r, c, v) for k, c in (("Vs", V - 2), ("Hs", H - 2)) for r in (31, 32, B + 30, 2 * B - 2)
                   for v in VALUES]
    if with_w:
        plants += [("W", 3, 4, v) for v in VALUES] + [("cW", V - 1, H - 1, v) for v in VALUES]
    row_sweep(f"rbm {form}", layout, host, ("Vs", "Hs") + io, io, {}, call, quiet(ref), plants, stats=stats)


# ------------------------------------------------------------------------------------------------------------------
# Part B: the shared layer's instance-batched kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tight", "shifted"])
def test_shared_layer_nonfinite(layout):
    """gemm_shared.hip at the smallest case of its views test (33 rows, 3 instances of 39 -> 10): a plant in instance
    i of X or E stays in instance i of the forward's / backward's output; W[k, c] and b[c] reach column c of every
    instance.  The update's G = sum_i X_i^T E_i: a plant at X[r, window i, column c] makes row c of W (and corrW)
    non-finite and nothing else; one at E[r, window i, column c] column c of W and b[c]."""
    rows, n, n_in, n_out = 33, 3, 39, 10
    g = np.random.default_rng(1200)
    X = g.standard_normal((rows, n * n_in)).astype(np.float32)
    E = g.standard_normal((rows, n * n_out)).astype(np.float32)
    Es = (E * np.float32(0.01)).astype(np.float32)
    W = (g.standard_normal((n_in, n_out)) * 0.1).astype(np.float32)
    b, cb = vec(g, n_out), vec(g, n_out, 0.01)
    corr = (g.standard_normal((n_in, n_out)) * 0.01).astype(np.float32)
    nf.check_conditions(multiplied=[X, E, Es, W], others=[b, cb, corr])
    L = lib()

    def inst(a, i, w):
        return f64(a)[:, i * w:(i + 1) * w]

    def fwd(h):
        return {"Y": np.concatenate([nf.matmul_fast(inst(h["X"], i, n_in), h["W"]) + f64(h["b"]) for i in range(n)],
                                    axis=1)}, None, None

    x_sites = [(0, 0), (rows - 1, n * n_in - 1), (rows // 2, n_in + n_in - 1), (32, 2 * n_in), (5, n_in + 36)]
    plants = [("X", r, c, v) for r, c in x_sites for v in VALUES]
    plants += [("W", r, c, v) for _, r, c in plant_sites(n_in, n_out, 0)[:6] for v in VALUES] + [("b", 0, 3, NAN)]
    row_sweep("shared_fwd", layout, dict(X=X, W=W, b=b), ("X", "W", "b"), ("Y",), dict(Y=(rows, n * n_out)),
              lambda v: L.tnet_shared_fwd(v["X"].ptr, v["X"].dim, v["W"].ptr, v["W"].dim, v["b"].ptr, n, v["Y"].ptr,
                                          v["Y"].dim, S()), quiet(fwd), plants)

    def bwd(h):
        return {"Eo": np.concatenate([nf.matmul_fast(inst(h["E"], i, n_out), f64(h["W"]).T) for i in range(n)],
                                     axis=1)}, None, None

    e_sites = [(0, 0), (rows - 1, n * n_out - 1), (rows // 2, n_out + n_out - 1), (32, 2 * n_out), (5, n_out + 6)]
    plants = [("E", r, c, v) for r, c in e_sites for v in VALUES]
    plants += [("W", r, c, v) for _, r, c in plant_sites(n_in, n_out, 1)[:6] for v in VALUES]
    row_sweep("shared_bwd", layout, dict(E=E, W=W), ("E", "W"), ("Eo",), dict(Eo=(rows, n * n_in)),
              lambda v: L.tnet_shared_bwd(v["E"].ptr, v["E"].dim, v["W"].ptr, v["W"].dim, n, v["Eo"].ptr, v["Eo"].dim,
                                          S()), quiet(bwd), plants)

    scale, mmt, l2 = -0.3 / (rows * n), 0.5, -1e-4

    def grads(h):
        gw = sum(nf.matmul_fast(inst(h["X"], i, n_in).T, inst(h["Es"], i, n_out)) for i in range(n))
        gb = sum(inst(h["Es"], i, n_out).sum(axis=0, keepdims=True) for i in range(n))
        return gw, gb

    def upd(h):
        gw, gb = grads(h)
        c, cbr = gw + mmt * f64(h["corr"]), gb + mmt * f64(h["cb"])
        w = f64(h["W"]) + scale * c
        return {"W": w + l2 * w, "corr": c, "b": f64(h["b"]) + scale * cbr, "cb": cbr}, None, None

    plants = [("X", r, c, v) for r, c in x_sites for v in VALUES] + [("Es", r, c, v) for r, c in e_sites for v in VALUES]
    plants += [("W", 3, 4, v) for v in VALUES] + [("corr", n_in - 1, n_out - 1, NAN), ("cb", 0, 2, NAN), ("b", 0, 1, NAN)]
    io = ("W", "corr", "b", "cb")
    row_sweep("shared_update", layout, dict(X=X, Es=Es, W=W, corr=corr, b=b, cb=cb), ("X", "Es") + io, io, {},
              lambda v: L.tnet_shared_update(v["X"].ptr, v["X"].dim, v["Es"].ptr, v["Es"].dim, n, v["W"].ptr, v["W"].dim,
                                             v["corr"].ptr, v["corr"].stride, v["b"].ptr, v["cb"].ptr, scale, mmt, l2,
                                             S()), quiet(upd), plants)

    def grad(h):
        gw, gb = grads(h)
        return {"G": gw, "gB": gb}, None, None

    plants = [("X", r, c, v) for r, c in x_sites for v in VALUES] + [("Es", r, c, v) for r, c in e_sites for v in VALUES]
    row_sweep("shared_grad", layout, dict(X=X, Es=Es), ("X", "Es"), ("G", "gB"), dict(G=(n_in, n_out), gB=(1, n_out)),
              lambda v: L.tnet_shared_grad(v["X"].ptr, v["X"].dim, v["Es"].ptr, v["Es"].dim, n, v["G"].ptr, v["G"].dim,
                                           v["gB"].ptr, S()), quiet(grad), plants)


@pytest.mark.parametrize("layout", ["tight", "shifted"])
def test_discrete_layer_nonfinite(layout):
    """gemm_discrete.hip at the smallest case of its views test (33 rows; blocks 39 -> 10, 1 -> 7, 5 -> 3): a plant in
    block k of X or E stays in block k of the forward's / backward's output, one in W_k[i, j] (in the packed buffer)
    reaches column j of block k; the update's X[r, block k, i] reaches row i of W_k and nothing else, E[r, block k, j]
    column j of W_k and its bias element"""
    from tnet_amd import DiscretePlan
    rows, blocks = 33, ((39, 10), (1, 7), (5, 3))
    plan = DiscretePlan(blocks)
    n_in, n_out = sum(b[0] for b in blocks), sum(b[1] for b in blocks)
    io_, oo_ = np.cumsum([0] + [b[0] for b in blocks]), np.cumsum([0] + [b[1] for b in blocks])
    g = np.random.default_rng(1500)
    X = g.standard_normal((rows, n_in)).astype(np.float32)
    E = g.standard_normal((rows, n_out)).astype(np.float32)
    Es = (E * np.float32(0.01)).astype(np.float32)
    Ws = [(g.standard_normal(b) * 0.1).astype(np.float32) for b in blocks]
    corrs = [(g.standard_normal(b) * 0.01).astype(np.float32) for b in blocks]
    b, cb = vec(g, n_out), vec(g, n_out, 0.01)
    nf.check_conditions(multiplied=[X, E, Es] + Ws, others=[b, cb] + corrs)
    Wp, Cp = plan.pack(Ws).reshape(1, -1), plan.pack(corrs).reshape(1, -1)
    L = lib()
    lay = {"Wp": "tight", "Cp": "tight"}

    def at(k, i, j):
        """the packed position of W_k[i, j]"""
        off, ld = plan.layout[k]
        return off + i * ld + j

    def blocks_of(h, key="Wp"):
        return [f64(w) for w in plan.unpack(np.asarray(h[key]).reshape(-1))]

    def packed(Ms):
        return f64(plan.pack(Ms)).reshape(1, -1)

    def fwd(h):
        Wk = blocks_of(h)
        return {"Y": np.concatenate([nf.matmul_fast(f64(h["X"])[:, io_[k]:io_[k + 1]], Wk[k]) for k in range(len(blocks))],
                                    axis=1) + f64(h["b"])}, None, None

    x_sites = [(0, 0), (rows - 1, n_in - 1), (5, 38), (32, 39), (7, 41), (rows // 2, 36)]
    e_sites = [(0, 0), (rows - 1, n_out - 1), (5, 9), (32, 10), (7, 17), (rows // 2, 16)]
    w_sites = [at(0, 0, 0), at(0, 38, 9), at(0, 36, 3), at(1, 0, 6), at(2, 4, 2), at(2, 0, 0)]
    w_plants = [("Wp", 0, c, v) for c in w_sites for v in VALUES]
    row_sweep("discrete_fwd", layout, dict(X=X, Wp=Wp, b=b), ("X", "Wp", "b"), ("Y",), dict(Y=(rows, n_out)),
              lambda v: L.tnet_discrete_fwd(v["X"].ptr, v["X"].dim, v["Wp"].ptr, plan.ptr, v["b"].ptr, v["Y"].ptr,
                                            v["Y"].dim, S()), quiet(fwd),
              [("X", r, c, v) for r, c in x_sites for v in VALUES] + w_plants + [("b", 0, 10, NAN)], layouts=lay)

    def bwd(h):
        Wk = blocks_of(h)
        return {"Eo": np.concatenate([nf.matmul_fast(f64(h["E"])[:, oo_[k]:oo_[k + 1]], Wk[k].T)
                                      for k in range(len(blocks))], axis=1)}, None, None

    row_sweep("discrete_bwd", layout, dict(E=E, Wp=Wp), ("E", "Wp"), ("Eo",), dict(Eo=(rows, n_in)),
              lambda v: L.tnet_discrete_bwd(v["E"].ptr, v["E"].dim, v["Wp"].ptr, plan.ptr, v["Eo"].ptr, v["Eo"].dim, S()),
              quiet(bwd), [("E", r, c, v) for r, c in e_sites for v in VALUES] + w_plants, layouts=lay)

    scale, mmt, l2 = -0.3 / rows, 0.5, -1e-4

    def grads(h):
        gw = [nf.matmul_fast(f64(h["X"])[:, io_[k]:io_[k + 1]].T, f64(h["Es"])[:, oo_[k]:oo_[k + 1]])
              for k in range(len(blocks))]
        return gw, f64(h["Es"]).sum(axis=0, keepdims=True)

    def upd(h):
        gw, gb = grads(h)
        Wk, Ck = blocks_of(h), blocks_of(h, "Cp")
        cs = [gw[k] + mmt * Ck[k] for k in range(len(blocks))]
        ws = [Wk[k] + scale * cs[k] for k in range(len(blocks))]
        cbr = gb + mmt * f64(h["cb"])
        return {"Wp": packed([w + l2 * w for w in ws]), "Cp": packed(cs), "b": f64(h["b"]) + scale * cbr,
                "cb": cbr}, None, None

    xe = [("X", r, c, v) for r, c in x_sites for v in VALUES] + [("Es", r, c, v) for r, c in e_sites for v in VALUES]
    io = ("Wp", "Cp", "b", "cb")
    row_sweep("discrete_update", layout, dict(X=X, Es=Es, Wp=Wp, Cp=Cp, b=b, cb=cb), ("X", "Es") + io, io, {},
              lambda v: L.tnet_discrete_update(v["X"].ptr, v["X"].dim, v["Es"].ptr, v["Es"].dim, plan.ptr, v["Wp"].ptr,
                                               v["Cp"].ptr, v["b"].ptr, v["cb"].ptr, scale, mmt, l2, S()),
              quiet(upd), xe + w_plants[:6] + [("Cp", 0, at(2, 4, 2), NAN), ("cb", 0, 16, NAN)], layouts=lay)

    def grad(h):
        gw, gb = grads(h)
        return {"Gp": packed(gw), "gB": gb}, None, None

    row_sweep("discrete_grad", layout, dict(X=X, Es=Es), ("X", "Es"), ("Gp", "gB"),
              dict(Gp=(1, plan.floats), gB=(1, n_out)),
              lambda v: L.tnet_discrete_grad(v["X"].ptr, v["X"].dim, v["Es"].ptr, v["Es"].dim, plan.ptr, v["Gp"].ptr,
                                             v["gB"].ptr, S()), quiet(grad), xe, layouts={"Gp": "tight"})


@pytest.mark.parametrize("layout", ["tight", "shifted"])
@pytest.mark.parametrize("form", [0x1, 0x2, 0x21, 0x22])  # test_gpu_sparse.py: single, sliced, and their 128 tiles
def test_sparse_layer_nonfinite(form, layout):
    """gemm_sparse.hip at the smallest case of its views test (33 x 39 x 10, a third of the weights alive), under the
    four forms of the fused update: X[r, i] reaches row i of corrW and accu, and of W only where the mask is set
    (W under a zero mask is exactly 0 by selection, also when its gradient is NaN); E[r, c] column c and the bias;
    tnet_sparse_grad's G = X^T E row i / column c"""
    import test_gpu_sparse as tp
    rows, n_in, n_out = 33, 39, 10
    X, E, W, corr, accu, mask, b, cb = tp.inputs(rows, n_in, n_out, 0.3)
    scale, mmt, l2 = -0.3 / rows, 0.5, -1e-4
    l1c = float(np.quantile(np.abs(W[mask != 0]), 1 / 3))
    nf.check_conditions(multiplied=[X, E], others=[W, corr, accu, b, cb])
    bits = tp.pack_host(mask, (n_out + 31) // 32, fill=0).view(np.int32)  # the view's stride is the kernel's ldmask
    host = dict(X=X, E=E, W=W, corr=corr, accu=accu, b=b.reshape(1, -1), cb=cb.reshape(1, -1), bits=bits)
    L = lib()

    def upd(h):
        r = tp.update_ref(np.asarray(h["X"]), np.asarray(h["E"]), f64(h["W"]), f64(h["corr"]), f64(h["accu"]), mask,
                          f64(h["b"])[0], f64(h["cb"])[0], scale, mmt, l1c, l2)
        return {"W": r["W"], "corr": r["corr"], "accu": r["accu"], "b": r["b"][None, :], "cb": r["cb"][None, :]}, None, None

    def call(v):
        L.tnet_sparse_update_form(form)
        try:
            return L.tnet_sparse_update(v["X"].ptr, v["X"].dim, v["E"].ptr, v["E"].dim, v["W"].ptr, v["W"].dim,
                                        v["corr"].ptr, v["corr"].stride, v["accu"].ptr, v["accu"].stride, v["bits"].ptr,
                                        v["bits"].stride, v["b"].ptr, v["cb"].ptr, scale, mmt, l1c, l2, S())
        finally:
            L.tnet_sparse_update_form(0)

    dead = tuple(int(i) for i in np.argwhere(mask == 0)[0])
    live = tuple(int(i) for i in np.argwhere(mask != 0)[-1])
    plants = [("X", r, c, v) for _, r, c in plant_sites(rows, n_in, 0) for v in VALUES]
    plants += [("E", r, c, v) for _, r, c in plant_sites(rows, n_out, 0) for v in VALUES]
    plants += [(k, *at, v) for k in ("corr", "accu") for at in (dead, live) for v in VALUES]
    plants += [("W", *live, v) for v in VALUES] + [("cb", 0, 3, NAN), ("b", 0, n_out - 1, NAN)]
    io = ("W", "corr", "accu", "b", "cb")
    clean = row_sweep(f"sparse_update form {form:#x}", layout, host, ("X", "E", "bits") + io, io, {}, call, quiet(upd),
                      plants, layouts={"bits": "tight"})
    assert (clean["W"][mask == 0] == 0).all()
    if form == 0x1:
        row_sweep("sparse_grad", layout, dict(X=X, E=E), ("X", "E"), ("G", "gB"), dict(G=(n_in, n_out), gB=(1, n_out)),
                  lambda v: L.tnet_sparse_grad(v["X"].ptr, v["X"].dim, v["E"].ptr, v["E"].dim, v["G"].ptr, v["G"].dim,
                                               v["gB"].ptr, S()),
                  quiet(lambda h: ({"G": nf.matmul_fast(f64(h["X"]).T, h["E"]),
                                    "gB": f64(h["E"]).sum(axis=0, keepdims=True)}, None, None)),
                  [p_ for p_ in plants if p_[0] in ("X", "E")])


# ------------------------------------------------------------------------------------------------------------------
# Part C: row and column kernels
# ------------------------------------------------------------------------------------------------------------------
def row_sweep(what, layout, host, ins, outs, shapes, call, ref, plants, stats=None, atol=None, layouts=None):
    """the sweep for kernels whose plants are listed by hand: plants = [(operand, row, column(s), value)].
    ref(host dict) -> ({out: float64 array}, xent of each row or None, correct of each row or None).  Integer
    outputs are compared for equality; where the restatement stays finite but changes, the softmax tests' rtol 2e-5
    (atol[out], default 1e-9) holds; the totals are read with tnet_stats_fetch."""
    ops = Operands(layout, host, ins, outs, shapes, layouts)

    def launch(w):
        if stats is not None:
            clear(stats)
        return ops.launch(call, w)

    def compare(got, clean, r, rc, w):
        fl = {k: v for k, v in got.items() if v.dtype.kind == "f"}
        for k in fl:
            check_outputs({k: fl[k]}, clean, r[0], rc[0], w, rtol=2e-5, atol=(atol or {}).get(k, 1e-9))
        for k in got:
            if k not in fl:
                np.testing.assert_array_equal(got[k], np.asarray(r[0][k]).reshape(got[k].shape), err_msg=f"{w}: {k}")
        if stats is not None:
            check_totals(stats, r[1], r[2], w)

    rc = ref(host)
    clean = launch(what + ": clean")
    compare(clean, clean, rc, rc, what + ": clean")
    for op, r, c, val in plants:
        w = f"{what}: {val} in {op}[{r}, {c}]"
        ops.plant(op, r, c, val)
        got = launch(w)
        hp = dict(host)
        hp[op] = nf.planted(host[op], r, c, val)
        compare(got, clean, ref(hp), rc, w)
        ops.restore()
    return clean


XENT_COLS = [135, 132, 1028, 4100]  # scalar, one wave cached, four waves a row, the re-reading fallback
XENT_CASES = [(c, "tight") for c in XENT_COLS] + [(132, "offset")]


@functools.lru_cache(maxsize=None)
def xent_case(cols):
    """six rows of logits, labels (row 0 unlabeled, row 3's label away from the planted columns), dense targets
    (one-hot rows 0 and 4, an all-zero row 2, soft rows 1, 3, 5) and the float32 posteriors"""
    g = np.random.default_rng(400 + cols)
    Z = (g.standard_normal((6, cols)) * 3).astype(np.float32)
    lab = g.integers(0, cols, size=6).astype(np.int32)
    lab[0], lab[3] = -1, 5
    D = np.zeros((6, cols), np.float32)
    D[0, lab[1]], D[4, lab[4]] = 1.0, 1.0
    for r in (1, 3, 5):
        D[r] = g.dirichlet(np.ones(cols)).astype(np.float32)
        D[r, lab[r]] += 0.5  # a clear maximum
    Y = nf.softmax_ref(Z).astype(np.float32)
    nf.check_conditions(others=[Z, D, Y])
    for a in (Z, lab, D, Y):
        a.setflags(write=False)
    return Z, lab, D, Y


def logit_plants(cols, lab, op="Z"):
    """a NaN and a +inf (the row becomes NaN: inf - inf) at the first, a middle and the last column, a -inf in a
    non-label column (y exactly 0 there, the rest a proper softmax), a -inf in the label column (cross-entropy
    -log(FLT_MIN)), a whole row of -inf (0 / 0)"""
    at = (0, cols // 2, cols - 1)
    assert lab[3] not in at
    p = [(op, 1, c, NAN) for c in at] + [(op, 2, c, INF) for c in at] + [(op, 3, c, NINF) for c in at]
    return p + [(op, 4, int(lab[4]), NINF), (op, 1, int(lab[1]), NAN), (op, 5, np.arange(cols), NINF)]


@pytest.mark.parametrize("cols,layout", XENT_CASES)
def test_softmax_nonfinite(cols, layout):
    """tnetF_softmax: a planted row changes alone; the other rows of Y are bit-identical to the clean run"""
    Z, lab, D, Y = xent_case(cols)
    L = lib()
    clean = row_sweep("softmax", layout, dict(Z=Z), ("Z",), ("Y",), dict(Y=Z.shape),
                      lambda v: L.tnetF_softmax(v["Y"].ptr, v["Z"].ptr, v["Z"].dim, S()),
                      lambda h: ({"Y": nf.softmax_ref(h["Z"])}, None, None), logit_plants(cols, lab))
    np.testing.assert_allclose(clean["Y"], nf.softmax_ref(Z), rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize("cols,layout", XENT_CASES)
def test_softmax_xent_nonfinite(cols, layout):
    """tnet_softmax_xent from logits and with Z == NULL: the cross-entropy total is NaN exactly when a labelled
    row's label posterior is NaN (87.34 before the clamp kept NaNs), -log(FLT_MIN) for a -inf label logit; `correct`
    is the restatement's (a NaN row matches nothing)"""
    Z, lab, D, Y = xent_case(cols)
    L = lib()
    stats = new_stats()

    def ref_z(h):
        Yr = nf.softmax_ref(h["Z"])
        E, xe, co = nf.xent_labels_ref(Yr, lab)
        return {"Y": Yr, "E": E}, xe, co

    row_sweep("softmax_xent from Z", layout, dict(Z=Z, lab=lab.reshape(1, -1)), ("Z", "lab"), ("Y", "E"),
              dict(Y=Z.shape, E=Z.shape),
              lambda v: L.tnet_softmax_xent(v["Z"].ptr, v["Z"].dim, v["lab"].ptr, v["Y"].ptr, v["Y"].stride, v["E"].ptr,
                                            v["E"].stride, stats.ptr, S()),
              ref_z, logit_plants(cols, lab), stats=stats, atol={"E": 1e-8})

    def ref_y(h):
        E, xe, co = nf.xent_labels_ref(h["Y"], lab)
        return {"E": E}, xe, co

    # Y is the input: E = Y - T element by element, the total through the label column alone
    plants = [("Y", 1, c, v) for c in (0, cols - 1, int(lab[1])) for v in VALUES]
    plants += [("Y", 0, cols // 2, v) for v in VALUES]  # an unlabeled row: no cross-entropy
    row_sweep("softmax_xent Z == NULL", layout, dict(Y=Y, lab=lab.reshape(1, -1)), ("Y", "lab"), ("E",),
              dict(E=Z.shape),
              lambda v: L.tnet_softmax_xent(None, v["Y"].dim, v["lab"].ptr, v["Y"].ptr, v["Y"].stride, v["E"].ptr,
                                            v["E"].stride, stats.ptr, S()),
              ref_y, plants, stats=stats)


@pytest.mark.parametrize("cols,layout", XENT_CASES)
def test_softmax_xent_dense_nonfinite(cols, layout):
    """tnet_softmax_xent_dense: the reference sums d * log(y) over ALL columns, so a NaN (or +inf) posterior under a
    zero target makes the row's cross-entropy NaN (NaN * 0) -- in a one-hot row, an all-zero row and a soft row"""
    Z, lab, D, Y = xent_case(cols)
    L = lib()
    stats = new_stats()

    def ref_z(h):
        Yr = nf.softmax_ref(h["Z"])
        E, xe, co = nf.xent_dense_ref(Yr, h["D"])
        return {"Y": Yr, "E": E}, xe, co

    plants = logit_plants(cols, lab) + [("D", 1, cols // 2, v) for v in VALUES] + [("D", 2, 0, NAN)]
    row_sweep("softmax_xent_dense from Z", layout, dict(Z=Z, D=D), ("Z", "D"), ("Y", "E"), dict(Y=Z.shape, E=Z.shape),
              lambda v: L.tnet_softmax_xent_dense(v["Z"].ptr, v["Z"].dim, v["D"].ptr, v["D"].stride, v["Y"].ptr,
                                                  v["Y"].stride, v["E"].ptr, v["E"].stride, stats.ptr, S()),
              ref_z, plants, stats=stats, atol={"E": 1e-8}, layouts={"D": "offset" if layout == "tight" else "tight"})

    def ref_y(h):
        E, xe, co = nf.xent_dense_ref(h["Y"], h["D"])
        return {"E": E}, xe, co

    zero_col = int(np.flatnonzero(D[4] == 0)[0])
    plants = [("Y", 4, zero_col, v) for v in VALUES] + [("Y", 4, int(lab[4]), v) for v in VALUES]
    plants += [("Y", 2, cols - 1, v) for v in VALUES] + [("Y", 3, 0, v) for v in VALUES]
    row_sweep("softmax_xent_dense Z == NULL", layout, dict(Y=Y, D=D), ("Y", "D"), ("E",), dict(E=Z.shape),
              lambda v: L.tnet_softmax_xent_dense(None, v["Y"].dim, v["D"].ptr, v["D"].stride, v["Y"].ptr,
                                                  v["Y"].stride, v["E"].ptr, v["E"].stride, stats.ptr, S()),
              ref_y, plants, stats=stats)
    # a row with no maximum on either side (NaN throughout Y and D) matches nothing: _check_class's ids -1 / -2
    Dn = D.copy()
    Dn[5] = NAN
    row_sweep("softmax_xent_dense Z == NULL, D row NaN", layout, dict(Y=Y, D=Dn), ("Y", "D"), ("E",), dict(E=Z.shape),
              lambda v: L.tnet_softmax_xent_dense(None, v["Y"].dim, v["D"].ptr, v["D"].stride, v["Y"].ptr,
                                                  v["Y"].stride, v["E"].ptr, v["E"].stride, stats.ptr, S()),
              ref_y, [("Y", 5, np.arange(cols), NAN), ("Y", 5, 0, NAN)], stats=stats)
    assert nf.xent_dense_ref(nf.planted(Y, 5, np.arange(cols), NAN), Dn)[2][5] == 0


BLOCK_DIMS = {"3-5-2": (3, 5, 2), "3x135": (135, 135, 135), "straddle": (255, 2, 255, 513)}


@pytest.mark.parametrize("key,layout", [(k, "tight") for k in BLOCK_DIMS] + [("3x135", "offset")])
def test_block_softmax_nonfinite(key, layout):
    """tnetF_block_softmax, tnet_block_softmax_xent and tnet_block_softmax_bwd: a plant in block b of row r stays in
    block b of row r of Y.  The fused call's E is y - onehot selected to the label's block and +0.0f elsewhere
    (include/tnet_kernels.h), so a NaN outside the label's block reaches neither E nor the cross-entropy, and one
    inside makes both NaN.  tnet_block_softmax_bwd follows tests/blocksoftmax_cases.py's sum rule: a block whose
    error sum is NaN or infinite fails both comparisons, is zeroed and counted as invalid.
    The reference's CPU source on a NaN outside the label's block: BlockSoftmax::BackpropagateFnc forms every
    block's sum, a NaN sum passes neither `sum > -0.1 && sum < 0.1` nor `sum > 0.9 && sum < 1.1`, and the else
    branch raises KALDI_ERR "Invalid sum: nan" (Activation.cc:117-126) with the output already zeroed -- the block's
    error is zero and the run ends, where this library zeroes the block, counts it and goes on."""
    dims = BLOCK_DIMS[key]
    N, rows = sum(dims), 6
    off = np.concatenate([[0], np.cumsum(dims)]).astype(np.int32)
    g = np.random.default_rng(500 + N)
    Z = (g.standard_normal((rows, N)) * 2.5).astype(np.float32)
    lab = g.integers(0, N, size=rows).astype(np.int32)
    lab[0] = -1
    blk = lambda c: int(np.searchsorted(off, c, side="right") - 1)  # noqa: E731
    L = lib()

    def other_block_col(r):
        b = (blk(lab[r]) + 1) % len(dims)
        return int(off[b + 1] - 1)

    # in the label's block (not on the label), on the label, and in another block; an unlabeled row
    plants = [("Z", 1, int(off[blk(lab[1])]) if off[blk(lab[1])] != lab[1] else int(lab[1]), v) for v in VALUES]
    plants += [("Z", 2, int(lab[2]), v) for v in VALUES] + [("Z", 3, other_block_col(3), v) for v in VALUES]
    plants += [("Z", 0, N - 1, v) for v in VALUES] + [("Z", 4, 0, NAN), ("Z", 5, N // 2, NAN)]
    host = dict(Z=Z, off=off.reshape(1, -1), lab=lab.reshape(1, -1))
    row_sweep("block_softmax", layout, host, ("Z", "off"), ("Y",), dict(Y=Z.shape),
              lambda v: L.tnetF_block_softmax(v["Y"].ptr, v["Z"].ptr, v["Z"].dim, v["off"].ptr, len(dims), S()),
              lambda h: ({"Y": nf.block_softmax_ref(h["Z"], dims)}, None, None), plants)

    def ref_fused(h):
        Y = nf.block_softmax_ref(h["Z"], dims)
        full, xe, co = nf.xent_labels_ref(Y, lab)
        E = np.zeros_like(Y)
        for r in range(rows):
            if lab[r] >= 0:
                b = blk(lab[r])
                E[r, off[b]:off[b + 1]] = full[r, off[b]:off[b + 1]]
        return {"Y": Y, "E": E}, xe, co

    stats = new_stats()
    clean = row_sweep("block_softmax_xent", layout, host, ("Z", "off", "lab"), ("Y", "E"), dict(Y=Z.shape, E=Z.shape),
                      lambda v: L.tnet_block_softmax_xent(v["Z"].ptr, v["Z"].dim, v["off"].ptr, len(dims), v["lab"].ptr,
                                                          v["Y"].ptr, v["Y"].stride, v["E"].ptr, v["E"].stride,
                                                          stats.ptr, S()),
                      ref_fused, plants, stats=stats, atol={"E": 1e-7})  # E = y - 1 from a float32 y: 6e-8 below 1

    # the sum rule on a dense error Y - T: every block of a labelled row sums to 0 or 1
    Ein = (clean["Y"].astype(np.float64) - (np.arange(N)[None, :] == lab[:, None])).astype(np.float32)
    Ein[0] = 0

    def ref_bwd(h):
        m, inv = nf.block_sum_rule_ref(h["Ein"], dims)
        return {"Eout": m, "inv": np.array([[inv]], np.int32)}, None, None

    plants = [("Ein", r, c, v) for r, c in ((1, int(lab[1])), (3, other_block_col(3)), (5, N - 1)) for v in VALUES]
    row_sweep("block_softmax_bwd", layout, dict(Ein=Ein, off=off.reshape(1, -1), inv=np.zeros((1, 1), np.int32)),
              ("Ein", "off", "inv"), ("Eout", "inv"), dict(Eout=Z.shape),
              lambda v: L.tnet_block_softmax_bwd(v["Ein"].ptr, v["Ein"].dim, v["off"].ptr, len(dims), v["Eout"].ptr,
                                                 v["Eout"].stride, v["inv"].ptr, S()),
              ref_bwd, plants)


# ---- column isolation: a plant in column j changes output j only
@pytest.mark.parametrize("rows", [33, 2049])
@pytest.mark.parametrize("layout", ["tight", "offset", "odd"])
def test_column_kernels_nonfinite(rows, layout):
    """tnetF_add_col_sum, tnet_bias_update, tnet_rbm_bias_update (column sums in 32-row slabs: one column, whichever
    slab the plant is in), tnet_mse (one element of E; the total's class) and tnetF_check_class (one row's match;
    a row that is NaN throughout on both sides has no maximum and matches nothing, cukernels.cu:405)"""
    cols = 77
    g = np.random.default_rng(600 + rows)
    E = g.standard_normal((rows, cols)).astype(np.float32)
    v0, b0, cb0 = (g.standard_normal((1, cols)).astype(np.float32) for _ in range(3))
    L = lib()
    sites = [(r, c) for _, r, c in plant_sites(rows, cols)] + [(rows // 2, 31), (32 if rows > 33 else 31, 32)]
    plants = [("E", r, c, v) for r, c in sites for v in VALUES]
    ws = DeviceArray(1, max(1, L.tnet_col_sum_workspace(MatrixDim(rows, cols, cols)) // 4 + 64), np.float32)

    def colsum(h):
        with np.errstate(all="ignore"):
            return np.asarray(h["E"], np.float64).sum(axis=0, keepdims=True)

    def f32(x):
        with np.errstate(all="ignore"):
            return np.asarray(np.asarray(x, np.float32), np.float64)

    row_sweep("add_col_sum", layout, dict(E=E, v=v0), ("E", "v"), ("v",), {},
              lambda v: L.tnetF_add_col_sum(0.5, v["E"].ptr, 2.0, v["v"].ptr, v["E"].dim, ws.ptr, S()),
              lambda h: ({"v": 0.5 * colsum(h) + 2.0 * np.asarray(h["v"], np.float64)}, None, None),
              plants + [("v", 0, 5, v) for v in VALUES])
    scale, mmt = -0.01, 0.9

    def ref_bias(h):
        with np.errstate(all="ignore"):
            c = f32(colsum(h)) + mmt * np.asarray(h["cb"], np.float64)
            return {"b": np.asarray(h["b"], np.float64) + scale * c, "cb": c}, None, None

    row_sweep("bias_update", layout, dict(E=E, b=b0, cb=cb0), ("E", "b", "cb"), ("b", "cb"), {},
              lambda v: L.tnet_bias_update(v["E"].ptr, v["E"].dim, v["b"].ptr, v["cb"].ptr, None, scale, mmt, ws.ptr,
                                           S()),
              ref_bias, plants + [("cb", 0, 7, v) for v in VALUES] + [("b", 0, 9, NAN)])
    neg_from = (rows // 2) | 5
    sg = np.where(np.arange(rows) < neg_from, 1.0, -1.0)[:, None]

    def ref_rbm(h):
        with np.errstate(all="ignore"):
            s = f32((np.asarray(h["E"], np.float64) * sg).sum(axis=0, keepdims=True))
            c = 0.5 * np.asarray(h["cb"], np.float64) + (0.1 / rows) * s
            return {"b": np.asarray(h["b"], np.float64) + c, "cb": c}, None, None

    row_sweep("rbm_bias_update", layout, dict(E=E, b=b0, cb=cb0), ("E", "b", "cb"), ("b", "cb"), {},
              lambda v: L.tnet_rbm_bias_update(v["E"].ptr, v["E"].dim, neg_from, v["b"].ptr, v["cb"].ptr, 0.1 / rows, 0.5,
                                               ws.ptr, S()),
              ref_rbm, plants)

    D = g.standard_normal((rows, cols)).astype(np.float32)
    stats = new_stats()

    def ref_mse(h):
        with np.errstate(all="ignore"):
            e = np.asarray(h["E"], np.float64) - np.asarray(h["D"], np.float64)
            return {"Eo": e}, (e * e).sum(axis=1), np.zeros(rows)

    row_sweep("mse", layout, dict(E=E, D=D), ("E", "D"), ("Eo",), dict(Eo=E.shape),
              lambda v: L.tnet_mse(v["E"].ptr, v["E"].dim, v["D"].ptr, v["D"].stride, v["Eo"].ptr, v["Eo"].stride,
                                   stats.ptr, S()),
              ref_mse, plants[:12] + [("D", rows - 1, 3, v) for v in VALUES], stats=stats)

    des = np.zeros((rows, cols), np.float32)
    des[np.arange(rows), g.integers(0, cols, rows)] = 1.0
    allnan = [("E", 2, np.arange(cols), NAN)]
    desn = des.copy()
    desn[2] = NAN
    for d_host, pl in ((des, plants[:12] + allnan), (desn, allnan)):
        row_sweep("check_class", layout, dict(E=E, des=d_host), ("E", "des"), ("match",),
                  dict(match=(1, rows, np.int32)),
                  lambda v: L.tnetF_check_class(v["E"].ptr, v["des"].ptr, v["match"].ptr, v["E"].dim, S()),
                  lambda h: ({"match": nf.check_class_ref(h["E"], h["des"])}, None, None), pl,
                  layouts={"match": "tight"})


class SgdSeg(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("corr", C.c_void_p), ("n", C.c_long), ("l2", C.c_float)]


SGD_SEGS = {"three": [(0, 4), (5, 4091), (4096, 1028)],  # element offsets 0, 5 and 4096; n % 4 of 0, 3 and 0
            "ten": [(k * 120 + (k % 3), 100 + k) for k in range(10)]}  # the second launch of 8 + 2


@pytest.mark.parametrize("layout", ["tight", "offset"])
@pytest.mark.parametrize("mmt", [0.0, 0.9])
@pytest.mark.parametrize("key", list(SGD_SEGS))
def test_sgd_update_nonfinite(key, mmt, layout):
    """tnet_sgd_update segment by segment and tnet_sgd_update_multi in one call, the segments packed into one
    poisoned buffer each for p, g and corr (NULL at mmt 0): one plant stays in one element of p / corr, the other
    segments and the gaps between them are bit-identical.  An infinite p becomes NaN in the decay pass (inf - inf)."""
    segs = SGD_SEGS[key]
    n_all = max(o + n for o, n in segs)
    g_ = np.random.default_rng(700 + n_all)
    host = dict(p=g_.standard_normal((1, n_all)).astype(np.float32), g=g_.standard_normal((1, n_all)).astype(np.float32))
    if mmt:
        host["corr"] = (g_.standard_normal((1, n_all)) * 0.1).astype(np.float32)
    scale, l2 = -0.01, -1e-4
    io = ("p", "corr") if mmt else ("p",)
    L = lib()

    def ref(h):
        out = {k: np.array(h[k], np.float64) for k in io}
        with np.errstate(all="ignore"):
            for o, n in segs:
                c = np.asarray(h["g"], np.float64)[0, o:o + n]
                if mmt:
                    c = c + mmt * np.asarray(h["corr"], np.float64)[0, o:o + n]
                    out["corr"][0, o:o + n] = c
                w = np.asarray(h["p"], np.float64)[0, o:o + n] + scale * c
                out["p"][0, o:o + n] = w + l2 * w
        return out, None, None

    def single(v):
        for o, n in segs:
            st = L.tnet_sgd_update(v["p"].ptr + 4 * o, v["g"].ptr + 4 * o, v["corr"].ptr + 4 * o if mmt else None, n,
                                   scale, mmt, l2, S())
            if st:
                return st
        return 0

    def multi(v):
        arr = (SgdSeg * len(segs))(*[SgdSeg(v["p"].ptr + 4 * o, v["g"].ptr + 4 * o,
                                            v["corr"].ptr + 4 * o if mmt else None, n, l2) for o, n in segs])
        return L.tnet_sgd_update_multi(C.cast(arr, C.c_void_p), len(segs), scale, mmt, S())

    at = sorted({segs[0][0], segs[0][0] + segs[0][1] - 1, segs[1][0], segs[1][0] + segs[1][1] - 1, segs[-1][0],
                 segs[-1][0] + segs[-1][1] - 1, segs[len(segs) // 2][0] + 3})
    plants = [(op, 0, c, v) for op in ("g",) + io for c in at for v in VALUES]
    for name, call in (("sgd_update", single), ("sgd_update_multi", multi)):
        row_sweep(f"{name} {key} mmt {mmt}", layout, host, ("g",) + io, io, {}, call, ref, plants)


@pytest.mark.parametrize("rows,cols,layout", [(36, 132, "tight"), (36, 132, "offset"), (37, 131, "odd")])
def test_map_ops_nonfinite(rows, cols, layout):
    """the map ops of elementwise.hip: a planted element of the matrix changes that element of the result, one of a
    column / row scale vector its column / row; a NaN under a zero mask becomes 0 (tnetF_apply_mask selects)"""
    g = np.random.default_rng(800 + cols)
    X = g.standard_normal((rows, cols)).astype(np.float32)
    A = g.standard_normal((rows, cols)).astype(np.float32)
    P = (np.abs(X) + np.float32(1e-3)).astype(np.float32)
    Ys = np.clip(nf.sigmoid_ref(A), 0.05, 0.95).astype(np.float32)
    sc, sr = g.standard_normal((1, cols)).astype(np.float32), g.standard_normal((1, rows)).astype(np.float32)
    mask = (g.random((rows, cols)) < 0.5).astype(np.float32)
    mask[0, 0], mask[rows - 1, cols - 1] = 0.0, 1.0
    nf.check_conditions(multiplied=[X, A, sc, sr], sigmoids=[Ys], others=[P])
    L = lib()
    sites = [(r, c) for _, r, c in plant_sites(rows, cols)]

    def all_values(op, where):
        return [(op, r, c, v) for r, c in where for v in VALUES]

    def f64(a):
        return np.asarray(a, np.float64)

    def run(what, host, ins, outs, shapes, call, ref, plants):
        def ref_(h):
            with np.errstate(all="ignore"):
                return ref(h), None, None
        row_sweep(what, layout, host, ins, outs, shapes, call, ref_, plants)

    run("apply_log", dict(M=P), ("M",), ("M",), {}, lambda v: L.tnetF_apply_log(v["M"].ptr, v["M"].dim, S()),
        lambda h: {"M": np.log(f64(h["M"]))}, all_values("M", sites))
    run("log_elem", dict(M=P), ("M",), ("M",), {}, lambda v: L.tnetF_log_elem(v["M"].ptr, v["M"].dim, S()),
        lambda h: {"M": nf._log_clamped(h["M"])}, all_values("M", sites))
    l1 = np.float32(0.3)
    run("apply_l1", dict(M=X), ("M",), ("M",), {}, lambda v: L.tnetF_apply_l1(v["M"].ptr, l1, v["M"].dim, S()),
        lambda h: {"M": np.where(np.abs(f64(h["M"])) < l1, 0.0, np.where(f64(h["M"]) > 0, f64(h["M"]) - l1,
                                                                        f64(h["M"]) + l1))}, all_values("M", sites))
    run("scale_cols", dict(M=X, s=sc), ("M", "s"), ("M",), {},
        lambda v: L.tnetF_scale_cols(v["M"].ptr, v["s"].ptr, v["M"].dim, S()),
        lambda h: {"M": f64(h["M"]) * f64(h["s"])}, all_values("M", sites) + all_values("s", [(0, 0), (0, cols - 1)]))
    run("scale_rows", dict(M=X, s=sr), ("M", "s"), ("M",), {},
        lambda v: L.tnetF_scale_rows(v["M"].ptr, v["s"].ptr, v["M"].dim, S()),
        lambda h: {"M": f64(h["M"]) * f64(h["s"]).T}, all_values("M", sites) + all_values("s", [(0, 0), (0, rows - 1)]))
    run("mul_elem", dict(M=X, A=A), ("M", "A"), ("M",), {},
        lambda v: L.tnetF_mul_elem(v["M"].ptr, v["A"].ptr, v["A"].stride, v["M"].dim, S()),
        lambda h: {"M": f64(h["M"]) * f64(h["A"])}, all_values("M", sites[:2]) + all_values("A", sites))
    run("add_scaled", dict(M=X, A=A), ("M", "A"), ("M",), {},
        lambda v: L.tnetF_add_scaled(2.0, v["A"].ptr, v["A"].stride, 0.5, v["M"].ptr, v["M"].dim, S()),
        lambda h: {"M": 2.0 * f64(h["A"]) + 0.5 * f64(h["M"])}, all_values("M", sites[:2]) + all_values("A", sites))
    run("add_scaled_row", dict(M=X, s=sc), ("M", "s"), ("M",), {},
        lambda v: L.tnetF_add_scaled_row(2.0, v["s"].ptr, 0.5, v["M"].ptr, v["M"].dim, S()),
        lambda h: {"M": 2.0 * f64(h["s"]) + 0.5 * f64(h["M"])}, all_values("M", sites) + all_values("s", [(0, 3)]))
    run("sigmoid", dict(M=X), ("M",), ("Y",), dict(Y=X.shape),
        lambda v: L.tnetF_sigmoid(v["Y"].ptr, v["M"].ptr, v["M"].dim, S()),
        lambda h: {"Y": nf.sigmoid_ref(h["M"])}, all_values("M", sites))
    run("diff_sigmoid", dict(E=X, Y=Ys), ("E", "Y"), ("Eo",), dict(Eo=X.shape),
        lambda v: L.tnetF_diff_sigmoid(v["Eo"].ptr, v["E"].ptr, v["Y"].ptr, v["E"].dim, S()),
        lambda h: {"Eo": f64(h["Y"]) * (1.0 - f64(h["Y"])) * f64(h["E"])}, all_values("E", sites) + all_values("Y", sites))
    # a NaN under a zero mask becomes 0 (the result there is bit-identical to the clean run's +0.0f); under a one it
    # stays; a non-finite mask entry is not zero: the element passes
    zero, one = (0, 0), (rows - 1, cols - 1)
    run("apply_mask", dict(M=X, mask=mask), ("M", "mask"), ("M",), {},
        lambda v: L.tnetF_apply_mask(v["M"].ptr, v["mask"].ptr, v["M"].dim, v["mask"].dim, S()),
        lambda h: {"M": np.where(f64(h["mask"]) == 0, 0.0, f64(h["M"]))},
        all_values("M", [zero, one]) + all_values("mask", [zero, one]))


# ------------------------------------------------------------------------------------------------------------------
# Part D: single-frame kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tight", "offset"])
@pytest.mark.parametrize("K,N", [(65, 63), (130, 68)])
def test_gemv_rowvec_nonfinite(K, N, layout):
    """tnet_gemv_rowvec: W[k, n] and b[n] reach y[n] (and W[k, n] the workspace partial of k's 64-row slice, column
    n); v[k] reaches every column"""
    g = np.random.default_rng(900 + K)
    host = dict(v=vec(g, K), W=(g.standard_normal((K, N)) * 0.05).astype(np.float32), b=vec(g, N))
    nf.check_conditions(multiplied=[host["v"], host["W"]], others=[host["b"]])
    slices = -(-K // 64)
    L = lib()
    for act in (0, 1):
        def ref(h, act=act):
            part = np.stack([f64(h["v"])[0, k:k + 64] @ f64(h["W"])[k:k + 64] for k in range(0, K, 64)])
            a = f64(h["b"]) + nf.matmul_fast(h["v"], h["W"])
            return {"y": nf.sigmoid_ref(a) if act else a, "ws": part.reshape(1, -1)}, None, None

        plants = [("W", r, c, v) for _, r, c in plant_sites(K, N, 0) for v in VALUES]
        plants += [("v", 0, c, v) for c in (0, 63, K - 1) for v in VALUES] + [("b", 0, N - 1, v) for v in VALUES]
        row_sweep(f"gemv_rowvec act {act}", layout, host, ("v", "W", "b"), ("y", "ws"),
                  dict(y=(1, N), ws=(1, slices * N)),
                  lambda v, act=act: L.tnet_gemv_rowvec(v["v"].ptr, K, v["W"].ptr, v["W"].stride, v["b"].ptr, v["y"].ptr,
                                                        N, act, v["ws"].ptr, S()), quiet(ref), plants)


@pytest.mark.parametrize("layout", ["tight", "offset"])
@pytest.mark.parametrize("n", [13, 68, 1028])
def test_gemv_rows_nonfinite(n, layout):
    """tnet_gemv_rows: the rows of W outside [r0, r0 + nrows) hold +inf and reach nothing; beta == 0 over a y full of
    NaN reads no y; W[r0 + i, c] reaches y[i], x[c] every row"""
    r0, nrows = 2, 7
    g = np.random.default_rng(950 + n)
    W = g.standard_normal((r0 + nrows + 1, n)).astype(np.float32)
    W[:r0], W[r0 + nrows:] = np.inf, np.inf
    x, s = vec(g, n), g.uniform(0.05, 0.95, (1, nrows)).astype(np.float32)
    L = lib()
    plants = [("W", r0 + i, c, v) for i, c in ((0, 0), (nrows - 1, n - 1), (3, n - 4), (3, n // 2)) for v in VALUES]
    plants += [("x", 0, c, v) for c in (0, n - 1) for v in VALUES]
    for beta, y0 in ((0.0, np.full((1, nrows), np.nan, np.float32)), (0.5, vec(g, nrows))):
        def ref(h, beta=beta):
            dot = (f64(h["W"])[r0:r0 + nrows] @ f64(h["x"])[0])[None, :]
            return {"y": ((beta * f64(h["y"]) if beta else 0.0) + dot) * f64(s) * (1 - f64(s))}, None, None

        clean = row_sweep(f"gemv_rows n {n} beta {beta}", layout, dict(W=W, x=x, y=y0, s=s), ("W", "x", "y", "s"),
                          ("y",), {},
                          lambda v, beta=beta: L.tnet_gemv_rows(v["W"].ptr, v["W"].stride, r0, nrows, n, v["x"].ptr,
                                                                v["y"].ptr, beta, v["s"].ptr, S()),
                          quiet(ref), plants + ([("y", 0, 3, v) for v in VALUES] if beta else []))
        np.testing.assert_allclose(clean["y"], quiet(ref)(dict(W=W, x=x, y=y0, s=s))[0]["y"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("layout", ["tight", "offset"])
@pytest.mark.parametrize("mmt", [0.0, 0.9])
@pytest.mark.parametrize("n_in,n_out", [(13, 7), (5, 68), (5, 260)])
def test_affine_bwd_update_row_nonfinite(n_in, n_out, mmt, layout):
    """tnet_affine_bwd_update_row: x[i] reaches row i of W / corrW, e[j] column j, b[j], corr_b[j] and every
    e_out / d_out (e_out = W e); W[i, j] its own element and e_out[i] / d_out[i]"""
    g = np.random.default_rng(1000 + n_out)
    host = dict(x=g.uniform(0.05, 0.95, (1, n_in)).astype(np.float32), e=vec(g, n_out, 0.1),
                W=(g.standard_normal((n_in, n_out)) * 0.1).astype(np.float32), b=vec(g, n_out),
                s=g.uniform(0.05, 0.95, (1, n_in)).astype(np.float32))
    io = ("W", "b")
    if mmt:
        host.update(corr=g.standard_normal((n_in, n_out)).astype(np.float32), cb=vec(g, n_out))
        io += ("corr", "cb")
    nf.check_conditions(multiplied=[host["x"], host["e"], host["W"]], sigmoids=[host["s"]])
    scale, l2 = -0.02, -1e-4
    L = lib()

    def ref(h):
        c = np.outer(f64(h["x"])[0], f64(h["e"])[0])
        gb = f64(h["e"])
        if mmt:
            c, gb = c + mmt * f64(h["corr"]), gb + mmt * f64(h["cb"])
        w = f64(h["W"]) + scale * c
        er = (f64(h["W"]) @ f64(h["e"])[0])[None, :]
        out = {"W": w + l2 * w, "b": f64(h["b"]) + scale * gb, "eo": er, "do": er * f64(h["s"]) * (1 - f64(h["s"]))}
        if mmt:
            out.update(corr=c, cb=gb)
        return out, None, None

    def call(v):
        C_, cb = v.get("corr"), v.get("cb")
        return L.tnet_affine_bwd_update_row(v["x"].ptr, n_in, v["e"].ptr, n_out, v["W"].ptr, v["W"].stride,
                                            C_.ptr if C_ else None, C_.stride if C_ else 0, v["b"].ptr,
                                            cb.ptr if cb else None, scale, mmt, l2, v["eo"].ptr, v["s"].ptr, v["do"].ptr,
                                            S())

    plants = [("x", 0, c, v) for c in (0, n_in - 1) for v in VALUES]
    plants += [("e", 0, c, v) for c in (0, n_out - 1, n_out // 2) for v in VALUES]
    plants += [("W", r, c, v) for _, r, c in plant_sites(n_in, n_out, 1)[:5] for v in VALUES]
    plants += [("s", 0, 1, NAN), ("b", 0, 2, NAN)] + ([("corr", 1, 3, v) for v in VALUES] if mmt else [])
    row_sweep(f"affine_bwd_update_row mmt {mmt}", layout, host, ("x", "e", "s") + io, io + ("eo", "do"),
              dict(eo=(1, n_in), do=(1, n_in)), call, quiet(ref), plants)


@pytest.mark.parametrize("layout", ["tight", "offset"])
@pytest.mark.parametrize("K,N", [(100, 300), (8, 1028)])
def test_gemv_rowvec_softmax_xent_nonfinite(K, N, layout):
    """the single-frame top layer: the cross-entropy in stats slot 0 is NaN when the frame's label posterior is NaN
    (gemv.hip clamped with fmaxf too), 0 for an unlabeled frame; W[k, n] / b[n] reach z[n] and, through the sum, y
    and e; a -inf logit is an exact zero posterior"""
    g = np.random.default_rng(1100 + N)
    host = dict(v=vec(g, K), W=(g.standard_normal((K, N)) * 0.1).astype(np.float32), b=vec(g, N))
    host["b"][0, N // 2] += 8.0  # a clear maximum
    nf.check_conditions(multiplied=[host["v"], host["W"]], others=[host["b"]])
    slices = -(-K // 64)
    L = lib()
    stats = new_stats()
    for t in (7, -1):
        lab = np.array([t], np.int32)

        def ref(h, lab=lab):
            z = f64(h["b"]) + nf.matmul_fast(h["v"], h["W"])
            y = nf.softmax_ref(z)
            e, xe, co = nf.xent_labels_ref(y, lab)
            return {"z": z, "y": y, "e": e}, xe, co

        def call(v):
            return L.tnet_gemv_rowvec_softmax_xent(v["v"].ptr, K, v["W"].ptr, v["W"].stride, v["b"].ptr, v["z"].ptr,
                                                   v["y"].ptr, v["e"].ptr, N, v["lab"].ptr, stats.ptr, v["ws"].ptr, S())

        plants = [("v", 0, K - 1, v) for v in VALUES] + [("W", K - 1, 7, v) for v in VALUES]
        plants += [("W", 0, N - 1, v) for v in VALUES] + [("b", 0, 7, v) for v in VALUES] + [("b", 0, 0, NINF)]
        hl = dict(host, lab=lab.reshape(1, 1))
        ops_outs = ("z", "y", "e")
        # (the workspace partials are covered by test_gemv_rowvec_nonfinite; here it is scratch outside the sweep)
        ws = PoisonView.empty(1, slices * N, layout)
        row_sweep(f"gemv_rowvec_softmax_xent label {t}", layout, hl, ("v", "W", "b", "lab"), ops_outs,
                  dict(z=(1, N), y=(1, N), e=(1, N)),
                  lambda v, ws=ws: call({**v, "ws": ws}), quiet(ref), plants, stats=stats, atol={"e": 1e-8})


@pytest.mark.parametrize("layout", ["tight", "offset"])
@pytest.mark.parametrize("nIn,H,N", [(8, 64, 5), (30, 70, 300)])
def test_rnn_out_chain_nonfinite(nIn, H, N, layout):
    """tnet_rnn_out_full -> tnet_rnn_out_bwd_update at the smallest shapes of test_rnn_out_full_views: a plant in
    bo[j] or Wo[k, j] reaches z[j] alone (h and the other logits bit-identical), one in hb[k] reaches h[k] and, through
    it, every logit; with a NaN in z the posterior is NaN and the cross-entropy in stats slot 0 is NaN for a labelled
    frame, 0 for an unlabeled one"""
    g = np.random.default_rng(1600 + N)
    hs = -(-(nIn + H) // 64)
    host = dict(hpart=(g.standard_normal((1, hs * H)) / np.sqrt(hs)).astype(np.float32), hb=vec(g, H),
                Wo=(g.standard_normal((H, N)) * 0.05).astype(np.float32), bo=vec(g, N))
    host["bo"][0, 1] += 6.0  # a clear maximum
    nf.check_conditions(multiplied=[host["Wo"]], others=[host["hpart"], host["hb"], host["bo"]])
    G, L = -(-N // 64), lib()
    smx = PoisonView.empty(1, 2 * G, layout, np.float64)
    ops = Operands(layout, host, ("hpart", "hb", "Wo", "bo"), ("h", "z"), dict(h=(1, H), z=(1, N)))

    def full(v):
        return L.tnet_rnn_out_full(v["hpart"].ptr, hs, v["hb"].ptr, v["h"].ptr, H, v["Wo"].ptr, v["Wo"].stride, N,
                                   v["bo"].ptr, v["z"].ptr, smx.ptr, S())

    def ref(h_):
        with np.errstate(all="ignore"):
            hh = nf.sigmoid_ref(f64(h_["hb"]) + f64(h_["hpart"]).reshape(hs, H).sum(axis=0, keepdims=True))
            return {"h": hh, "z": f64(h_["bo"]) + nf.matmul_fast(hh, h_["Wo"])}

    stats = new_stats()
    key = DeviceArray(1, 1, np.uint64, stride=1)
    rc = ref(host)
    clean = ops.launch(full, "rnn_out_full: clean")
    plants = [("bo", 0, j, v) for j in (0, N - 1, 3) for v in VALUES]
    plants += [("Wo", k, j, v) for k, j in ((0, 0), (H - 1, N - 1), (H // 2, 3)) for v in VALUES]
    plants += [("hb", 0, H - 1, v) for v in VALUES]
    for t in (3, -1):
        lab = PoisonView.vector(np.array([t], np.int32), layout)
        for op, r, c, val in plants:
            w = f"rnn_out_full label {t}: {val} in {op}[{r}, {c}]"
            ops.plant(op, r, c, val)
            got = ops.launch(full, w)
            hp = dict(host)
            hp[op] = nf.planted(host[op], r, c, val)
            # (hb = -inf: h[k] is exactly 0 and every logit changes, finitely: test_rnn_out_full_views' z bound)
            check_outputs(got, clean, ref(hp), rc, w, rtol=1e-5, atol=1e-5)
            # the backward on what the forward left: z, the softmax pairs and h are its inputs
            ye = Operands(layout, {}, (), ("y", "e"), dict(y=(1, N), e=(1, N)))
            clear(stats)
            check(L.tnet_memset(key.ptr, 0, 8))

            def bwd(v):
                return L.tnet_rnn_out_bwd_update(ops.v["z"].ptr, smx.ptr, G, N, lab.ptr, ops.v["h"].ptr, H,
                                                 ops.v["Wo"].ptr, ops.v["Wo"].stride, None, 0, ops.v["bo"].ptr, None,
                                                 -0.03, 0.0, -1e-5, v["y"].ptr, v["e"].ptr, None, None, stats.ptr,
                                                 key.ptr, 0, S())

            out = ye.launch(bwd, w + " -> rnn_out_bwd_update")
            Y = nf.softmax_ref(got["z"])
            E, xe, co = nf.xent_labels_ref(Y, np.array([t]))
            for k_, r_, atol in (("y", Y, 1e-9), ("e", E, 1e-8)):
                np.testing.assert_array_equal(nf.classes(out[k_]), nf.classes(r_), err_msg=f"{w}: {k_}")
                fin = np.isfinite(r_)
                np.testing.assert_allclose(out[k_][fin], r_[fin], rtol=2e-5, atol=atol, err_msg=f"{w}: {k_}")
            xent = fetch(stats)[0]
            assert nf.classes(np.float64(xent)) == nf.classes(np.float64(xe.sum())), \
                f"{w}: cross-entropy {xent!r}, the restatement gives {xe.sum()!r}"
            if t >= 0 and not np.isfinite(got["z"]).all() and np.isnan(Y).all():
                assert np.isnan(xent), w
            ops.restore()
