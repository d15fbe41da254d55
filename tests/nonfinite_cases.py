"""Non-finite values inside the input matrices (tests/test_nonfinite_cpu.py, tests/test_gpu_nonfinite.py).

The poisoned views of tests/kernel_views.py put NaNs AROUND a matrix.  Here one +inf, -inf or NaN is planted INSIDE an
input, and the output must be non-finite exactly where IEEE arithmetic on the entry point's stated formula makes it so:
the plant's footprint (a row, a column, one slab sum, one block, one element).  Two things make that checkable without
a tolerance:

  * The footprint comes from a float64 restatement run on the planted input, never from the kernel.  The inputs are
    conditioned (check_conditions) so that the restatement's non-finite set is exactly the predicted row / column /
    slab / block: no exact zero in an operand that multiplies the plant (0 * inf would be NaN, a zero weight would
    hide a NaN in a kernel that multiplies instead of selecting -- and also in the restatement), sigmoid outputs well
    inside (0, 1), one plant per call, no finite value above 1e4 (no overflow whose place depends on summation order).
  * Outside the footprint the kernel must return what it returned on the clean input -- the same call with the planted
    element holding the finite value it overwrote -- bit for bit.  A kernel computes an element outside the footprint
    from the same operands in the same order in both runs, so any difference at all is the plant leaking: a clamped
    re-read that is multiplied by zero instead of dropped, a neighbouring row in a fused column sum, a split-K partial
    or a pair launch's other half picking the value up.

  VALUES                                   (+inf, -inf, nan)
  classes(a)                               0 finite, 1 +inf, 2 -inf, 3 nan, elementwise
  footprint_violation(got, clean, ref)     None, or a message naming the first offending element
  assert_footprint(got, clean, ref, what)  (a) ref finite -> got bit-identical to clean; (b) ref not finite -> same class
  softmax_ref, max_id, check_class_ref, xent_labels_ref, xent_dense_ref, block_softmax_ref
                                           float64 restatements that keep the reference's comparisons (cukernels.cu
                                           _softmax: `if (max < x) max = x` from -1e20; _check_class: `if (val > max)`
                                           from id -1 / -2; _log_elem: `if (v < FLT_MIN) v = FLT_MIN`), because numpy's
                                           shortcuts treat a NaN differently (np.argmax picks one)
  plant_sites(R, C, k_axis)                where to plant in an [R x C] operand reduced along k_axis
  check_conditions(...)                    the input conditions above, asserted on the CPU before any GPU call
  rows_of / cols_of / elems_of             predicted footprints as boolean masks
"""
import numpy as np

VALUES = (np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan))
FLT_MIN = float(np.finfo(np.float32).tiny)
FINITE, PINF, NINF, NAN = 0, 1, 2, 3
CLASS_NAMES = ("finite", "+inf", "-inf", "nan")
TILE_DEPTHS = (16, 32, 64)
MAX_FINITE = 1e4
SLAB = 32  # rows of a column-sum slab (tnet_colsum_slabs)
UPDATE_L2 = -1e-4  # the l2 of the affine update families


def classes(a):
    a = np.asarray(a)
    out = np.zeros(a.shape, np.int8)
    out[np.isposinf(a)] = PINF
    out[np.isneginf(a)] = NINF
    out[np.isnan(a)] = NAN
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def footprint_violation(got, clean, ref, inside=None):
    """None, or a message about the first element (row-major) that breaks the footprint rule.

    got, clean   float32 results of the planted and of the clean call
    ref          the restatement on the planted input (any float type)
    inside       optional mask of elements the caller checks itself although ref is finite there: where the plant
                 changes a value without making it non-finite (sigmoid(+-inf) is exactly 1 / 0, a softmax row with a
                 -inf logit).  Elements with a non-finite ref are always inside."""
    got, clean, ref = np.asarray(got), np.asarray(clean), np.asarray(ref)
    assert got.shape == clean.shape == ref.shape, (got.shape, clean.shape, ref.shape)
    cr, cg = classes(ref), classes(got)
    fin = cr == FINITE
    outside = fin if inside is None else fin & ~np.asarray(inside, bool)
    leak = outside & (_bits(got) != _bits(clean))
    wrong = ~fin & (cg != cr)
    bad = leak | wrong
    if not bad.any():
        return None
    at = tuple(int(i) for i in np.argwhere(bad)[0])
    if leak[at]:
        return (f"{int(leak.sum())} element(s) outside the footprint changed; first at {at}, outside the footprint "
                f"(a leak): got {got[at]!r} (0x{int(_bits(got)[at]):08x}), the clean run gave {clean[at]!r} "
                f"(0x{int(_bits(clean)[at]):08x})")
    return (f"{int(wrong.sum())} element(s) inside the footprint have the wrong class; first at {at}, inside the "
            f"footprint with the wrong class: got {got[at]!r} ({CLASS_NAMES[cg[at]]}), the reference gives "
            f"{CLASS_NAMES[cr[at]]}")


def assert_footprint(got, clean, ref, what, inside=None):
    msg = footprint_violation(got, clean, ref, inside)
    assert msg is None, f"{what}: {msg}"


# ------------------------------------------------------------------------------------------------ restatements
def softmax_ref(Z):
    """_softmax (cukernels.cu:220-242) in float64: the maximum starts at -1e20 and `max < x` never takes a NaN"""
    Z = np.asarray(Z, np.float64)
    rows, cols = Z.shape
    mx = np.full(rows, -1e20)
    for c in range(cols):
        x = Z[:, c]
        up = mx < x
        mx[up] = x[up]
    with np.errstate(all="ignore"):
        Y = np.exp(Z - mx[:, None])
        s = np.zeros(rows)
        for c in range(cols):
            s = s + Y[:, c]
        return Y / s[:, None]


def max_id(A, start):
    """the scan of _check_class (cukernels.cu:405-415): id = start; if (val > max) from max = -1e20"""
    A = np.asarray(A, np.float64)
    rows, cols = A.shape
    idx = np.full(rows, start, np.int64)
    mx = np.full(rows, -1e20)
    for c in range(cols):
        v = A[:, c]
        up = v > mx
        mx[up] = v[up]
        idx[up] = c
    return idx


def check_class_ref(out, des):
    """match[r] of _check_class: out_id starts at -1 and des_id at -2, so a row without a maximum matches nothing"""
    return (max_id(out, -1) == max_id(des, -2)).astype(np.int32)


def _log_clamped(Y):
    """_log_elem (cukernels.cu:131-141): `if (v < FLT_MIN) v = FLT_MIN; log(v)` -- a NaN stays a NaN"""
    Y = np.array(Y, np.float64)
    Y[Y < FLT_MIN] = FLT_MIN
    with np.errstate(all="ignore"):
        return np.log(Y)


def xent_labels_ref(Y, lab):
    """orc_xent_eval (oracle/tnet_oracle.c) in float64: (E = Y - T, xent of each row, correct of each row); a label
    outside [0, N) is an unlabeled row (desired class 0, no cross-entropy)"""
    Y = np.asarray(Y, np.float64)
    rows, cols = Y.shape
    t = np.asarray(lab, np.int64).copy()
    t[(t < 0) | (t >= cols)] = -1
    has = t >= 0
    T = np.zeros_like(Y)
    T[np.flatnonzero(has), t[has]] = 1.0
    correct = (max_id(Y, -1) == np.where(has, t, 0)).astype(np.int64)
    xent = np.zeros(rows)
    xent[has] = -_log_clamped(Y[np.flatnonzero(has), t[has]])
    return Y - T, xent, correct


def xent_dense_ref(Y, D):
    """CuCrossEntropy::Evaluate on dense targets: LogElem, MulElem, sum over ALL columns -- so a NaN (or a +inf,
    whose log is inf) under a zero target gives 0 * NaN = NaN for the row; correct by _check_class"""
    Y, D = np.asarray(Y, np.float64), np.asarray(D, np.float64)
    with np.errstate(all="ignore"):
        prod = D * _log_clamped(Y)
        xent = np.zeros(len(Y))
        for c in range(Y.shape[1]):
            xent = xent - prod[:, c]
    return Y - D, xent, check_class_ref(Y, D).astype(np.int64)


def block_softmax_ref(Z, dims):
    """tests/blocksoftmax_cases.py block_softmax with the reference's comparisons"""
    Z = np.asarray(Z, np.float64)
    Y = np.empty_like(Z)
    lo = 0
    for d in dims:
        Y[:, lo:lo + d] = softmax_ref(Z[:, lo:lo + d])
        lo += d
    return Y


def block_sum_rule_ref(E, dims):
    """BlockSoftmax::BackpropagateFnc (tests/blocksoftmax_cases.py sum_rule): a block whose error sum lies in
    (-0.1, 0.1) passes, one in (0.9, 1.1) is zeroed, anything else -- a NaN or infinite sum fails both comparisons --
    is zeroed and counted as invalid.  Returns (masked error, invalid count)."""
    E = np.asarray(E, np.float64)
    out = np.zeros_like(E)
    invalid, lo = 0, 0
    with np.errstate(all="ignore"):
        for d in dims:
            s = np.zeros(len(E))
            for c in range(lo, lo + d):
                s = s + E[:, c]
            keep = (s > -0.1) & (s < 0.1)
            invalid += int((~keep & ~((s > 0.9) & (s < 1.1))).sum())
            out[keep, lo:lo + d] = E[keep, lo:lo + d]
            lo += d
    return out, invalid


def sigmoid_ref(z):
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def slab_sums_ref(E):
    """[ceil(rows / 32) x cols]: the sum of each 32-row slab, float64"""
    E = np.asarray(E, np.float64)
    slabs = -(-len(E) // SLAB)
    with np.errstate(all="ignore"):
        return np.stack([E[s * SLAB:(s + 1) * SLAB].sum(axis=0) for s in range(slabs)])


def matmul_ref(A, B):
    """float64 product on numpy's own loops (einsum without BLAS): every term enters the sum, in IEEE arithmetic"""
    with np.errstate(all="ignore"):
        return np.einsum("ik,kj->ij", np.asarray(A, np.float64), np.asarray(B, np.float64))


def matmul_fast(A, B):
    """the same product through numpy's matmul (BLAS): what the GPU tests' inner loops use.  tests/test_nonfinite_cpu.py
    holds it to matmul_ref's classes on planted operands, so a BLAS that skipped or reordered a term would show"""
    with np.errstate(all="ignore"):
        return np.matmul(np.asarray(A, np.float64), np.asarray(B, np.float64))


# ------------------------------------------------------------------------------------------------ plant sites
def plant_sites(R, C, k_axis=None):
    """[(name, r, c)] for an operand [R x C].  k_axis: the axis the entry point reduces over (0: rows are k,
    1: columns are k, None: none).  Always: the first element, the last row, the last column.  Along k (length K):
    the last k, k = 63, k = 64, the first index of the K tail for tile depths 16 / 32 / 64, and K - 4 (the 16-byte
    chunk a tail clamp re-reads).  Sites that fall outside the operand or repeat an earlier one are dropped."""
    sites = [("first", 0, 0), ("last row", R - 1, C // 3), ("last column", R // 3, C - 1),
             ("last element", R - 1, C - 1)]
    if k_axis is not None:
        K, other = ((R, C) if k_axis == 0 else (C, R))
        o = (2 * other) // 3
        ks = [("last k", K - 1), ("k = 63", 63), ("k = 64", 64), ("K - 4", K - 4)]
        ks += [(f"first k of the tail at depth {d}", (K // d) * d) for d in TILE_DEPTHS if K % d]
        for name, k in ks:
            if 0 <= k < K:
                sites.append((name, k, o) if k_axis == 0 else (name, o, k))
    seen, out = set(), []
    for name, r, c in sites:
        if 0 <= r < R and 0 <= c < C and (r, c) not in seen:
            seen.add((r, c))
            out.append((name, r, c))
    return out


def check_conditions(multiplied=(), sigmoids=(), others=()):
    """the input conditions of the module docstring; every operand is a finite array"""
    for a in multiplied:
        assert not (np.asarray(a) == 0).any(), "an exact zero in an operand that multiplies a planted value"
    for a in sigmoids:
        a = np.asarray(a)
        assert (a >= 0.05).all() and (a <= 0.95).all(), "a sigmoid output outside [0.05, 0.95]"
    for a in tuple(multiplied) + tuple(sigmoids) + tuple(others):
        a = np.asarray(a)
        if a.dtype.kind == "f":
            assert np.isfinite(a).all() and (np.abs(a) <= MAX_FINITE).all(), "an operand is not finite and <= 1e4"


def planted(a, r, c, v):
    b = np.array(a, np.float32).reshape(np.asarray(a).shape if np.asarray(a).ndim == 2 else (1, -1))
    b[r, c] = v
    return b.reshape(np.asarray(a).shape)


# ------------------------------------------------------------------------------------------------ footprints
def rows_of(shape, rows):
    m = np.zeros(shape, bool)
    m[np.atleast_1d(rows)] = True
    return m


def cols_of(shape, cols):
    m = np.zeros(shape, bool)
    m[..., np.atleast_1d(cols)] = True
    return m


def elems_of(shape, *at):
    m = np.zeros(shape, bool)
    for a in at:
        m[a] = True
    return m


def nothing(shape):
    return np.zeros(shape, bool)


def nonfinite(a):
    return ~np.isfinite(np.asarray(a, np.float64))


# ------------------------------------------------------------------------------------------------ the GEMM family
class Family:
    """one entry point in one variant.
    ins    names of the operands it reads (keys of the data dict); an in-place operand is also in outs
    outs   names of what it writes
    ref    ref(d, mm) -> {out name: float64 array}: the stated formula on the data dict d, products through mm
    ops    {operand: (k_axis, predict)}: where plant_sites puts plants, and predict(shapes, r, c) -> {out name: mask}
           the predicted footprint of a plant at [r, c] (outputs it does not name are untouched)"""

    def __init__(self, name, ins, outs, ref, ops, **params):
        self.name, self.ins, self.outs, self.ref, self.ops, self.params = name, ins, outs, ref, ops, params


def affine_data(rows, n_in, n_out, seed=0):
    """operands of the affine family at (rows, n_in, n_out), conditioned as check_conditions asks"""
    g = np.random.default_rng(1000 + seed)

    def rnd(shape, scale=1.0):
        return (g.standard_normal(shape) * scale).astype(np.float32)

    d = dict(X=rnd((rows, n_in)), W=rnd((n_in, n_out), 0.1), b=rnd((1, n_out)), b_in=rnd((1, n_in)),
             E=rnd((rows, n_out)), Es=rnd((rows, n_out), 0.01), corr=rnd((n_in, n_out), 0.01),
             corr_b=rnd((1, n_out), 0.01), A=rnd((rows, n_in)))
    d["Yb"] = np.clip(sigmoid_ref(rnd((rows, n_in))), 0.05, 0.95).astype(np.float32)
    d["P"] = slab_sums_ref(d["Es"]).astype(np.float32)
    check_conditions(multiplied=[d[k] for k in ("X", "W", "E", "Es", "A")], sigmoids=[d["Yb"]],
                     others=[d[k] for k in ("b", "b_in", "corr", "corr_b", "P")])
    for a in d.values():
        a.setflags(write=False)
    return d


def sgemm_data(M, N, K, ta, tb, seed=0):
    g = np.random.default_rng(2000 + seed)
    d = dict(A=g.standard_normal((K, M) if ta == "T" else (M, K)).astype(np.float32),
             B=g.standard_normal((N, K) if tb == "T" else (K, N)).astype(np.float32),
             C=g.standard_normal((M, N)).astype(np.float32))
    check_conditions(multiplied=[d["A"], d["B"]], others=[d["C"]])
    for a in d.values():
        a.setflags(write=False)
    return d


def _f64(a):
    return np.asarray(a, np.float64)


def _act(z, act):
    if act in (1, 3):
        z = sigmoid_ref(z)
    return -z if act in (2, 3) else z


def _slab(r):
    return r // SLAB


def sgemm_family(ta, tb, beta, alpha=0.75):
    def ref(d, mm):
        A, B = _f64(d["A"]), _f64(d["B"])
        with np.errstate(all="ignore"):
            c = alpha * mm(A.T if ta == "T" else A, B.T if tb == "T" else B)
            return {"C": c + beta * _f64(d["C"]) if beta else c}  # beta == 0 reads no C

    ops = {"A": (0 if ta == "T" else 1, lambda s, r, c: {"C": rows_of(s["C"], c if ta == "T" else r)}),
           "B": (1 if tb == "T" else 0, lambda s, r, c: {"C": cols_of(s["C"], r if tb == "T" else c)})}
    ins = ("A", "B")
    if beta:
        ops["C"] = (None, lambda s, r, c: {"C": elems_of(s["C"], (r, c))})
        ins += ("C",)
    return Family(f"sgemm {ta}{tb} beta {beta}", ins, ("C",), ref, ops, ta=ta, tb=tb, alpha=alpha, beta=beta)


def gemm_families():
    """the GEMM family's entry points over affine_data(); tests/test_gpu_nonfinite.py has the call of each name"""
    fams = []
    def E():
        return np.errstate(all="ignore")

    for act in (0, 1, 2, 3):
        fams.append(Family(
            f"affine_fwd act {act}", ("X", "W", "b"), ("Y",),
            lambda d, mm, act=act: {"Y": _act(mm(d["X"], d["W"]) + _f64(d["b"]), act)},
            {"X": (1, lambda s, r, c: {"Y": rows_of(s["Y"], r)}),
             "W": (0, lambda s, r, c: {"Y": cols_of(s["Y"], c)}),
             "b": (None, lambda s, r, c: {"Y": cols_of(s["Y"], c)})}, act=act))
    for act in (0, 1):
        fams.append(Family(
            f"affine_fwd_t act {act}", ("E", "W", "b_in"), ("Yt",),
            lambda d, mm, act=act: {"Yt": _act(mm(d["E"], _f64(d["W"]).T) + _f64(d["b_in"]), act)},
            {"E": (1, lambda s, r, c: {"Yt": rows_of(s["Yt"], r)}),
             "W": (1, lambda s, r, c: {"Yt": cols_of(s["Yt"], r)}),
             "b_in": (None, lambda s, r, c: {"Yt": cols_of(s["Yt"], c)})}, act=act))

    def bwd(d, mm, dsig, slabs):
        with E():
            z = mm(d["E"], _f64(d["W"]).T)
            if dsig:
                z = z * (_f64(d["Yb"]) * (1.0 - _f64(d["Yb"])))
        return {"Eo": z, "Po": slab_sums_ref(z)} if slabs else {"Eo": z}

    for name, dsig, slabs in (("affine_bwd dsig 0", 0, False), ("affine_bwd dsig 1", 1, False),
                              ("affine_bwd_colsum", 1, True), ("affine_bwd_colsum_t", 1, True)):
        def p_e(s, r, c, slabs=slabs):
            out = {"Eo": rows_of(s["Eo"], r)}
            if slabs:
                out["Po"] = rows_of(s["Po"], _slab(r))
            return out

        def p_w(s, r, c, slabs=slabs):
            out = {"Eo": cols_of(s["Eo"], r)}
            if slabs:
                out["Po"] = cols_of(s["Po"], r)
            return out

        def p_y(s, r, c, slabs=slabs, dsig=dsig):
            if not dsig:
                return {}  # Ybelow is not part of the formula
            out = {"Eo": elems_of(s["Eo"], (r, c))}
            if slabs:
                out["Po"] = elems_of(s["Po"], (_slab(r), c))
            return out

        fams.append(Family(name, ("E", "W", "Yb"), ("Eo", "Po") if slabs else ("Eo",),
                           lambda d, mm, dsig=dsig, slabs=slabs: bwd(d, mm, dsig, slabs),
                           {"E": (1, p_e), "W": (1, p_w), "Yb": (None, p_y)}, dsig=dsig))

    fams.append(Family("colsum_slab_sums", ("E",), ("Pe",), lambda d, mm: {"Pe": slab_sums_ref(d["E"])},
                       {"E": (None, lambda s, r, c: {"Pe": elems_of(s["Pe"], (_slab(r), c))})}))

    def update(d, mm, mmt, bias, scale):
        with E():
            c = mm(_f64(d["X"]).T, d["Es"])
            if mmt:
                c = c + mmt * _f64(d["corr"])
            w = _f64(d["W"]) + scale * c
            out = {"W": w + UPDATE_L2 * w}  # the decay pass is always made (cuBiasedLinearity.cc:62-63): inf -> NaN
            if mmt:
                out["corr"] = c
            if bias:
                gb = _f64(_f64(d["P"]).sum(axis=0, keepdims=True).astype(np.float32))
                cb = gb + mmt * _f64(d["corr_b"]) if mmt else gb
                out["b"] = _f64(d["b"]) + scale * cb
                if mmt:
                    out["corr_b"] = cb
        return out

    for bias in (False, True):
        for mmt in (0.0, 0.5):
            def both(mask_of, mmt=mmt):
                return lambda s, r, c: {k: mask_of(s[k], r, c) for k in (("W", "corr") if mmt else ("W",))}

            def bboth(mmt=mmt):
                return lambda s, r, c: {k: cols_of(s[k], c) for k in (("b", "corr_b") if mmt else ("b",))}

            ops = {"X": (0, both(lambda sh, r, c: rows_of(sh, c))),
                   "Es": (0, both(lambda sh, r, c: cols_of(sh, c))),
                   "W": (None, lambda s, r, c: {"W": elems_of(s["W"], (r, c))})}
            ins, outs = ("X", "Es", "W"), ("W",)
            if mmt:
                ops["corr"] = (None, both(lambda sh, r, c: elems_of(sh, (r, c))))
                ins, outs = ins + ("corr",), outs + ("corr",)
            if bias:
                ops["P"] = (None, bboth())
                ops["b"] = (None, lambda s, r, c: {"b": cols_of(s["b"], c)})
                ins, outs = ins + ("P", "b"), outs + ("b",)
                if mmt:
                    ops["corr_b"] = (None, bboth())
                    ins, outs = ins + ("corr_b",), outs + ("corr_b",)
            fams.append(Family(f"affine_update{'_bias' if bias else ''} mmt {mmt}", ins, outs,
                               lambda d, mm, mmt=mmt, bias=bias: update(d, mm, mmt, bias, d["scale"]), ops,
                               mmt=mmt, bias=bias))

    fams.append(Family("affine_grad", ("X", "Es"), ("G",), lambda d, mm: {"G": mm(_f64(d["X"]).T, d["Es"])},
                       {"X": (0, lambda s, r, c: {"G": rows_of(s["G"], c)}),
                        "Es": (0, lambda s, r, c: {"G": cols_of(s["G"], c)})}))
    fams.append(Family("affine_grad_bias", ("X", "Es", "P"), ("G", "gb"),
                       lambda d, mm: {"G": mm(_f64(d["X"]).T, d["Es"]),
                                      "gb": _f64(_f64(d["P"]).sum(axis=0, keepdims=True).astype(np.float32))},
                       {"X": (0, lambda s, r, c: {"G": rows_of(s["G"], c)}),
                        "Es": (0, lambda s, r, c: {"G": cols_of(s["G"], c)}),
                        "P": (None, lambda s, r, c: {"gb": cols_of(s["gb"], c)})}))

    def rbm(d, mm, mmt=0.5, l2=-2e-4):
        with E():
            c = mmt * _f64(d["corr"]) + d["rbm_scale"] * mm(_f64(d["X"]).T, d["E"]) + l2 * _f64(d["W"])
            return {"W": _f64(d["W"]) + c, "corr": c}

    wc = ("W", "corr")
    fams.append(Family("rbm_update", ("X", "E", "W", "corr"), wc, rbm,
                       {"X": (0, lambda s, r, c: {k: rows_of(s[k], c) for k in wc}),
                        "E": (0, lambda s, r, c: {k: cols_of(s[k], c) for k in wc}),
                        "W": (None, lambda s, r, c: {k: elems_of(s[k], (r, c)) for k in wc}),
                        "corr": (None, lambda s, r, c: {k: elems_of(s[k], (r, c)) for k in wc})}, mmt=0.5, l2=-2e-4))
    fams.append(Family("transpose", ("A",), ("At",), lambda d, mm: {"At": _f64(d["A"]).T.copy()},
                       {"A": (None, lambda s, r, c: {"At": elems_of(s["At"], (c, r))})}))
    return fams


def with_scales(d, rows):
    """the data dict plus the scalar parameters the update formulas use"""
    d = dict(d)
    d["scale"], d["rbm_scale"] = -0.3 / rows, 0.1 / rows
    return d


def affected(ref, ref_clean):
    """where the plant reaches the restatement's output: non-finite, or another finite value than on the clean input
    (sigmoid(+-inf) is exactly 1 / 0)"""
    ref, ref_clean = np.asarray(ref, np.float64), np.asarray(ref_clean, np.float64)
    return nonfinite(ref) | (ref != ref_clean)
