"""tests/nonfinite_cases.py without a GPU: the restatements against the oracle's C code on planted inputs, the
predicted footprints against float64 numpy for every entry point, plant site and value, and assert_footprint itself
(a leak outside the footprint, a wrong class inside it and one flipped low bit are each caught and located)."""
import numpy as np
import pytest

import nonfinite_cases as nf
import oracle as orc
from nonfinite_cases import VALUES, FLT_MIN

INF, NINF, NAN = VALUES
SHAPES = [(33, 65, 31), (70, 135, 100)]


def test_classes():
    a = np.array([[0.0, np.inf, -np.inf, np.nan, -0.0, 3e38]], np.float32)
    assert nf.classes(a).tolist() == [[0, 1, 2, 3, 0, 0]]
    assert nf.classes(a.astype(np.float64)).tolist() == [[0, 1, 2, 3, 0, 0]]


def test_plant_sites():
    """K = 100 (K % 4 == 0, no multiple of 16 / 32 / 64): the last k, 63, 64 (also the tail's first k at depth 64),
    96 (K - 4, and the tail's first k at depths 16 and 32); K = 31 has no k = 63 / 64 and its tails start at 16 and 0"""
    s = dict((n, (r, c)) for n, r, c in nf.plant_sites(70, 100, 1))
    ks = sorted(c for _, c in s.values())
    assert s["first"] == (0, 0) and s["last element"] == (69, 99)
    assert {99, 63, 64, 96} <= set(ks)
    assert all(0 <= r < 70 and 0 <= c < 100 for r, c in s.values())
    assert len(set(s.values())) == len(s)
    rows31 = [r for _, r, c in nf.plant_sites(31, 65, 0)]
    assert {0, 30, 27, 16} <= set(rows31) and max(rows31) == 30
    assert len(nf.plant_sites(5, 7)) == 4


def rows6(cols, seed=5):
    return np.random.default_rng(seed).standard_normal((6, cols)).astype(np.float32) * 2


@pytest.mark.parametrize("cols", [7, 135, 132])
def test_softmax_restatement_matches_the_oracle(cols):
    """orc.softmax is the C restatement of _softmax; on clean and on planted rows the float64 loop has its classes
    everywhere and its values where finite"""
    Z = rows6(cols)
    Z[1, 3] = NAN
    Z[2, cols - 1] = INF
    Z[3, 0] = NINF
    Z[4, :] = NINF
    got, ref = nf.softmax_ref(Z), orc.softmax(Z)
    np.testing.assert_array_equal(nf.classes(got), nf.classes(ref))
    fin = np.isfinite(ref)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=2e-6, atol=1e-30)
    # the footprints: a NaN or a +inf takes its whole row (inf - inf), a -inf logit is an exact zero, a row of
    # -inf is 0 / 0
    assert np.isnan(got[[1, 2, 4]]).all() and np.isfinite(got[[0, 3, 5]]).all()
    assert got[3, 0] == 0.0 and abs(got[3].sum() - 1) < 1e-12


@pytest.mark.parametrize("cols", [7, 135])
def test_xent_restatements_match_the_oracle(cols):
    Z = rows6(cols)
    lab = np.array([2, 3, -1, 0, 5, cols - 1], np.int32)
    Z[1, 3] = NAN          # the label's row is NaN
    Z[3, 0] = NINF         # -inf in the label column: -log(FLT_MIN)
    Z[4, 1] = NINF         # -inf elsewhere
    Y = orc.softmax(Z)
    E, xent, correct = nf.xent_labels_ref(Y, lab)
    Eo, xo, co = orc.xent_eval(Y, lab)
    np.testing.assert_array_equal(nf.classes(E), nf.classes(Eo))
    fin = np.isfinite(Eo)
    np.testing.assert_allclose(E[fin], Eo[fin], rtol=1e-6, atol=1e-9)
    assert np.isnan(xo) and np.isnan(xent.sum()) and np.isnan(xent[1]) and np.isfinite(np.delete(xent, 1)).all()
    assert xent[3] == -np.log(FLT_MIN) and xent[2] == 0
    assert int(correct.sum()) == co and correct[1] == 0
    # without the NaN row the totals agree
    keep = [0, 2, 3, 4, 5]
    _, x2, c2 = orc.xent_eval(Y[keep], lab[keep])
    np.testing.assert_allclose(xent[keep].sum(), x2, rtol=1e-6)
    assert int(correct[keep].sum()) == c2
    # dense targets that are the one-hot rows: the same numbers, except that a NaN anywhere in a row -- labelled
    # or not -- makes the row's cross-entropy NaN (NaN * 0)
    D = np.zeros_like(Y)
    has = lab >= 0
    D[np.flatnonzero(has), lab[has]] = 1
    Ed, xd, cd = nf.xent_dense_ref(Y, D)
    np.testing.assert_array_equal(nf.classes(Ed), nf.classes(E))
    np.testing.assert_allclose(xd[keep], xent[keep], rtol=1e-12)
    assert np.isnan(xd[1])
    Yn = Y.copy()
    Yn[2, 4] = NAN         # row 2 is unlabeled: all-zero targets
    assert np.isnan(nf.xent_dense_ref(Yn, D)[1][2]) and nf.xent_labels_ref(Yn, lab)[1][2] == 0
    Yn[2, 4] = INF         # 0 * log(inf)
    assert np.isnan(nf.xent_dense_ref(Yn, D)[1][2])
    Yn[2, 4] = NINF        # clamped to FLT_MIN: finite, times 0
    assert nf.xent_dense_ref(Yn, D)[1][2] == 0


def test_check_class_restatement():
    """np.argmax would pick a NaN; the reference's scan never does, and a row without a maximum matches nothing"""
    out = np.array([[1, NAN, 3, 2], [NAN, NAN, NAN, NAN], [NAN, NAN, NAN, NAN], [INF, 1, 2, 3], [-1e30, NINF, 0, 0]],
                   np.float32)
    des = np.array([[0, 0, 1, 0], [NAN, NAN, NAN, NAN], [1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]], np.float32)
    assert nf.max_id(out, -1).tolist() == [2, -1, -1, 0, 2]
    assert nf.check_class_ref(out, des).tolist() == [1, 0, 0, 1, 1]
    assert np.argmax(out[0]) == 1  # the shortcut this module does not use


def test_block_restatements():
    """a plant in block b of a row stays in block b of Y; the sum rule counts a NaN block sum as invalid"""
    import blocksoftmax_cases as bc
    dims = (3, 5, 2)
    Z = rows6(10)
    np.testing.assert_allclose(nf.block_softmax_ref(Z, dims), bc.block_softmax(Z, dims), rtol=1e-12)
    E = nf.block_softmax_ref(Z, dims)
    E[np.arange(6), [0, 4, 9, 1, 5, 8]] -= 1
    m, inv = nf.block_sum_rule_ref(E, dims)
    m2, inv2 = bc.sum_rule(E, dims)
    np.testing.assert_array_equal(m, m2)
    assert inv == inv2 == 0
    for v in VALUES:
        Zp = Z.copy()
        Zp[2, 4] = v
        Y = nf.block_softmax_ref(Zp, dims)
        aff = nf.affected(Y, nf.block_softmax_ref(Z, dims))
        np.testing.assert_array_equal(aff, nf.elems_of(Y.shape, (2, slice(3, 8))))
    En = E.copy()
    En[2, 3:8] = NAN
    m, inv = nf.block_sum_rule_ref(En, dims)
    assert inv == 1 and (m[2, 3:8] == 0).all() and np.isfinite(m).all()


# ---------------------------------------------------------------------------------------------- footprints
def sgemm_fams():
    return [nf.sgemm_family(ta, tb, beta) for ta in "NT" for tb in "NT" for beta in (0.0, 0.5)]


def check_family(fam, d):
    """every plant site and value of every operand: the restatement's affected set is the predicted footprint, its
    non-finite part has the classes the BLAS product gives too, and everything else is bit-identical to the clean
    restatement"""
    clean = fam.ref(d, nf.matmul_ref)
    shapes = {k: v.shape for k, v in clean.items()}
    assert set(clean) == set(fam.outs)
    for v in clean.values():
        assert np.isfinite(v).all()
    n = 0
    for op, (k_axis, predict) in fam.ops.items():
        a = d[op]
        for site, r, c in nf.plant_sites(a.shape[0], a.shape[1], k_axis):
            for val in VALUES:
                dp = dict(d)
                dp[op] = nf.planted(a, r, c, val)
                ref, fast = fam.ref(dp, nf.matmul_ref), fam.ref(dp, nf.matmul_fast)
                want = predict(shapes, r, c)
                for o in fam.outs:
                    what = f"{fam.name}: {val} in {op}[{r}, {c}] ({site}): {o}"
                    aff = nf.affected(ref[o], clean[o])
                    np.testing.assert_array_equal(aff, want.get(o, nf.nothing(shapes[o])), err_msg=what)
                    np.testing.assert_array_equal(nf.classes(fast[o]), nf.classes(ref[o]), err_msg=what)
                    if np.isnan(val):  # a NaN makes its whole footprint NaN; an infinity may saturate (sigmoid)
                        assert np.isnan(ref[o][aff]).all(), what
                n += 1
    return n


@pytest.mark.parametrize("rows,n_in,n_out", SHAPES)
def test_gemm_family_footprints(rows, n_in, n_out):
    d = nf.with_scales(nf.affine_data(rows, n_in, n_out), rows)
    fams = nf.gemm_families()
    assert len({f.name for f in fams}) == len(fams)
    assert sum(check_family(f, d) for f in fams) > 1000


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_sgemm_footprints(M, N, K):
    for fam in sgemm_fams():
        check_family(fam, nf.sgemm_data(M, N, K, fam.params["ta"], fam.params["tb"]))


def test_sigmoid_saturates_exactly():
    """what lets the forward's sigmoid rows be checked for equality: sigmoid(+inf) == 1, sigmoid(-inf) == 0"""
    assert nf.sigmoid_ref(np.array([np.inf, -np.inf])).tolist() == [1.0, 0.0]
    assert np.isnan(nf.sigmoid_ref(np.array([np.nan]))).all()


def test_check_conditions():
    a = np.ones((2, 3), np.float32)
    nf.check_conditions(multiplied=[a], sigmoids=[a * 0.5], others=[a * 9e3])
    z = a.copy()
    z[1, 1] = 0
    with pytest.raises(AssertionError, match="exact zero"):
        nf.check_conditions(multiplied=[z])
    with pytest.raises(AssertionError, match="sigmoid"):
        nf.check_conditions(sigmoids=[a * 0.99])
    with pytest.raises(AssertionError, match="1e4"):
        nf.check_conditions(others=[a * 2e4])
    z[1, 1] = NAN
    with pytest.raises(AssertionError, match="finite"):
        nf.check_conditions(others=[z])


# ---------------------------------------------------------------------------------------------- assert_footprint
def footprint_case():
    clean = np.random.default_rng(3).standard_normal((5, 8)).astype(np.float32)
    ref = clean.astype(np.float64)
    ref[2, :] = [np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf, np.nan, np.inf]
    got = clean.copy()
    got[2, :] = ref[2, :]
    return got, clean, ref


def test_assert_footprint_accepts_the_footprint():
    got, clean, ref = footprint_case()
    nf.assert_footprint(got, clean, ref, "ok")
    got[2, 2] = np.float32(np.nan).view(np.uint32).__or__(np.uint32(5)).view(np.float32)  # another NaN payload: same class
    nf.assert_footprint(got, clean, ref, "ok")
    # -0.0 == 0.0 but is another bit pattern: outside the footprint it counts
    clean[0, 0] = got[0, 0] = 0.0
    ref[0, 0] = 0.0
    nf.assert_footprint(got, clean, ref, "ok")
    got[0, 0] = -0.0
    with pytest.raises(AssertionError, match=r"first at \(0, 0\), outside the footprint \(a leak\)"):
        nf.assert_footprint(got, clean, ref, "signed zero")


@pytest.mark.parametrize("at", [(0, 0), (1, 7), (3, 2), (4, 7)])
@pytest.mark.parametrize("val", VALUES)
def test_assert_footprint_catches_a_leak(at, val):
    got, clean, ref = footprint_case()
    got[at] = val
    with pytest.raises(AssertionError) as e:
        nf.assert_footprint(got, clean, ref, "leak")
    assert f"first at {at}, outside the footprint (a leak)" in str(e.value) and "1 element(s)" in str(e.value)


@pytest.mark.parametrize("col,val,name", [(0, -np.inf, r"\+inf"), (2, np.inf, "nan"), (1, 1.5, "-inf"), (4, 0.0, "nan")])
def test_assert_footprint_catches_a_wrong_class(col, val, name):
    got, clean, ref = footprint_case()
    got[2, col] = val
    with pytest.raises(AssertionError, match=rf"first at \(2, {col}\), inside the footprint with the wrong class.*"
                                             rf"the reference gives {name}"):
        nf.assert_footprint(got, clean, ref, "class")


@pytest.mark.parametrize("at", [(0, 3), (4, 0)])
def test_assert_footprint_catches_a_flipped_low_bit(at):
    got, clean, ref = footprint_case()
    w = got.view(np.uint32)
    w[at] ^= 1
    assert abs(float(got[at]) - float(clean[at])) <= 1.2e-7 * abs(float(clean[at]))  # no tolerance would notice
    with pytest.raises(AssertionError, match=r"outside the footprint \(a leak\)") as e:
        nf.assert_footprint(got, clean, ref, "bit")
    assert f"first at {at}" in str(e.value)


def test_assert_footprint_names_the_first_offender_and_honours_inside():
    got, clean, ref = footprint_case()
    got[3, 1] = np.nan
    got[2, 0] = np.nan      # wrong class, earlier in row-major order
    with pytest.raises(AssertionError, match=r"first at \(2, 0\), inside"):
        nf.assert_footprint(got, clean, ref, "order")
    got, clean, ref = footprint_case()
    ref[1, :] = 1.0         # finite but changed by the plant: the caller's to check
    got[1, :] = 1.0
    with pytest.raises(AssertionError, match=r"first at \(1, 0\)"):
        nf.assert_footprint(got, clean, ref, "saturated")
    nf.assert_footprint(got, clean, ref, "saturated", inside=nf.rows_of(ref.shape, 1))
    got[2, 1] = np.inf      # `inside` does not excuse a wrong class
    with pytest.raises(AssertionError, match="wrong class"):
        nf.assert_footprint(got, clean, ref, "saturated", inside=nf.rows_of(ref.shape, 1))
