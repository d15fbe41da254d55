"""The normalisation pass on the GPU: tnet_col_moments / tnet_col_moments_fetch (csrc/kernels/col_moments.hip) and
tnet_amd.Normalizer, the TNormCu loop (csrc/host/cunorm.cpp), against the float64 restatement tests/tnorm_cases.py and
the reference fixture tests/golden/tnorm_ex01.npz (tests/golden/make_tnorm.py: reference CPU TFeaCat output of the
first four components of examples/01's Hamm_dct_norm, through the restatement).

Kernel tests are exact: integer inputs |x| <= 1024 make every double sum exact whatever its order, so first / second
must equal numpy's bit for bit.  The loop tests' bounds are derived where they are used:
  against the reference fixture   |d first_j| <= T_REL * abs_sum_j,  |d second_j| <= 2 T_REL * second_j
      T_REL = 1e-5 is the per-element relative tolerance tests/test_gpu_frontend.py grants <blocklinearity> against a
      float64 product (test_blocklinearity, rtol 1e-5) and this transform's sums against reference TFeaCat output
      (test_transform_vs_reference_tfeacat: 1e-5 * sum |y| and 1e-5 * sum y^2); a relative error t per element moves
      y by t |y| and y^2 by 2 t y^2.  The summation-order term 2 N 2^-53 is added (negligible beside it).
  against the library's own output   only the order of the double sums differs: 2 N 2^-53 * sum |y| (resp. sum y^2)
  the written text applied to the corpus   see test_text_normalises_the_corpus.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tnorm_cases as tc  # noqa: E402
import tnet_amd  # noqa: E402
from kernel_views import POISON_INPUT, PoisonView, assert_frame_untouched, assert_unchanged  # noqa: E402
from tnet_amd import DeviceArray, formats  # noqa: E402
from tnet_amd._lib import MatrixDim, check, header_constant, lib  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(REPO, "tests", "golden", "ex01")
R = header_constant("TNET_COL_MOMENTS_ROWS")    # the kernel's slab height
SLOTS = header_constant("TNET_COL_MOMENTS_SLOTS")
T_REL = 1e-5
U64 = 2.0 ** -53


def S():
    return lib().tnet_stream()


# ------------------------------------------------------------------------------------------- kernel

class Acc:
    """a zeroed device accumulator for `cols` columns"""

    def __init__(self, cols):
        self.cols = cols
        self.words = int(lib().tnet_col_moments_words(cols))
        assert self.words == SLOTS * 2 * cols + 1
        self.buf = DeviceArray(1, self.words, np.float64, stride=self.words)   # zeroed
        self.ptr = self.buf.ptr

    def add(self, x_ptr, dim, tag):
        check(lib().tnet_col_moments(x_ptr, dim, self.ptr, tag, S()), "tnet_col_moments")

    def add_array(self, x, tag=0):
        d = DeviceArray.from_numpy(np.ascontiguousarray(x, np.float32)) if x.shape[0] else None
        self.add(d.ptr if d is not None else None, MatrixDim(x.shape[0], x.shape[1], d.stride if d else x.shape[1]),
                 tag)
        return d  # keep alive

    def fetch(self, ptr=None):
        first, second = np.empty(self.cols, np.float64), np.empty(self.cols, np.float64)
        bad = C.c_int(-2)
        check(lib().tnet_col_moments_fetch(ptr or self.ptr, self.cols, first.ctypes.data, second.ctypes.data,
                                           C.byref(bad), S()), "tnet_col_moments_fetch")
        return first, second, bad.value


def _ints(rng, rows, cols):
    return rng.integers(-tc.EXACT_MAX, tc.EXACT_MAX + 1, (rows, cols)).astype(np.float32)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def _expect(mats, cols):
    first, second = np.zeros(cols), np.zeros(cols)
    for x in mats:
        f, s, _ = tc.moments(x)
        first += f
        second += s
    return first, second


@pytest.mark.parametrize("cols", tc.EXACT_COLS)
def test_exact_sums(cols):
    """every row count of the table (1 .. 65, R - 1, R, R + 1, SLOTS * R + 1: one slab more than the slots, so slot 0
    takes two slabs) at this width; three matrices of different heights, one of them empty, into one accumulator"""
    rng = np.random.default_rng(cols)
    rows_list = tc.exact_rows(R, SLOTS)
    for k, rows in enumerate(rows_list):
        mats = [_ints(rng, rows, cols), _ints(rng, 0, cols), _ints(rng, rows_list[(k + 3) % len(rows_list)], cols)]
        acc = Acc(cols)
        keep = [acc.add_array(x, tag=i) for i, x in enumerate(mats)]
        first, second, bad = acc.fetch()
        ef, es = _expect(mats, cols)
        assert bad == -1
        assert _bits_equal(first, ef) and _bits_equal(second, es), (rows, cols)
        del keep


@pytest.mark.parametrize("cols", [64, 65])
def test_square_is_fp32(cols):
    """x = 1 + 2^-12: the fp32 square is 1 + 2^-11 exactly (the tie rounds to even); a double square or an fp64 FMA
    keeps the 2^-24.  64 columns take the 16-byte loads, 65 the scalar ones."""
    rows = 2 * R + 3
    x = np.full((rows, cols), 1 + 2.0 ** -12, np.float32)
    acc = Acc(cols)
    keep = acc.add_array(x)
    first, second, bad = acc.fetch()
    assert bad == -1
    assert _bits_equal(first, np.full(cols, rows * (1 + 2.0 ** -12)))
    assert _bits_equal(second, np.full(cols, rows * (1 + 2.0 ** -11)))
    assert not _bits_equal(second, np.full(cols, rows * (1 + 2.0 ** -11 + 2.0 ** -24)))
    del keep


@pytest.mark.parametrize("acc_layout", ["tight", "offset"])
@pytest.mark.parametrize("layout", ["tight", "offset", "shifted", "odd"])
def test_views(layout, acc_layout):
    """X as a poisoned view (16-byte aligned or not, a stride that is a multiple of 4 or not): the input stays
    bit-identical, a stray read of poison would turn a sum NaN, and the accumulator -- an 8-byte view -- keeps its
    frame"""
    rng = np.random.default_rng(7)
    for rows, cols in tc.VIEW_SHAPES:
        x = _ints(rng, rows, cols)
        X = PoisonView(x, layout, poison=POISON_INPUT)
        words = int(lib().tnet_col_moments_words(cols))
        A = PoisonView(np.zeros((1, words)), acc_layout, dtype=np.float64)
        for tag in range(2):
            check(lib().tnet_col_moments(X.ptr, X.dim, A.ptr, tag, S()), "tnet_col_moments")
        acc = Acc(cols)
        first, second, bad = acc.fetch(A.ptr)
        assert_unchanged(X, X.initial, f"X {layout} {rows}x{cols}")
        assert_frame_untouched(A, f"accumulator {acc_layout} {rows}x{cols}")
        ef, es = _expect([x, x], cols)
        assert bad == -1
        assert _bits_equal(first, ef) and _bits_equal(second, es), (layout, rows, cols)


def test_deterministic_bits():
    """two fresh accumulators, the same five calls on random float data: bit-identical fetches"""
    rng = np.random.default_rng(11)
    mats = [(rng.standard_normal((rows, 598)) * 50).astype(np.float32) for rows in (136, 1, 3 * R, SLOTS * R + 5, 77)]
    devs = [DeviceArray.from_numpy(x) for x in mats]
    out = []
    for _ in range(2):
        acc = Acc(598)
        for k, d in enumerate(devs):
            acc.add(d.ptr, d.dim, k)
        out.append(acc.fetch())
    assert out[0][2] == out[1][2] == -1
    assert _bits_equal(out[0][0], out[1][0]) and _bits_equal(out[0][1], out[1][1])
    ef, es = _expect(mats, 598)   # and they are the sums, to summation order
    _, _, ab = zip(*[tc.moments(x) for x in mats])
    n = sum(x.shape[0] for x in mats)
    assert (np.abs(out[0][0] - ef) <= 2 * n * U64 * sum(ab)).all()
    assert (np.abs(out[0][1] - es) <= 2 * n * U64 * es).all()


def test_nonfinite_tags():
    """tags 7, 3, 9: a NaN under 7, 1e20f (finite; its fp32 square is infinite) under 3, clean under 9 -> 3; all clean
    -> -1.  Infinite inputs are data, not faults."""
    rng = np.random.default_rng(5)
    clean = [_ints(rng, rows, 65) for rows in (40, 2 * R, 9)]
    acc = Acc(65)
    keep = [acc.add_array(x, tag) for x, tag in zip(clean, (7, 3, 9))]
    first, second, bad = acc.fetch()
    assert bad == -1 and np.isfinite(first).all() and np.isfinite(second).all()
    dirty = [x.copy() for x in clean]
    dirty[0][17, 5] = np.nan
    dirty[1][R + 1, 64] = np.float32(1e20)
    acc = Acc(65)
    keep = [acc.add_array(x, tag) for x, tag in zip(dirty, (7, 3, 9))]
    first, second, bad = acc.fetch()
    assert bad == 3
    assert np.isnan(first[5]) and np.isnan(second[5]) and np.isinf(second[64]) and np.isfinite(first[64])
    acc = Acc(65)   # the same with the larger tag seen first, and an infinite input
    dirty[2][0, 0] = np.inf
    keep = [acc.add_array(x, tag) for x, tag in zip(reversed(dirty), (9, 3, 7))]
    assert acc.fetch()[2] == 3
    del keep


def test_argument_checks():
    acc = Acc(8)
    x = DeviceArray.from_numpy(np.ones((4, 8), np.float32))
    assert lib().tnet_col_moments(x.ptr, MatrixDim(4, 8, 7), acc.ptr, 0, S()) == -1      # stride < cols
    assert lib().tnet_col_moments(x.ptr, MatrixDim(4, 0, 8), acc.ptr, 0, S()) == -1
    assert lib().tnet_col_moments(x.ptr, MatrixDim(4, 8, 64), acc.ptr, -1, S()) == -1    # a tag is >= 0
    assert lib().tnet_col_moments(x.ptr, MatrixDim(4, 8, 64), acc.ptr + 4, 0, S()) == -1  # 8-byte alignment
    assert lib().tnet_col_moments(None, MatrixDim(0, 8, 8), acc.ptr, 0, S()) == 0        # rows == 0: no-op
    assert lib().tnet_col_moments_words(8192) == SLOTS * 2 * 8192 + 1


# --------------------------------------------------------------------------------------------- loop

@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "tnorm_ex01.npz"))


@pytest.fixture(scope="module")
def head_layers():
    return formats.read_nnet(os.path.join(EX, "Hamm_dct_norm"))[:4]


@pytest.fixture(scope="module")
def corpus_ext():
    """the 100 examples/01 utterances with the recipe's 25 + 25 repeated context frames"""
    c = formats.read_corpus(os.path.join(EX, "test.scp"), os.path.join(EX, "test_3s.mlf"),
                            os.path.join(EX, "mono_state_phn_set_135_phn"))
    return [formats.extend_frames(x, tc.EX01_EXT, tc.EX01_EXT) for x in c.feats]


@pytest.fixture(scope="module")
def own(head_layers, corpus_ext):
    """float64 numpy statistics of what Network.propagate returns for the head transform (the same kernels and
    values the Normalizer sums), trimmed: first, second (fp32 squares), abs_sum"""
    net = tnet_amd.Network.from_layers(head_layers, precision=9)
    acc = tc.Accumulator(598, tc.EX01_EXT, tc.EX01_EXT, False)
    for xe in corpus_ext:
        acc.add(net.propagate(DeviceArray.from_numpy(xe)).numpy()[tc.EX01_EXT:-tc.EX01_EXT])
    assert acc.summed == tc.EX01_FRAMES
    return acc


def _run(head_layers, corpus_ext, how, count_ext):
    net = tnet_amd.Network.from_layers(head_layers, precision=9)
    nz = tnet_amd.Normalizer(net, start_ext=tc.EX01_EXT, end_ext=tc.EX01_EXT, count_ext_frames=count_ext)
    assert nz.dim == 598
    if how == "add":
        for xe in corpus_ext:
            nz.add(xe)
    else:
        cwd = os.getcwd()
        os.chdir(EX)
        try:
            r = tnet_amd.FeatureReader("test.scp", start_ext=tc.EX01_EXT, end_ext=tc.EX01_EXT)
            assert nz.add_reader(r) == tc.EX01_FRAMES
        finally:
            os.chdir(cwd)
    return nz


@pytest.fixture(scope="module")
def runs(head_layers, corpus_ext):
    """the four passes (add / add_reader x the two frame counts), finished"""
    out = {}
    for how in ("add", "reader"):
        for count_ext in (True, False):
            nz = _run(head_layers, corpus_ext, how, count_ext)
            nz.finish()
            out[how, count_ext] = nz
    return out


@pytest.mark.parametrize("count_ext", [True, False])
@pytest.mark.parametrize("how", ["add", "reader"])
def test_loop_vs_reference_fixture(runs, gold, how, count_ext):
    nz = runs[how, count_ext]
    first, second, frames = nz.stats()
    mode = "ext" if count_ext else "true"
    assert frames == int(gold[f"frames_{mode}"]) == (tc.EX01_FRAMES_EXT if count_ext else tc.EX01_FRAMES)
    n = tc.EX01_FRAMES
    df = np.abs(first - gold["first"]) / gold["abs_sum"]
    ds = np.abs(second - gold["second"]) / gold["second"]
    print(f"{how} {mode}: max |d first| / abs_sum = {df.max():.3e} (bound {T_REL + 2 * n * U64:.3e}), "
          f"max |d second| / second = {ds.max():.3e} (bound {2 * T_REL + 2 * n * U64:.3e})")
    assert (df <= T_REL + 2 * n * U64).all()
    assert (ds <= 2 * T_REL + 2 * n * U64).all()
    # bias / window follow from the sums by the restatement's own arithmetic, bit for bit
    bias, window = nz.vectors()
    eb, ew = tc.finish(first, second, frames)
    assert _bits_equal(bias, eb) and _bits_equal(window, ew)
    assert nz.bad_window_entries() == 0
    assert nz.report() == tc.report(frames, bias, window)


def test_add_and_reader_agree_bit_for_bit(runs):
    a, b = runs["add", True].stats(), runs["reader", True].stats()
    assert _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1]) and a[2] == b[2]
    c = runs["add", False].stats()
    assert _bits_equal(a[0], c[0]) and _bits_equal(a[1], c[1])   # the count changes N only


def test_loop_vs_own_output(runs, own):
    """the same values summed by numpy in float64: only the order of the double sums differs"""
    first, second, _ = runs["add", False].stats()
    n = tc.EX01_FRAMES
    df = np.abs(first - own.first) / own.abs_sum
    ds = np.abs(second - own.second) / own.second
    print(f"own output: max |d first| / abs_sum = {df.max():.3e}, max |d second| / second = {ds.max():.3e} "
          f"(bound {2 * n * U64:.3e})")
    assert (df <= 2 * n * U64).all() and (ds <= 2 * n * U64).all()


def test_text_normalises_the_corpus(runs, own, head_layers, corpus_ext, tmp_path):
    """.write() is the restatement's text of the vectors; head + norm assembled by tools/tnorm.py --assemble's cat loads
    as a Network; with the true frame count it gives the corpus per-column mean ~ 0 and variance ~ 1.

    Bounds (per column; u = 2^-24, t = (1 + 5e-6)(1 + u) - 1: six significant digits of text, then the float32 the
    network holds; mu, m2 = mean of y and of y^2, sigma^2 = m2 - mu^2 of the head's output y; w = the window):
      b^ = -mu (1 + d_b), w^ = w (1 + d_w), |d| <= t;  z = fl(fl(y + b^) w^) = (y + b^) w^ (1 + e), |e| <= 2u + u^2
      mean z  = w^ [ -mu d_b + mean((y + b^) e) ]            |mean z| <= w (1 + t) (|mu| t + 3u mean |y + b^|)
      the window was made from fp32 squares: second = sum y^2 (1 + eta), |eta| <= u, so w^2 sigma^2 = 1 +- u m2 w^2
      var z   = var of c (1 + e), c = (y + b^) w^ with var c = w^^2 sigma^2 in [A-, A+],
                A+- = (1 +- t)^2 (1 +- u m2 w^2);  sd z within 3u rms(c) of sd c, rms(c)^2 = var c + (mean c)^2
      |var z - 1| <= (A+ - 1) + 6u rms sqrt(A+) + (3u rms)^2
    plus 4 N 2^-53 for the float64 sums of the check itself."""
    nz = runs["add", False]
    bias, window = nz.vectors()
    norm_path, head_path, full_path = (str(tmp_path / n) for n in ("norm.nnet", "head.nnet", "full.nnet"))
    nz.write(norm_path)
    assert open(norm_path).read() == tc.norm_text(bias, window)
    formats.write_nnet(head_layers, head_path, precision=9)
    # the command line itself, once: the same pass over the script file in a process of its own
    tool_norm = str(tmp_path / "tool_norm.nnet")
    p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "tnorm.py"), "-S", "test.scp", "-H", head_path,
                        f"--TARGETMMF={tool_norm}", f"--STARTFRMEXT={tc.EX01_EXT}", f"--ENDFRMEXT={tc.EX01_EXT}",
                        "--true-frame-count", "--assemble", full_path], capture_output=True, text=True, cwd=EX,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert open(tool_norm).read() == open(norm_path).read()
    assert open(full_path).read() == open(head_path).read() + open(norm_path).read()
    assert nz.report() in p.stdout
    net = tnet_amd.Network(path=full_path)
    assert [c[0] for c in net.components()] == [L.tag for L in head_layers] + ["<bias>", "<window>"]
    # layers() is the same pair as the text to six digits
    L = nz.layers()
    back = formats.read_nnet(norm_path)
    np.testing.assert_allclose(back[0].b, L[0].b, rtol=1e-5)
    np.testing.assert_allclose(back[1].extra["window"], L[1].extra["window"], rtol=1e-5)

    n = tc.EX01_FRAMES
    zsum, zsq, absdev = np.zeros(598), np.zeros(598), np.zeros(598)
    bhat = back[0].b.astype(np.float64)
    head = tnet_amd.Network.from_layers(head_layers, precision=9)
    for xe in corpus_ext:
        X = DeviceArray.from_numpy(xe)
        z = net.propagate(X).numpy()[tc.EX01_EXT:-tc.EX01_EXT].astype(np.float64)
        y = head.propagate(X).numpy()[tc.EX01_EXT:-tc.EX01_EXT].astype(np.float64)
        zsum += z.sum(0)
        zsq += (z * z).sum(0)
        absdev += np.abs(y + bhat).sum(0)
    mean_z = zsum / n
    var_z = zsq / n - mean_z ** 2
    u = 2.0 ** -24
    t = (1 + 5e-6) * (1 + u) - 1
    mu, m2 = own.first / n, own.second / n
    mean_bound = window * (1 + t) * (np.abs(mu) * t + 3 * u * absdev / n) + 4 * n * U64
    a_plus = (1 + t) ** 2 * (1 + u * m2 * window ** 2)
    rms = np.sqrt(a_plus + mean_bound ** 2)
    var_bound = (a_plus - 1) + 6 * u * rms * np.sqrt(a_plus) + (3 * u * rms) ** 2 + 4 * n * U64 * (1 + mean_bound ** 2)
    print(f"normalised corpus: max |mean| / bound = {(np.abs(mean_z) / mean_bound).max():.3f}, "
          f"max |var - 1| / bound = {(np.abs(var_z - 1) / var_bound).max():.3f}; "
          f"max |mean| {np.abs(mean_z).max():.3e}, max |var - 1| {np.abs(var_z - 1).max():.3e}")
    assert (np.abs(mean_z) <= mean_bound).all()
    assert (np.abs(var_z - 1) <= var_bound).all()


def test_nan_names_the_utterance(head_layers, corpus_ext):
    net = tnet_amd.Network.from_layers(head_layers, precision=9)
    nz = tnet_amd.Normalizer(net, start_ext=tc.EX01_EXT, end_ext=tc.EX01_EXT)
    for k, xe in enumerate(corpus_ext[:44]):
        if k in (41, 43):
            xe = xe.copy()
            xe[xe.shape[0] // 2, 3] = np.nan
        nz.add(xe)
    with pytest.raises(tnet_amd.TnetError, match=r"nan/inf in accumulators\s+utterance index:41\b"):
        nz.finish()


def test_nan_from_a_reader_names_the_file(tmp_path):
    """no transform (dim = the feature dimension); the logical name comes from the reader"""
    rng = np.random.default_rng(3)
    names = ["a", "b", "c"]
    os.makedirs(tmp_path / "f")
    for k, nme in enumerate(names):
        x = rng.standard_normal((20 + k, 5)).astype(np.float32)
        if nme == "b":
            x[7, 2] = np.float32(1e20)   # finite, but its square is not
        formats.write_htk(str(tmp_path / "f" / (nme + ".fea")), x)
    open(tmp_path / "list.scp", "w").write("".join(f"f/{nme}.fea\n" for nme in names))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        r = tnet_amd.FeatureReader("list.scp", start_ext=2, end_ext=2)
        nz = tnet_amd.Normalizer(dim=5, start_ext=2, end_ext=2)
        assert nz.add_reader(r) == 20 + 21 + 22
    finally:
        os.chdir(cwd)
    with pytest.raises(tnet_amd.TnetError, match=r"nan/inf in accumulators\s+utterance index:1\s+utterance:f/b\.fea"):
        nz.finish()


def test_refusals():
    nz = tnet_amd.Normalizer(dim=4, start_ext=3, end_ext=2)
    with pytest.raises(tnet_amd.TnetError, match="5 rows cannot carry 3 \\+ 2 context rows"):
        nz.add(np.zeros((5, 4), np.float32))
    with pytest.raises(tnet_amd.TnetError, match="feature dim 3"):
        nz.add(np.zeros((9, 3), np.float32))
    nz.add(np.ones((6, 4), np.float32))        # one summed row
    first, second, frames = nz.stats()
    assert first.tolist() == [1.0] * 4 and second.tolist() == [1.0] * 4 and frames == 6
    with pytest.raises(tnet_amd.TnetError, match="already been fetched"):
        nz.add(np.ones((6, 4), np.float32))
    with pytest.raises(tnet_amd.TnetError, match="Finish"):
        nz.vectors()
    nz.finish()
    bias, window = nz.vectors()                # mean 1/6, variance 1/6 - 1/36
    assert _bits_equal(bias, np.full(4, (1.0 * (1.0 / 6)) * -1.0))
    with pytest.raises(ValueError):
        tnet_amd.Normalizer()
    # a constant column: zero variance, an infinite window as in the reference, counted, not clamped
    nz = tnet_amd.Normalizer(dim=2, count_ext_frames=False)
    nz.add(np.array([[2.0, 1.0], [2.0, 3.0]], np.float32))
    nz.finish()
    assert np.isinf(nz.vectors()[1][0]) and nz.bad_window_entries() == 1
    assert "max_window: inf" in nz.report()


def test_merge_over_a_host_communicator():
    """rank 0 holds list A, a second rank's recorded 2 D + 1 doubles (its first, second, N over list B) are added by the
    communicator's callback: the merged statistics are the one-pass statistics of A + B, bit for bit on integer data"""
    rng = np.random.default_rng(9)
    D, se, ee = 261, 2, 3
    A = [_ints(rng, rows, D) for rows in (40, 6, 2 * R + se + ee)]
    B = [_ints(rng, rows, D) for rows in (17, 90)]

    def run(utts):
        nz = tnet_amd.Normalizer(dim=D, start_ext=se, end_ext=ee)
        for x in utts:
            nz.add(x)
        return nz

    fb, sb, nb = run(B).stats()
    other = np.concatenate([fb, sb, [float(nb)]])
    calls = []

    def allreduce(a):
        if a.size == 2:          # the communicator's creation check: every rank contributes the same pair
            a *= 2
            return
        calls.append(a.size)
        a += other

    comm = tnet_amd.Comm.host(0, 2, allreduce)
    nz = run(A)
    nz.merge(comm)
    assert calls == [2 * D + 1]
    whole = run(A + B)
    fw, sw, nw = whole.stats()
    fm, sm, nm = nz.stats()
    assert nm == nw == sum(x.shape[0] for x in A + B)
    assert _bits_equal(fm, fw) and _bits_equal(sm, sw)
    ef, es = _expect([x[se:x.shape[0] - ee] for x in A + B], D)
    assert _bits_equal(fm, ef) and _bits_equal(sm, es)
    nz.finish()
    whole.finish()
    assert _bits_equal(nz.vectors()[0], whole.vectors()[0]) and _bits_equal(nz.vectors()[1], whole.vectors()[1])
    with pytest.raises(tnet_amd.TnetError, match="only before Finish"):
        nz.merge(comm)
    # a rank holding a bad utterance fails before the collective
    bad = run([np.full((8, D), np.nan, np.float32)])
    with pytest.raises(tnet_amd.TnetError, match="nan/inf in accumulators"):
        bad.merge(comm)
    assert calls == [2 * D + 1]
