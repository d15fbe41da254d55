"""The normalisation pass without a GPU: the reference fixture (tests/golden/tnorm_ex01.npz, made by
tests/golden/make_tnorm.py from the reference CPU TFeaCat's output) against the identities of the float64 restatement
(tests/tnorm_cases.py), the norm file's text through formats.read_nnet, and the command line of tools/tnorm.py."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import tnorm_cases as tc
from tnet_amd import formats

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tools", "tnorm.py")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "tnorm_ex01.npz"))


def test_fixture_frame_counts_and_identities(gold):
    """N = 60,457 (the quirk) and 55,457; bias / window recomputed from the stored sums bit for bit; the quirk
    scales the mean by 55457 / 60457; Cauchy-Schwarz and |first| <= abs_sum hold column by column"""
    assert int(gold["summed"]) == tc.EX01_FRAMES == int(gold["frames_true"])
    assert int(gold["frames_ext"]) == tc.EX01_FRAMES_EXT == tc.EX01_FRAMES + 100 * 2 * tc.EX01_EXT
    first, second, abs_sum = gold["first"], gold["second"], gold["abs_sum"]
    assert first.shape == second.shape == abs_sum.shape == (598,)
    assert (np.abs(first) <= abs_sum).all() and (second > 0).all()
    assert (abs_sum ** 2 <= second * tc.EX01_FRAMES * (1 + 1e-6)).all()     # (sum |y|)^2 <= n sum y^2
    for mode in ("ext", "true"):
        bias, window = tc.finish(first, second, int(gold[f"frames_{mode}"]))
        np.testing.assert_array_equal(bias, gold[f"bias_{mode}"])
        np.testing.assert_array_equal(window, gold[f"window_{mode}"])
        assert np.isfinite(window).all() and (window > 0).all()
    np.testing.assert_allclose(gold["bias_ext"], gold["bias_true"] * (tc.EX01_FRAMES / tc.EX01_FRAMES_EXT), rtol=1e-14)
    # with the true count the normalised corpus has unit variance: second/n - mean^2 = 1/window^2
    mean = first / tc.EX01_FRAMES
    np.testing.assert_allclose(second / tc.EX01_FRAMES - mean * mean, gold["window_true"] ** -2.0, rtol=1e-12)


def test_restatement_fp32_square_and_counts():
    """moments() squares in float32: 1 + 2^-12 squares to 1 + 2^-11 exactly (the tie rounds to even), where a double
    square keeps the 2^-24; the two frame counts"""
    y = np.full((7, 3), 1 + 2.0 ** -12, np.float32)
    first, second, abs_sum = tc.moments(y)
    assert (first == 7 * (1 + 2.0 ** -12)).all() and (abs_sum == first).all()
    assert (second == 7 * (1 + 2.0 ** -11)).all()
    assert ((y.astype(np.float64) ** 2).sum(0) == 7 * (1 + 2.0 ** -11 + 2.0 ** -24)).all()
    for count_ext, n in ((True, 7 + 4 + 12), (False, 7 + 4)):
        a = tc.Accumulator(3, 2, 4, count_ext)
        a.add(y)
        a.add(y[:4])
        assert (a.frames, a.summed) == (n, 11)
    bias, window = tc.finish([2.0, 0.0, 4.0], [4.0, 0.0, 4.0], 2)   # variances 1, 0, -2
    assert bias.tolist() == [-1.0, -0.0, -2.0]
    assert window[0] == 1.0 and np.isinf(window[1]) and np.isnan(window[2])


@pytest.mark.parametrize("mode", ["ext", "true"])
def test_text_parses_back(gold, mode):
    """the reference's text: header lines, 'v D  ' vectors of 6 significant digits, blank lines; read_nnet returns
    the stored vectors within one unit of the sixth digit"""
    text = str(gold[f"text_{mode}"])
    assert text == tc.norm_text(gold[f"bias_{mode}"], gold[f"window_{mode}"])
    lines = text.split("\n")
    assert lines[0] == "<bias> 598 598" and lines[3] == "<window> 598 598"
    assert lines[1].startswith("v 598  ") and lines[1].endswith(" ") and lines[4].startswith("v 598  ")
    assert lines[2] == "" and lines[5] == "" and lines[6] == "" and len(lines) == 7
    layers = formats.read_nnet(text)
    assert [(L.tag, L.n_out, L.n_in) for L in layers] == [("<bias>", 598, 598), ("<window>", 598, 598)]
    for got, want in ((layers[0].b, gold[f"bias_{mode}"]), (layers[1].extra["window"], gold[f"window_{mode}"])):
        # six significant digits: half a unit of the sixth digit is relative 5e-6; one unit bounds it, with the
        # float32 rounding of the parsed value (6e-8) inside
        assert (np.abs(np.asarray(got, np.float64) - want) <= 1e-5 * np.abs(want)).all()


def test_fmt_double_is_percent_g():
    assert [tc.fmt_double(x) for x in (0.0, -544.1169797, 1e-5, 123456789.0, float("inf"), float("nan"),
                                       -float("nan"))] == ["0", "-544.117", "1e-05", "1.23457e+08", "inf", "nan",
                                                           "-nan"]
    assert tc.fmt_vector([1.0, 0.5]) == "v 2  1 0.5 "
    assert tc.report(60457, np.array([-1.0, 2.5]), np.array([0.25, 4.0])) == \
        "frames: 60457, max_bias: 2.5, max_window: 4, min_window: 0.25\n"


def _tool():
    spec = importlib.util.spec_from_file_location("tnorm_tool", TOOL)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_tool_help_runs_without_gpu():
    p = subprocess.run([sys.executable, TOOL, "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    for word in ("-S", "-H", "--TARGETMMF", "--STARTFRMEXT", "--ENDFRMEXT", "--NATURALREADORDER", "--CMEANDIR",
                 "--CMEANMASK", "--VARSCALEDIR", "--VARSCALEMASK", "--VARSCALEFN", "--true-frame-count", "--assemble"):
        assert word in p.stdout, word
    assert "60,457" in p.stdout or "context" in p.stdout   # the quirk is stated in the help


def test_tool_argument_parsing():
    t = _tool()
    a = t.parse_args(["-S", "train.scp", "-H", "hamm_dct.nnet", "--TARGETMMF=norm.nnet", "--STARTFRMEXT=25",
                      "--ENDFRMEXT", "25"])
    assert (a.script, a.mmf, a.targetmmf, a.startfrmext, a.endfrmext) == ("train.scp", "hamm_dct.nnet", "norm.nnet",
                                                                          25, 25)
    assert a.naturalreadorder is False and a.true_frame_count is False and a.assemble is None
    assert a.cmeanmask is None and a.varscalefn is None
    a = t.parse_args(["-S", "x.scp", "-H", "t.nnet", "--TARGETMMF", "n", "--NATURALREADORDER=TRUE",
                      "--true-frame-count", "--assemble", "full.nnet", "--CMEANDIR=cmn", "--CMEANMASK=%%%.fea",
                      "--VARSCALEDIR=cvn", "--VARSCALEMASK=%%%.fea", "--VARSCALEFN=cvg"])
    assert a.naturalreadorder is True and a.true_frame_count is True and a.assemble == "full.nnet"
    assert (a.cmeandir, a.cmeanmask, a.varscaledir, a.varscalemask, a.varscalefn) == ("cmn", "%%%.fea", "cvn",
                                                                                      "%%%.fea", "cvg")
    with pytest.raises(SystemExit):
        t.parse_args(["-S", "x.scp", "--TARGETMMF=n"])          # Source MMF must be specified [-H]
    with pytest.raises(SystemExit):
        t.parse_args(["-S", "x.scp", "-H", "t", "--TARGETMMF=n", "--STARTFRMEXT=-1"])


def test_tool_assemble_text(tmp_path):
    """--assemble is the scheduler's `cat $MMF $NORM`"""
    t = _tool()
    mmf, norm, out = (str(tmp_path / n) for n in ("t.nnet", "norm.nnet", "full.nnet"))
    open(mmf, "w").write("<window> 2 2\nv 2  1 2 \n")
    open(norm, "w").write(tc.norm_text(np.array([-1.0, 0.5]), np.array([2.0, 4.0])))
    t.assemble(mmf, norm, out)
    assert open(out).read() == open(mmf).read() + open(norm).read()
    layers = formats.read_nnet(out)
    assert [L.tag for L in layers] == ["<window>", "<bias>", "<window>"]
