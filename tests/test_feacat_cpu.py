"""The forward pass without a GPU: the float64 restatement (tests/feacat_cases.py) against the reference fixture
tests/golden/feacat_ref.npz (tests/golden/make_feacat.py: the reference CPU TFeaCat in its four output modes), the host
HTK writer tnet_htk_write against the reference's own file, the file-name rule, the packing plan and the command
line of tools/tfeacat.py.

The `log` finding.  TFeaCatCu.cc:247 / :256 call log() on a float.  Which overload that is decides the arithmetic:
the fixture's LOGPOSTERIOR, GMMBYPASS and both-mode outputs equal the fp64 form -- (float) log((double) y), (float)
sqrt(-2.0 * log((double) y)), the second mode acting on the first's fp32 result -- BIT FOR BIT on the utterances
stored in full (test_mode_function_reproduces_the_reference asserts equality, not a tolerance); the fp32 form
differs from the fixture in about 3 % (log) and 15 % (bypass) of the elements.
"""
import importlib.util
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import feacat_cases as fc
import tnet_amd
from tnet_amd import formats

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tools", "tfeacat.py")
FULL = ("040", "086")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(REPO, "tests", "golden", "feacat_ref.npz"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------- the mode function

@pytest.mark.parametrize("mode", [m for m in fc.MODES if m])
@pytest.mark.parametrize("name", FULL)
def test_mode_function_reproduces_the_reference(gold, mode, name):
    """bit equality on the full utterances: the reference's log is the double one"""
    y = gold[f"none_Y_{name}"]
    ref = gold[f"{fc.MODE_NAMES[mode]}_Y_{name}"]
    assert y.shape == ref.shape and y.shape[1] == 135
    assert np.array_equal(_bits(fc.mode_fn(y, mode)), _bits(ref))


def test_fp32_log_is_not_the_reference(gold):
    """the other overload would have shown: the fixture can tell the two apart"""
    y = gold["none_Y_040"]
    assert np.count_nonzero(_bits(np.log(y)) != _bits(gold["logposterior_Y_040"])) > 0


def test_fixture_shapes_and_sums(gold):
    """rows / header fields are those of the input whatever the mode; the stored sums are the full utterances'"""
    names = [str(n) for n in gold["names"]]
    for mode in fc.MODE_NAMES.values():
        assert np.array_equal(gold[f"{mode}_rows"], gold["none_rows"])
        assert set(gold[f"{mode}_kind"]) == {formats.HTK_USER} and set(gold[f"{mode}_size"]) == {4 * 135}
        assert np.array_equal(gold[f"{mode}_period"], gold["none_period"])
        assert not gold[f"{mode}_nonfinite"].any()
        for n in FULL:
            y = gold[f"{mode}_Y_{n}"].astype(np.float64)
            k = names.index(n)
            assert y.shape[0] == gold[f"{mode}_rows"][k]
            assert y.sum() == gold[f"{mode}_sum"][k] and (y ** 2).sum() == gold[f"{mode}_sumsq"][k]


def test_mode_function_edge_values():
    """0 -> -inf / +inf; 1 -> +0 (log) and -0 (bypass: -2.0 * +0.0 = -0.0 and sqrt(-0.0) = -0.0, IEEE 754 6.3);
    the bypass's -0 then logs to -inf; negative -> NaN; NaN and +inf propagate (sqrt(-2 * inf) = sqrt(-inf) = NaN)"""
    y = fc.SPECIALS  # 0, -0, 1, denormal, -0.5, NaN, +inf
    lg = fc.mode_fn(y, fc.LOGPOSTERIOR)
    assert lg[0] == -np.inf and lg[1] == -np.inf and _bits(lg[2:3])[0] == 0x00000000
    assert np.isfinite(lg[3]) and abs(lg[3] - np.float32(-149 * np.log(2.0))) <= 1e-5
    assert np.isnan(lg[4]) and np.isnan(lg[5]) and lg[6] == np.inf
    bp = fc.mode_fn(y, fc.GMMBYPASS)
    assert bp[0] == np.inf and bp[1] == np.inf and _bits(bp[2:3])[0] == 0x80000000
    assert np.isfinite(bp[3]) and np.isnan(bp[4]) and np.isnan(bp[5]) and np.isnan(bp[6])
    both = fc.mode_fn(y, fc.GMMBYPASS | fc.LOGPOSTERIOR)
    assert both[0] == np.inf and both[2] == -np.inf and np.isnan(both[4:]).all()


# ------------------------------------------------------------------------------------------- the HTK writer

def test_htk_write_is_the_references_file(gold, tmp_path):
    """the same matrix, the same header fields: byte-identical to the file the reference wrote (big-endian), and in
    host order the same fields and words unswapped"""
    ref = gold["file_gmmbypass_040"].tobytes()
    Y = gold["gmmbypass_Y_040"]
    k = [str(n) for n in gold["names"]].index("040")
    period = int(gold["gmmbypass_period"][k])
    big, native = str(tmp_path / "big.fea"), str(tmp_path / "native.fea")
    tnet_amd.htk_write(big, Y, sample_period=period, kind=formats.HTK_USER, swap=True)
    assert open(big, "rb").read() == ref
    tnet_amd.htk_write(native, Y, sample_period=period, kind=formats.HTK_USER, swap=False)
    n, per, size, kind = struct.unpack(">iihh", ref[:12])
    want = struct.pack("<iihh", n, per, size, kind) + np.frombuffer(ref[12:], ">u4").astype("<u4").tobytes()
    assert open(native, "rb").read() == want
    # and the project's own Python writer agrees with both
    formats.write_htk(str(tmp_path / "py.fea"), Y, period, formats.HTK_USER)
    assert open(tmp_path / "py.fea", "rb").read() == ref


@pytest.mark.parametrize("rows,cols,period", [(0, 3, 100000), (1, 1, 1), (7, 135, 100000), (3, 8191, 625)])
def test_htk_header_round_trip(tmp_path, rows, cols, period):
    rng = np.random.default_rng(rows * 10000 + cols)
    Y = rng.standard_normal((rows, cols)).astype(np.float32)
    path = str(tmp_path / "y.fea")
    tnet_amd.htk_write(path, Y, sample_period=period)
    assert formats.read_htk_header(path) == (rows, period, 4 * cols, formats.HTK_USER)
    assert os.path.getsize(path) == 12 + 4 * rows * cols
    assert np.array_equal(_bits(formats.read_htk(path)), _bits(Y))


def test_htk_write_refuses_what_the_header_cannot_hold(tmp_path):
    """8192 columns are 32768 bytes a sample: the int16 field would read -32768 (the reference writes that)"""
    path = str(tmp_path / "wide.fea")
    with pytest.raises(tnet_amd.TnetError, match="8192"):
        tnet_amd.htk_write(path, np.zeros((1, 8192), np.float32))
    assert not os.path.exists(path)


def test_htk_write_names_the_file_it_cannot_create(tmp_path):
    path = str(tmp_path / "no_such_dir" / "y.fea")
    with pytest.raises(tnet_amd.TnetError, match="no_such_dir/y.fea"):
        tnet_amd.htk_write(path, np.zeros((2, 3), np.float32))


# ------------------------------------------------------------------------------------------- names and packs

@pytest.mark.parametrize("args,want", fc.FILE_NAME_CASES)
def test_file_name_rule(args, want):
    assert fc.make_htk_file_name(*args) == want


@pytest.mark.parametrize("lengths,pack_rows", [
    ([1, 2, 63, 64, 65, 300], 128),      # the GPU loop test's corpus: the 300-row utterance straddles three packs
    ([5], 128), ([128], 128), ([129], 128), ([128, 128], 128), ([1] * 300, 7), ([1000, 1, 1000], 256),
    ([3, 4], 1), ([10, 20, 30], 10 ** 6)])
def test_packing_plan_invariants(lengths, pack_rows):
    packs = fc.plan(lengths, pack_rows)
    total = sum(lengths)
    assert len(packs) == -(-total // pack_rows)
    seen = {u: 0 for u in range(len(lengths))}
    last = (-1, -1)
    for k, pack in enumerate(packs):
        fill = 0
        for u, utt_row, pack_row, rows in pack:
            assert rows > 0 and pack_row == fill          # back to back, no holes
            assert utt_row == seen[u]                     # every row exactly once, in order within the utterance
            assert (u, utt_row) > last                    # and utterances in the order they came
            last = (u, utt_row)
            seen[u] += rows
            fill += rows
        assert fill <= pack_rows
        assert fill == pack_rows or k == len(packs) - 1   # only the last pack may be short
    assert [seen[u] for u in range(len(lengths))] == list(lengths)


def test_packing_plan_straddle():
    packs = fc.plan([1, 2, 63, 64, 65, 300], 128)
    assert [sorted({u for u, *_ in p}) for p in packs] == [[0, 1, 2, 3], [3, 4, 5], [5], [5]]


# ------------------------------------------------------------------------------------------- the tool

def _tool():
    spec = importlib.util.spec_from_file_location("tfeacat_tool", TOOL)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_tool_help_runs_without_gpu():
    p = subprocess.run([sys.executable, TOOL, "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    for word in ("-S", "-H", "--FEATURETRANSFORM", "-l", "--TARGETPARAMDIR", "-y", "--TARGETPARAMEXT", "--GMMBYPASS",
                 "--LOGPOSTERIOR", "--STARTFRMEXT", "--ENDFRMEXT", "--NATURALREADORDER", "--CMEANDIR", "--CMEANMASK",
                 "--VARSCALEDIR", "--VARSCALEMASK", "--VARSCALEFN", "-T", "--rank", "--world"):
        assert word in p.stdout, word


def test_tool_defaults_and_booleans():
    t = _tool()
    a = t.parse_args(["-S", "test.scp", "-H", "final.nnet"])
    assert (a.targetparamext, a.targetparamdir, a.featuretransform) == ("fea", None, None)
    assert (a.gmmbypass, a.logposterior, a.naturalreadorder) == (False, False, False)
    assert (a.startfrmext, a.endfrmext, a.rank, a.world, a.trace, a.files) == (0, 0, 0, 1, 0, [])
    a = t.parse_args(["-H", "n.nnet", "--GMMBYPASS=TRUE", "--LOGPOSTERIOR", "--NATURALREADORDER=false", "-l", "out",
                      "-y", "post", "--STARTFRMEXT=25", "--ENDFRMEXT", "25", "--rank", "3", "--world", "8", "-T", "1",
                      "--FEATURETRANSFORM=t.nnet", "a.fea", "b.fea"])
    assert (a.gmmbypass, a.logposterior, a.naturalreadorder) == (True, True, False)
    assert (a.targetparamdir, a.targetparamext, a.startfrmext, a.endfrmext) == ("out", "post", 25, 25)
    assert (a.rank, a.world, a.trace, a.featuretransform, a.files) == (3, 8, 1, "t.nnet", ["a.fea", "b.fea"])
    for bad in (["-S", "x.scp"],                                     # -H missing
                ["-H", "n.nnet"],                                    # no input at all
                ["-S", "x.scp", "-H", "n.nnet", "--GMMBYPASS=maybe"],
                ["-S", "x.scp", "-H", "n.nnet", "--STARTFRMEXT=-1"],
                ["-S", "x.scp", "-H", "n.nnet", "--rank", "2", "--world", "2"]):
        with pytest.raises(SystemExit):
            t.parse_args(bad)


def test_tool_record_order_and_sharding(tmp_path):
    """the command line's files first, then the script's lines (TFeaCatCu.cc:175-205); a rank takes every N-th"""
    t = _tool()
    scp = tmp_path / "x.scp"
    scp.write_text("s1.fea\n\ns2.fea\ns3.fea\n")
    recs = t.records(str(scp), ["p1.fea", "p2.fea"])
    assert recs == ["p1.fea", "p2.fea", "s1.fea", "s2.fea", "s3.fea"]
    shards = [tnet_amd.shard_utterances(recs, r, 2) for r in range(2)]
    assert shards == [["p1.fea", "s1.fea", "s3.fea"], ["p2.fea", "s2.fea"]]
