"""Every branch of the fused SGD step's scheduler (CuNetwork::TrainBunch) on the GPU: per case of tests/step_cases.py
and per step, the launch tags the library reports (tnet_kernel_timing_report) equal the case's hand-written table --
so a pair launch that is silently declined fails here even though its two-call fallback computes the same -- and every
exposed output, every parameter and the objective's statistics equal the float64 restatement (stack_cases.Oracle).

Tolerances (step_cases.param_tolerance / output_tolerance): outputs and the small cases' parameters rtol 2e-4, atol
2e-6; large cases' parameters |W - W_ref| <= 2 ulp(W) + 1e-4 max|W_ref - W_init| per block, their top layer compared
through Y and not through its logits (as tests/test_gpu_fullsize.py); the objective's sum rtol 1e-5; frames and the
correct count exact.  The momentum buffers are not readable through the API: they are compared through the parameters of the
steps after the first.

The switch matrix runs one child process per TNET_* setting (tests/step_modes_worker.py), one after another; a child
that ends with anything but exit status 0 fails its test and every later matrix test at once."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle as orc  # noqa: E402
import stack_cases as sc  # noqa: E402
import step_cases as cases  # noqa: E402
import step_modes_worker as worker  # noqa: E402

_RESULTS = {}
_BROKEN = []      # a run that raised (a library error, not a failed comparison): nothing more is started on the GPU


def _guarded(fn, *args, **kw):
    if _BROKEN:
        pytest.fail(f"an earlier run raised ({_BROKEN[0]})")
    try:
        return fn(*args, **kw)
    except Exception as e:
        _BROKEN.append(repr(e)[:200])
        raise


def _run(name):
    """the default process's run of a case, once per module"""
    if name not in _RESULTS:
        _RESULTS[name] = _guarded(worker.run_case, cases.ALL_CASES[name])
    return _RESULTS[name]


def _check(case, res, tags=None, what=""):
    """tags, outputs, parameters and statistics of one run against the table and the restatement; prints the worst
    share of the tolerance before it asserts"""
    want_steps, ref = cases.reference(case)
    init = cases.initial_state(case)
    tags = case.tags if tags is None else tags
    f = sc.parse_factors(case.factors) or [1.0] * cases.n_layers(case)
    if case.runner.endswith("trainer"):
        want_steps = want_steps[-1:]          # the whole drain: the last step's parameters
    assert len(res["steps"]) == len(want_steps)
    worst = 0.0
    for s, ((outs, state, got_tags), (wo, ws, _)) in enumerate(zip(res["steps"], want_steps)):
        assert got_tags == tags, f"{what}{case.name} step {s}: tags {got_tags} != {tags}"
        for i, got in outs.items():
            share = float((np.abs(got - wo[i]) / cases.output_tolerance(wo[i], case, i)).max())
            worst = max(worst, share)
            assert share <= 1.0, f"{what}{case.name} step {s} output {i}: {share:.3g} tolerances"
        assert set(state) == set(ws)
        for key, w in ws.items():
            if not (case.train and f[int(key.split(".")[0]) // 2] > 0):
                np.testing.assert_array_equal(state[key], init[key].astype(np.float32), err_msg=f"{case.name} {key}")
                continue
            share = float((np.abs(state[key] - w) / cases.param_tolerance(case, key, w, init[key])).max())
            worst = max(worst, share)
            assert share <= 1.0, f"{what}{case.name} step {s} {key}: {share:.3g} tolerances"
    err, frames, correct = res["stats"]
    print(f"{what}{case.name}: worst deviation / tolerance = {worst:.3g}, objective {err:.9g} vs {ref.xent:.9g}")
    assert frames == ref.frames == sum(case.rows)
    assert correct == cases.reference(case)[0][-1][2]
    np.testing.assert_allclose(err, ref.xent, rtol=cases.OBJ_RTOL)


@pytest.mark.parametrize("name", list(cases.ALL_CASES))
def test_step_takes_the_tabled_launches_and_matches_the_restatement(name):
    case = cases.ALL_CASES[name]
    _check(case, _run(name))


@pytest.mark.parametrize("name", ["keep-output", "keep-output-wide"])
def test_keeping_the_output_changes_no_parameter(name):
    on, off = _run(name + "-on"), _run(name + "-off")
    for (_, a, _), (_, b, _) in zip(on["steps"], off["steps"]):
        for key in a:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert on["stats"] == off["stats"]


@pytest.mark.parametrize("name", ["fused-top-cap", "pair-narrow"])
def test_kernel_timing_changes_no_parameter(name):
    timed = _run(name)
    plain = _guarded(worker.run_case, cases.ALL_CASES[name], timed=False)
    for (oa, a, _), (ob, b, tags) in zip(timed["steps"], plain["steps"]):
        assert tags == {}
        for key in a:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        for i in oa:
            np.testing.assert_array_equal(oa[i], ob[i], err_msg=f"output {i}")
    assert timed["stats"] == plain["stats"]


@pytest.mark.parametrize("name,local", [("dp-pair-narrow", "pair-narrow"), ("dp-mlp3", "gather-tail-mlp3")])
def test_one_rank_data_parallel_step_equals_the_local_step(name, local):
    """the same bunches through the exchange (gradient GEMMs, reduction over one rank, flat SGD apply) and through the
    fused update GEMMs: each within the tolerance of the restatement (above), and of each other"""
    case = cases.ALL_CASES[name]
    _, ws, _ = cases.reference(case)[0][-1]
    init = cases.initial_state(case)
    a, b = _run(name)["steps"][-1][1], _run(local)["steps"][-1][1]
    for key, w in ws.items():
        share = float((np.abs(a[key].astype(np.float64) - b[key]) / cases.param_tolerance(case, key, w, init[key])).max())
        assert share <= 1.0, (key, share)


_RBM_EXPECTED = {}


def _check_rbm(name, res, what=""):
    """as tests/test_gpu_rbm.py::test_rbm_trainer_epoch_matches_oracle, at its tolerances"""
    if name not in _RBM_EXPECTED:
        layer, feats, B, cache = cases.rbm_corpus(name)
        rs = orc.RandState(cases.RBM_SEED, B, layer.n_out)
        X = np.concatenate(feats)
        sched = orc.epoch_schedule_x([len(f) for f in feats], cache, B, rs.x_after)
        m = orc.RBM.from_layer(layer)
        for b in sched:
            m.step(X[b], rs, cases.RBM_LR, cases.RBM_MMT, cases.RBM_WC)
        _RBM_EXPECTED[name] = (m, len(sched))
    m, nb = _RBM_EXPECTED[name]
    mse, frames, steps = res["stats"]
    got = res["steps"][0][1]
    assert steps == nb and frames == m.frames, what
    np.testing.assert_allclose(mse, m.mse, rtol=1e-4, err_msg=what)
    for key, want in (("W", m.W), ("vb", m.vb), ("hb", m.hb)):
        np.testing.assert_allclose(got[key], want, rtol=2e-4, atol=2e-6, err_msg=f"{what}{name} {key}")


def _check_rnn(name, res, what=""):
    """as tests/test_gpu_rnn.py::test_rnn_strict_parity_mode compares a trainer with oracle.RNN, at its tolerances"""
    layers, feats, labels, bptt = cases.rnn_corpus(name)
    m = orc.RNN(layers[0].W, layers[0].b, layers[1].W, layers[1].b)
    for f, l in zip(feats, labels):
        m.utterance(f, l, bptt, cases.RNN_LR, cases.RNN_MMT, cases.RNN_WC)
    err, frames, correct = res["stats"]
    got = res["steps"][0][1]
    assert frames == m.frames == sum(len(l) for l in labels), what
    np.testing.assert_allclose(err, m.xent, rtol=1e-4, err_msg=what)
    assert abs(correct - m.correct) <= 1
    for key, want in (("Wr", m.Wr), ("br", m.br), ("W2", m.W2), ("b2", m.b2)):
        np.testing.assert_allclose(got[key], want, rtol=2e-3, atol=2e-5, err_msg=f"{what}{name} {key}")


# ---- the switch matrix
_CHILD = {"died": None, "results": {}}


def _child(env, tmp_path_factory):
    """the child's results under `env` ("NAME=value", or "" for the default), run once per module"""
    if env in _CHILD["results"]:
        return _CHILD["results"][env]
    if _CHILD["died"] is not None:
        pytest.fail(f"an earlier child died ({_CHILD['died']})")
    if _BROKEN:
        pytest.fail(f"an earlier run raised ({_BROKEN[0]})")
    out = str(tmp_path_factory.mktemp("step_modes") / "out.npz")
    e = dict(os.environ)
    if env:
        k, v = env.split("=")
        e[k] = v
    names = ",".join(cases.SETTINGS[env].cases)
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "step_modes_worker.py"), out, names], env=e,
                           timeout=120, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _CHILD["died"] = f"{env or 'default'}: timeout"
        pytest.fail(f"the child under {env or 'the default'} ran into its time limit")
    if p.returncode != 0:
        # by a signal, or by a library error raised in the child (a HIP error surfaces so): either way no further
        # child is started on this GPU
        how = f"signal {-p.returncode}" if p.returncode < 0 else f"exit status {p.returncode}"
        _CHILD["died"] = f"{env or 'default'}: {how}"
        pytest.fail(f"the child under {env or 'the default'} ended with {how}\n{p.stderr[-4000:]}")
    with np.load(out) as z:
        _CHILD["results"][env] = worker.unpack(z)
    return _CHILD["results"][env]


@pytest.mark.parametrize("env", list(cases.SETTINGS))
def test_switch_matrix(env, tmp_path_factory):
    """each setting's cases against the restatement at the default's tolerances and against the setting's tag table;
    where step_cases names a case bit-identical to the default, its parameters equal the default child's bit for bit"""
    setting = cases.SETTINGS[env]
    results = _child(env, tmp_path_factory)
    assert set(results) == set(setting.cases)
    for name in setting.cases:
        if name in cases.RBM:
            _check_rbm(name, results[name], what=f"[{env or 'default'}] ")
            continue
        if name in cases.RNN:
            _check_rnn(name, results[name], what=f"[{env or 'default'}] ")
            continue
        _check(cases.ALL_CASES[name], results[name], cases.setting_tags(env, name), what=f"[{env or 'default'}] ")
    if setting.bit_equal_default:
        default = _child("", tmp_path_factory)
        for name in setting.bit_equal_default:
            for (_, a, _), (_, b, _) in zip(results[name]["steps"], default[name]["steps"]):
                for key in a:
                    np.testing.assert_array_equal(a[key], b[key], err_msg=f"{env} {name} {key}")
            assert results[name]["stats"] == default[name]["stats"]
