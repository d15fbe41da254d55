"""CPU-side checks that make tests/step_cases.py trustworthy on its own (no GPU): run in float32 numpy the restatement
stays within a quarter of the GPU comparison's tolerance for every case; the uniform-rate cases agree with the C
oracle (oracle.MLP.step); three deliberately wrong restatements each leave the right one by at least ten tolerances, so
the comparison can tell them apart; every trained parameter block moves by many tolerances; and every tag table is
well-formed.  The tests print their figures; tests/step_cases.py's docstring holds a copy."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle as orc  # noqa: E402
import stack_cases as sc  # noqa: E402
import step_cases as cases  # noqa: E402

NAMES = list(cases.ALL_CASES)
SENSITIVITY = 10.0


def test_case_table():
    c = cases.CASES
    assert all(x.rows == sc.ROWS for x in cases.SMALL if x.name not in ("top-split", "colsum-declined"))
    assert sc.ROWS == (32, 19, 64, 1) and min(c["colsum-declined"].rows) > 8192 and c["colsum-declined"].dims[-1] > 256
    assert c["top-split"].dims[-2] in (512, 768, 1024) and c["top-split"].dims[-1] <= 256 and min(c["top-split"].rows) >= 64
    assert c["fused-top-cap"].dims[-1] == 256 and c["three-call-top"].dims[-1] == 257
    assert all(len(x.rows) == 2 and x.large for x in cases.LARGE)
    assert {x.consts for x in cases.ALL_CASES.values()} == set(sc.CONSTS)      # all four combinations are used
    for name in ("keep-output", "keep-output-wide"):
        on, off = c[name + "-on"], c[name + "-off"]
        assert on.keep and not off.keep and on._replace(name="", keep=False) == off._replace(name="")
    # small widths are no multiples of 32 unless a gate needs it (the 256-class cap, the K = 512 top)
    for x in cases.SMALL:
        assert all(d % 32 or d in (256, 512) for d in x.dims), x.name


def _f32(case):
    s32, r32 = cases.run_oracle(case, dtype=np.float32)
    assert all(v.dtype == np.float32 for v in s32[-1][1].values())
    return s32, r32


@pytest.mark.parametrize("name", NAMES)
def test_float32_restatement_stays_within_a_quarter_of_the_tolerance(name):
    """... and the steps move every trained parameter block by at least ten times the comparison's tolerance, leave
    every frozen one bit-equal, and the correct count is decided by a margin float32 cannot flip"""
    case = cases.ALL_CASES[name]
    s64, r64 = cases.reference(case)
    s32, r32 = _f32(case)
    share = cases.worst_share(case, s32, r32.xent)
    print(f"float32 headroom {name}: worst deviation / tolerance = {share:.3g}")
    assert share <= sc.HEADROOM
    assert r32.frames == r64.frames == sum(case.rows)
    assert s32[-1][2] == s64[-1][2]
    init, last = cases.initial_state(case), s64[-1][1]
    f = sc.parse_factors(case.factors) or [1.0] * cases.n_layers(case)
    for key, v in last.items():
        assert np.isfinite(v).all()
        trained = case.train and f[int(key.split(".")[0]) // 2] > 0
        if not trained:
            np.testing.assert_array_equal(v, init[key], err_msg=key)
            continue
        moved = float((np.abs(v - init[key]) / cases.param_tolerance(case, key, v, init[key])).max())
        assert moved >= SENSITIVITY, f"{key} moved by {moved:.3g} tolerances"
    # the correct count is exact: in no row does the label's output lie within twice the outputs' tolerance of the
    # largest other output, so an output inside its tolerance cannot change whether the label is the row's maximum
    for (outs, _, _), (_, lab) in zip(s64, cases.data(case)):
        Y = outs[-1].copy()
        own = Y[np.arange(len(lab)), lab].copy()
        Y[np.arange(len(lab)), lab] = -1.0
        other = Y.max(axis=1)
        assert (np.abs(own - other) > 2 * cases.output_tolerance(np.maximum(own, other))).all()


UNIFORM = [n for n in NAMES if cases.ALL_CASES[n].factors is None and cases.ALL_CASES[n].train]


def _oracle_mlp_share(case, dtype=np.float32):
    """the C oracle's trajectory against the restatement: worst relative deviation of any parameter, and the worst
    share of the comparison's tolerance"""
    L = cases.layers(case)
    k = cases.consts(case)
    ref = orc.MLP.from_layers(L, dtype)
    steps, _ = cases.reference(case)
    init = cases.initial_state(case)
    rel = share = 0.0
    for (X, lab), (_, st, _) in zip(cases.data(case), steps):
        ref.step(X, lab, k["lr"], mmt=k["mmt"], wc=k["wc"], graddivfrm=k["gdf"])
        for l in range(len(ref.W)):
            for key, got in ((f"{2 * l}.W", ref.W[l]), (f"{2 * l}.b", ref.b[l])):
                d = np.abs(got - st[key])
                rel = max(rel, float(d.max() / np.abs(st[key]).max()))
                share = max(share, float((d / cases.param_tolerance(case, key, st[key], init[key])).max()))
    return rel, share, ref


def test_uniform_rate_cases_agree_with_the_c_oracle_to_1e_12():
    """oracle.MLP.step -- tnet_oracle.c's orc_mlp_step, pinned by the reference CPU TNet -- built with double storage
    (liboracle64.so: the same source, -DORC_DOUBLE) against the float64 restatement: worst |oracle - restatement| /
    max|restatement| per parameter block <= 1e-12 over every uniform-rate case, the objective's sum and the correct
    count too.  So the restatement IS the oracle's algorithm, not merely close to it.  (With its usual float32
    storage the oracle can agree to float32 rounding only, measured 1.0e-7 to 3.0e-7;
    test_c_oracle_within_the_float32_headroom bounds that.)"""
    worst = {}
    for name in UNIFORM:
        case = cases.ALL_CASES[name]
        worst[name], _, ref = _oracle_mlp_share(case, np.float64)
        steps, r64 = cases.reference(case)
        print(f"C oracle (double storage) vs restatement {name}: worst relative deviation = {worst[name]:.3g}")
        assert ref.W[0].dtype == np.float64
        assert abs(ref.xent - r64.xent) <= 1e-12 * abs(r64.xent), name
        assert ref.correct == steps[-1][2] and ref.frames == r64.frames
    assert max(worst.values()) <= 1e-12, worst


@pytest.mark.parametrize("name", UNIFORM)
def test_c_oracle_within_the_float32_headroom(name):
    """oracle.MLP.step is a float32 program (double accumulation inside its products, float32 storage), pinned by the
    reference CPU TNet: like the float32 numpy restatement it must stay within stack_cases.HEADROOM of the
    comparison's tolerance of the float64 restatement, and its objective sum within rtol 1e-5 * HEADROOM"""
    case = cases.ALL_CASES[name]
    rel, share, ref = _oracle_mlp_share(case)
    _, r64 = cases.reference(case)
    share = max(share, abs(ref.xent - r64.xent) / (cases.OBJ_RTOL * abs(r64.xent)))
    print(f"C oracle vs restatement {name}: worst deviation / tolerance = {share:.3g}")
    assert share <= sc.HEADROOM
    assert ref.correct == cases.reference(case)[0][-1][2] and ref.frames == r64.frames


@pytest.mark.parametrize("name", NAMES)
def test_wrong_restatements_leave_the_tolerance(name):
    case = cases.ALL_CASES[name]
    applicable = [v for v in cases.WRONG if cases.wrong_applies(case, v)]
    if cases.n_layers(case) > 1 and case.factors is None and case.train:
        assert applicable == ["post-update-backward"]
    for variant in applicable:
        steps, ref = cases.run_oracle(case, cases.WRONG[variant])
        ratio = cases.worst_share(case, steps, ref.xent)
        print(f"sensitivity {name} {variant}: worst deviation / tolerance = {ratio:.3g}")
        assert ratio >= SENSITIVITY, (variant, ratio)


def test_every_wrong_restatement_is_exercised():
    for variant in cases.WRONG:
        assert sum(cases.wrong_applies(c, variant) for c in cases.ALL_CASES.values()) >= 1, variant
    # the learn-rate factor case of tests/test_gpu_train.py: all three apply
    assert all(cases.wrong_applies(cases.CASES["stopper-middle"], v) for v in cases.WRONG)


# ---- the tag tables
def _layer_roles(tags):
    """per shape KxN how often it appears as forward, backward, update / gradient"""
    roles = {"fwd": Counter(), "bwd": Counter(), "upd": Counter(), "other": Counter()}
    for tag, n in tags.items():
        kind, _, shapes = tag.partition(":")
        parts = kind.split("+")
        assert parts[0].startswith("gemm_") or kind in ("softmax_xent", "colsum", "gather", "bias_update",
                                                        "sgd_apply"), tag
        if not parts[0].startswith("gemm_"):
            roles["other"][tag] += n
            continue
        ops = [parts[0][len("gemm_"):]] + parts[1:]
        sh = shapes.split("+")
        real = [o for o in ops if o not in ("softmax", "gather")]
        if len(sh) == 1 and len(real) == 2:
            sh = sh * 2            # `gemm_upd+bwd:KxN`: both halves of one shape
        assert len(sh) == len(real), tag
        assert n % len(real) == 0, tag        # a count is the number of GEMMs: a pair tag counts 2 per launch
        n //= len(real)
        for o, s in zip(real, sh):
            roles["fwd" if o == "fwd" else "bwd" if o == "bwd" else "upd"][s] += n
            assert o in ("fwd", "bwd", "upd", "grad"), tag
    return roles


def _check_table(case, tags, steps):
    nl = cases.n_layers(case)
    shapes = [f"{case.dims[l]}x{case.dims[l + 1]}" for l in range(nl)]
    assert len(set(shapes)) == nl or case.dims == tuple(cases.PAIR_WIDE)
    f = sc.parse_factors(case.factors) or [1.0] * nl
    stopper = next(i for i, x in enumerate(f) if x > 0)
    roles = _layer_roles(tags)
    for l, s in enumerate(shapes):
        same = shapes.count(s)
        assert roles["fwd"][s] == steps * same, (case.name, "forward", s)
        trained = sum(1 for j in range(nl) if shapes[j] == s and case.train and f[j] > 0)
        assert roles["upd"][s] == steps * trained, (case.name, "update", s)
        bwd = sum(1 for j in range(nl) if shapes[j] == s and case.train and j > stopper)
        assert roles["bwd"][s] == steps * bwd, (case.name, "backward", s)
    assert set(roles["fwd"]) | set(roles["bwd"]) | set(roles["upd"]) <= set(shapes)
    top = case.dims[-1]
    fused = any(t.startswith("gemm_fwd+softmax:") for t in tags)
    assert fused != (f"softmax_xent:{top}" in tags)
    applies = {f"sgd_apply:{x}" for x in shapes} | {"sgd_apply:2layers"}
    assert set(roles["other"]) <= {f"softmax_xent:{top}", f"colsum:{top}", f"bias_update:{top}", "gather"} | applies
    assert case.runner.startswith("dp") or not set(roles["other"]) & applies
    if f"colsum:{top}" in tags:
        assert not fused and case.train and f[-1] > 0


@pytest.mark.parametrize("name", NAMES)
def test_tag_table_is_well_formed(name):
    """every linear layer has exactly one forward tag per step, every trained layer exactly one update (alone or
    inside a pair tag), no backward tag at or below the stopper, the objective either fused or on its own"""
    case = cases.ALL_CASES[name]
    _check_table(case, case.tags, len(case.rows) if case.runner.endswith("trainer") else 1)
    if case.runner == "trainer":
        def gathers(tags):
            return sum(n // max(1, t.partition(":")[0].count("+")) for t, n in tags.items() if "gather" in t)
        assert gathers(case.tags) == len(case.rows) == gathers(cases.TRAINER_NO_TAIL[name])


@pytest.mark.parametrize("env", list(cases.SETTINGS))
def test_setting_tables_are_well_formed(env):
    s = cases.SETTINGS[env]
    assert set(s.bit_equal_default) <= set(s.cases)
    assert set(s.cases) <= set(cases.SETTINGS[""].cases)      # the default child runs every case a setting runs
    assert set(s.tags) <= set(s.cases) <= set(cases.ALL_CASES) | set(cases.NOT_MLP)
    for name in s.cases:
        if name in cases.NOT_MLP:
            continue
        case = cases.ALL_CASES[name]
        _check_table(case, cases.setting_tags(env, name), len(case.rows) if case.runner.endswith("trainer") else 1)
    assert env == "" or (env.startswith("TNET_") and env.count("=") == 1)
    # bit-equality with the default child is asserted only beside the sentence that claims it, or for tag-identical
    # stream / event / gather settings whose comment says why
    if s.bit_equal_default and env.startswith(("TNET_GEMM_", "TNET_PAIR_")):
        assert len(s.note) > 40, env


def test_parse_report():
    text = "gemm_fwd:23x48 2 0.01 100\ntranspose:48x40 1 0.1 3\ncolsum:300 1 0.2 4\n@runs:1 3 0.2 9\n"
    assert cases.parse_report(text) == {"gemm_fwd:23x48": 2, "colsum:300": 1}
