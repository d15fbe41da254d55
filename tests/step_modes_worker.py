"""Runs cases of tests/step_cases.py on the GPU.  tests/test_gpu_step_branches.py imports run_case for the default
process, and starts this file as a child process for every TNET_* switch of its matrix (the library reads each switch
once per process): `step_modes_worker.py OUT.npz CASE[,CASE...]` runs the named cases under whatever environment it
was given and writes every step's exposed outputs, parameters and launch-tag counts and the objective's statistics to
OUT.npz."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(os.path.dirname(HERE), "nnet-asr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import stack_cases as sc  # noqa: E402
import step_cases as cases  # noqa: E402
from tnet_amd import Comm, DeviceArray, Network, Objective, RbmTrainer, RnnTrainer, Trainer, synchronize  # noqa: E402
from tnet_amd._lib import check, lib  # noqa: E402


def timing(on):
    """kernel timing per launch over every tag; turning it on also clears what an earlier run left in the report"""
    check(lib().tnet_kernel_timing_filter(b""), "timing_filter")
    check(lib().tnet_kernel_timing(1 if on else 0), "kernel_timing")
    if on:
        report()


def report():
    buf = C.create_string_buffer(1 << 16)
    check(lib().tnet_kernel_timing_report(buf, len(buf)), "kernel_timing_report")
    return cases.parse_report(buf.value.decode())


def _state(net):
    return {key: v for key, v in sc.state(net).items()}


def _network(case):
    """the case's network.  A large case's weights (up to 12 M of them) are not sent through the text format, which
    takes 5 to 7 s to write: the network is read from a text of zeros and the float32 parameters are uploaded
    (the text at 9 digits holds the same float32 values: tests/test_stack_cases_cpu.py)"""
    L = cases.layers(case)
    if not case.large:
        return Network.from_layers(L)
    text = []
    for l in L:
        text.append(f"{l.tag} {l.n_out} {l.n_in}\n")
        if l.W is not None:
            row = "0 " * l.n_in + "\n"
            text.append(f"m {l.n_out} {l.n_in}\n" + row * l.n_out + f"v {l.n_out}  " + "0 " * l.n_out + "\n\n")
    net = Network(text="".join(text))
    for i, l in enumerate(L):
        if l.W is not None:
            net.set_params(i, l.W, l.b)
    return net


def run_case(case, timed=True):
    """{"steps": [(outputs {component: array}, parameters {key: array}, tags {tag: count})], "stats": (sum, frames,
    correct)}.  A Trainer case is one entry: the whole drain's tags and the parameters after it."""
    net = _network(case)
    sc.configure(net, cases.consts(case), case.factors)
    net.keep_output(case.keep)
    obj = Objective()
    steps = []
    comm = Comm(0, 1, Comm.unique_id()) if case.runner.startswith("dp") else None
    timing(timed)
    try:
        if case.runner == "dp":
            net.set_comm(comm)
        if case.runner.endswith("trainer"):
            B = case.rows[0]
            assert all(r == B for r in case.rows)
            tr = Trainer(net, obj, bunchsize=B, cachesize=B * len(case.rows), seed=cases.TRAINER_SEED, randomize=True,
                         crossval=not case.train)
            if comm is not None:
                tr.set_comm(comm)
            # one utterance that fills the cache exactly: the trainer shuffles and drains it at once
            tr.add_utterance(*cases.corpus(case))
            tr.finish()
            assert tr.steps == len(case.rows)
            synchronize()
            steps.append(({}, _state(net), report() if timed else {}))
            del tr
        else:
            for X, lab in cases.data(case):
                net.train_bunch(obj, DeviceArray.from_numpy(X), DeviceArray.vector(lab), train=case.train)
                tags = report() if timed else {}
                outs = {i: net.output(i, len(lab)) for i in cases.exposed_outputs(case)}
                steps.append((outs, _state(net), tags))
    finally:
        timing(False)
        if comm is not None:
            net.set_comm(None)
            synchronize()
            del comm
    return {"steps": steps, "stats": obj.stats()}


def run_rbm(name):
    """one RbmTrainer epoch of step_cases.rbm_corpus(name): the parameters, and (mse, frames, steps) as `stats`"""
    layer, feats, B, cache = cases.rbm_corpus(name)
    net = Network.from_layers([layer])
    tr = RbmTrainer(net, bunchsize=B, cachesize=cache, seed=cases.RBM_SEED, learn_rate=cases.RBM_LR,
                    momentum=cases.RBM_MMT, weightcost=cases.RBM_WC)
    tr.train_corpus(feats)
    mse, frames = tr.stats()
    W, vb, hb, _ = net.rbm_params(0)
    return {"steps": [({}, {"W": W, "vb": vb, "hb": hb}, {})], "stats": (mse, frames, tr.steps)}


def run_rnn(name):
    """one RnnTrainer pass over step_cases.rnn_corpus(name): the parameters and the objective's statistics"""
    layers, feats, labels, bptt = cases.rnn_corpus(name)
    net = Network.from_layers(layers)
    net.set_learn_rate(cases.RNN_LR)
    net.set_momentum(cases.RNN_MMT)
    net.set_weightcost(cases.RNN_WC)
    obj = Objective()
    RnnTrainer(net, obj, bptt=bptt).train_corpus(feats, labels)
    synchronize()
    (Wr, br), (W2, b2) = net.recurrent_params(0), net.linear_params()[0]
    return {"steps": [({}, {"Wr": Wr, "br": br, "W2": W2, "b2": b2}, {})], "stats": obj.stats()}


def pack(results):
    flat = {}
    for name, res in results.items():
        for s, (outs, state, tags) in enumerate(res["steps"]):
            for i, a in outs.items():
                flat[f"{name}|{s}|out|{i}"] = a
            for key, a in state.items():
                flat[f"{name}|{s}|par|{key}"] = a
            flat[f"{name}|{s}|tags"] = np.array(json.dumps(tags))
        flat[f"{name}|stats"] = np.array(res["stats"], np.float64)
    return flat


def unpack(npz):
    results = {}
    for key in npz.files:
        parts = key.split("|")
        res = results.setdefault(parts[0], {"steps": {}, "stats": None})
        if parts[1] == "stats":
            res["stats"] = tuple(float(x) for x in npz[key])
            continue
        step = res["steps"].setdefault(int(parts[1]), ({}, {}, {}))
        if parts[2] == "tags":
            step[2].update(json.loads(str(npz[key])))
        elif parts[2] == "out":
            step[0][int(parts[3])] = npz[key]
        else:
            step[1][parts[3]] = npz[key]
    for res in results.values():
        res["steps"] = [res["steps"][s] for s in sorted(res["steps"])]
    return results


def main(out, names):
    results = {name: run_rbm(name) if name in cases.RBM else run_rnn(name) if name in cases.RNN
               else run_case(cases.ALL_CASES[name]) for name in names.split(",")}
    synchronize()
    np.savez(out, **pack(results))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
