"""Subprocess worker of tests/test_gpu_rnn.py::test_rnn_strict_parity_mode (TNET_RNN_AHEAD is read once per process):
trains the recurrent network on fixed corpora -- 135 and 4000 outputs, bptt 0 and 4, with momentum and weight cost --
on the fused per-frame chain and on the component-by-component chain (TNET_RNN_GENERIC=1), then one 300-frame
utterance on the fused chain, and writes the inputs, the statistics and every parameter to an .npz.  With
TNET_RNN_AHEAD=0 in the environment the fused chain is the older one (PropagatePartial with the update folded into
the next frame's forward: the arithmetic of the component chain per element, the strict-parity mode); by default it is
the look-ahead chain, which differs from it by fp32 reassociation."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nnet-asr_amd"))
from tnet_amd import Network, Objective, RnnTrainer, formats, synchronize  # noqa: E402

NIN, H, LR, MMT, WC = 40, 64, 0.02, 0.5, 1e-4
CORPORA = [(f"s{S}_b{bptt}", S, bptt, (50, 33)) for S in (135, 4000) for bptt in (0, 4)] + [("long", 135, 4, (300,))]


def train(layers, feats, labels, bptt, generic):
    os.environ["TNET_RNN_GENERIC"] = "1" if generic else "0"
    try:
        net = Network.from_layers(layers)
        net.set_learn_rate(LR)
        net.set_momentum(MMT)
        net.set_weightcost(WC)
        obj = Objective()
        RnnTrainer(net, obj, bptt=bptt).train_corpus(feats, labels)
        synchronize()
        (Wr, br), (W2, b2) = net.recurrent_params(0), net.linear_params()[0]
        return dict(stats=np.array(obj.stats(), np.float64), Wr=Wr, br=br, W2=W2, b2=b2)
    finally:
        os.environ.pop("TNET_RNN_GENERIC", None)


def main(out):
    res = {}
    for name, S, bptt, lens in CORPORA:
        rng = np.random.default_rng(S + bptt + len(lens))
        layers = formats.gen_recurrent_init(NIN, H, S, seed=11)
        feats = [rng.standard_normal((T, NIN)).astype(np.float32) for T in lens]
        labels = [rng.integers(0, S, T).astype(np.int32) for T in lens]
        res.update({f"{name}/in/Wr": layers[0].W, f"{name}/in/br": layers[0].b, f"{name}/in/W2": layers[1].W,
                    f"{name}/in/b2": layers[1].b, f"{name}/in/bptt": np.array(bptt)})
        for u, (f, l) in enumerate(zip(feats, labels)):
            res[f"{name}/in/feat{u}"], res[f"{name}/in/lab{u}"] = f, l
        for chain in ("fused",) + (("generic",) if name != "long" else ()):
            for k, v in train(layers, feats, labels, bptt, chain == "generic").items():
                res[f"{name}/{chain}/{k}"] = v
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
