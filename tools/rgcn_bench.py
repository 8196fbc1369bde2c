"""R-GCN through the sparse GGNN (graph_rnn_cell = RNN, the reference README's fourth command), dense-transform route against the
compacted route (params['compact_rnn']): one JSON line for a synthetic QM9 batch at the benchmark size (~100k nodes, hidden 100,
eight layers of one timestep, ReLU, mean aggregation, no edge bias).

Two models in one process on the same resident batch -- key off and key on -- measured in `--rounds` interleaved rounds, so both
arms see the same clocks and the same neighbours; per arm the median and min .. max over the rounds of the device-event time.
Three legs (all by default, `--leg cell|forward|step` for one):
  cell      the node update alone on the same inputs: ggnn_gather_segment_sum_f32 over the compact rows + ggnn_rnn_f32 (two
            launches, `incoming` through HBM, raw weights staged per call) against the one ggnn_rnn_packed_gather_f32 launch,
            `--iters` updates per round.  `incoming` is compared bit for bit first, h' by its largest difference.  For the fused
            launch also the algorithmic HBM bytes, computed from shapes -- per message one Hc row, per node one h row read and one
            h' row written, the indices (row_ptr, gather_row) and the in-degree table -- and the fraction of the 8 TB/s roof.
  forward   the inference forward (compute_final_node_representations under no_grad), `--fwd-iters` forwards per round
  step      one training step (train_batch; edge-weight dropout as the reference trains), `--step-iters` steps per round; per arm
            also `host`: the wall-clock ms per step until the train_batch calls have RETURNED (the launching thread's share).
An arm counts as faster only if its whole min .. max range lies below the other arm's.
Run from the repository root:  python tools/rgcn_bench.py [--graphs 5600] [--rounds 9] [--out profiles/rgcn_route.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ggnn_amd  # noqa: E402
from attention_bench import HBM_ROOF, _interleaved  # noqa: E402

ARMS = ("dense", "compact")                                 # key off, key on
README = {"use_edge_bias": False, "use_edge_msg_avg_aggregation": True, "residual_connections": {},
          "layer_timesteps": [1, 1, 1, 1, 1, 1, 1, 1], "graph_rnn_cell": "RNN", "graph_rnn_activation": "ReLU"}


def _models(a):
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0)
    cfg = dict(README, hidden_size=a.hidden, batch_size=100000, random_seed=0)
    arms = {}
    for name in ARMS:
        model = ggnn_amd.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms,
                                              "--config": dict(cfg, **({"compact_rnn": True} if name == "compact" else {}))})
        assert model.rnn_route() == (name == "compact"), name
        arms[name] = model
    return arms


def cell_leg(a, arms):
    ops = ggnn_amd.ops
    model = arms["compact"]
    feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
    index, nin = feed["message_index"], feed["num_incoming_edges_per_type"]
    comp = index._compact
    V, T, M, R = index.num_nodes, index.num_edge_types, index.num_messages, comp.num_rows
    D = model._kw
    assert ops.rnn_fused_supported(D, 1), "the cell leg needs a width with the fused cell at nx = 1"
    gen = torch.Generator(device="cuda").manual_seed(0)
    h = torch.rand((V, D), device="cuda", generator=gen) * 2 - 1
    cell = model.gnn_weights.rnn_cells[0]
    W, b = cell.kernel.detach().contiguous(), cell.bias.detach().contiguous()
    Hc = ops.msg_transform_compact(h, model.gnn_weights.edge_weights[0].detach().view(T, D, D).contiguous(), comp)
    packed = ops.rnn_pack(W, 1)
    act = model.params["graph_rnn_activation"]
    results = {}

    def composed():
        inc = ops.gather_segment_sum_compact(Hc, index, comp, nin, None, True)
        results["dense"] = (ops.rnn([inc], h, W, b, act), inc)

    def fused():
        save = {}
        results["compact"] = (ops.rnn_packed_gather([], h, packed, b, Hc, index, comp.gather_row, nin, act, save=save), save["incoming"])

    def fused_inference():
        ops.rnn_packed_gather([], h, packed, b, Hc, index, comp.gather_row, nin, act)
    composed(); fused()
    same_incoming = bool(torch.equal(results["dense"][1], results["compact"][1]))
    diff = float((results["dense"][0] - results["compact"][0]).abs().max())
    res = _interleaved({"dense": composed, "compact": fused_inference}, a.iters, a.rounds, unit=1e3)   # us
    bts = M * D * 4 + V * 2 * D * 4 + (V + 1) * 4 + M * 4 + V * T * 4
    res.update({"unit": "us per node update (dense arm: segment sum over the compact rows + ggnn_rnn_f32; compact arm: the fused launch)",
                "V": V, "M": M, "R": R, "T": T, "D": D, "updates_per_round": a.iters, "incoming_bit_identical": same_incoming,
                "max_abs_difference_of_outputs": diff, "max_abs_output": float(results["dense"][0].abs().max()),
                "fused_bytes_derived": int(bts), "fused_roof_fraction": round(bts / HBM_ROOF / (res["compact"]["median"] * 1e-6), 3)})
    return res


def forward_leg(a, arms):
    feeds = {n: next(iter(arms[n].make_minibatch_iterator(arms[n].valid_data, is_training=False))) for n in ARMS}
    finals = {}

    def make(n):
        model = arms[n]

        def run():
            model.feed(feeds[n])
            finals[n] = model.compute_final_node_representations()
        return run
    with torch.no_grad():
        fns = {n: make(n) for n in ARMS}
        for fn in fns.values():
            fn()
        diff = float((finals["dense"] - finals["compact"]).abs().max())
        scale = float(finals["dense"].abs().max())
        res = _interleaved(fns, a.fwd_iters, a.rounds)
    V = feeds["dense"]["initial_node_representation"].shape[0]
    res.update({"unit": "ms per forward", "V": int(V), "timesteps": int(sum(arms["dense"].params["layer_timesteps"])),
                "forwards_per_round": a.fwd_iters, "max_abs_difference_of_final_states": diff, "max_abs_final_state": scale})
    return res


def step_leg(a, arms):
    feeds = {}
    for n, m in arms.items():
        np.random.seed(0)
        feeds[n] = dict(next(iter(m.make_minibatch_iterator(m.train_data, is_training=True))), out_layer_dropout_keep_prob=1.0)
    fns = {n: (lambda n=n: arms[n].train_batch(feeds[n])) for n in arms}
    res = _interleaved(fns, a.step_iters, a.rounds, host=True)
    res.update({"unit": "ms per training step", "V": int(feeds["dense"]["initial_node_representation"].shape[0]),
                "steps_per_round": a.step_iters, "edge_weight_dropout_keep_prob": feeds["dense"]["edge_weight_dropout_keep_prob"]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=5600)
    ap.add_argument("--hidden", type=int, default=100)
    ap.add_argument("--leg", choices=("all", "cell", "forward", "step"), default="all")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--fwd-iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rgcn_bench needs a GPU"
    arms = _models(a)
    out = {"metric": "sparse GGNN with the BasicRNNCell (R-GCN configuration), synthetic QM9: dense-transform route (key off) vs "
                     "compacted route (compact_rnn)", "graphs": a.graphs, "hidden_size": a.hidden, "rounds": a.rounds,
           "layer_timesteps": arms["dense"].params["layer_timesteps"], "graph_rnn_activation": arms["dense"].params["graph_rnn_activation"]}
    legs = {"cell": cell_leg, "forward": forward_leg, "step": step_leg}
    for name, leg in legs.items():
        if a.leg in ("all", name):
            out[name] = leg(a, arms)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
