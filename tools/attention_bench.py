"""Propagation attention, dense-transform route against the compacted route (params['compact_attention']): one JSON line for a
synthetic QM9 batch at the benchmark size (~100k nodes, hidden 100, the reference's default layers, use_propagation_attention).

Two models in one process on the same resident batch -- key off and key on -- measured in `--rounds` interleaved rounds, so both
arms see the same clocks and the same neighbours; per arm the median and min .. max over the rounds of the device-event time.
Three legs (all by default, `--leg kernel|forward|step` for one):
  kernel    the attention-weighted segment sum alone: ggnn_gather_segment_sum_attn_f32 on the dense [V, T*D] rows against
            ggnn_gather_segment_sum_attn_compact_f32 on the compact [R, D] rows, `--iters` launches per round.  For the new kernel
            also the algorithmic HBM bytes, computed from shapes -- per message one h row and one Hc row, per node one h row read
            and one out row written, the indices (row_ptr, slot_pair, slot_row), the in-degree table -- and the fraction of the
            8 TB/s roof they reach.  Both outputs are compared first (max |difference|).
  forward   the inference forward (compute_final_node_representations under no_grad), `--fwd-iters` forwards per round
  step      one training step (train_batch; edge-weight dropout 0.8 as the reference trains), `--step-iters` steps per round
An arm counts as faster only if its whole min .. max range lies below the other arm's.
Run from the repository root:  python tools/attention_bench.py [--graphs 5600] [--rounds 9] [--out profiles/attention_route.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ggnn_amd  # noqa: E402

HBM_ROOF = 8.0e12
ARMS = ("dense", "compact")                                 # key off, key on


def _round(fn, iters):
    """Device-event ms per call of `iters` back-to-back calls."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def _interleaved(fns, iters, rounds, unit=1.0):
    """fns: {arm: callable}.  -> {arm: {median, min, max, rounds}} (times * unit), plus the verdict and the ratio of medians."""
    for fn in fns.values():                                 # warm-up: code objects, workspaces, the caching allocator, weight images
        _round(fn, 5)
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            times[n].append(_round(fn, iters) * unit)
    out = {n: {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4),
               "rounds": [round(x, 4) for x in t]} for n, t in times.items()}
    out["compact_faster"] = bool(out["compact"]["max"] < out["dense"]["min"])
    out["dense_faster"] = bool(out["dense"]["max"] < out["compact"]["min"])
    out["speedup_median"] = round(out["dense"]["median"] / out["compact"]["median"], 3)
    return out


def _models(a):
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0)
    cfg = {"hidden_size": a.hidden, "use_propagation_attention": True, "batch_size": 100000, "random_seed": 0}
    arms = {}
    for name in ARMS:
        extra = {"compact_attention": True} if name == "compact" else {}
        model = ggnn_amd.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms,
                                              "--config": dict(cfg, **extra)})
        assert model.attention_route() == (name == "compact"), name
        arms[name] = model
    return arms


def kernel_leg(a, arms):
    ops = ggnn_amd.ops
    model = arms["compact"]
    feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
    index, nin = feed["message_index"], feed["num_incoming_edges_per_type"]
    comp = index._compact
    V, T, M, R = index.num_nodes, index.num_edge_types, index.num_messages, comp.num_rows
    D = model._kw
    gen = torch.Generator(device="cuda").manual_seed(0)
    h = (torch.rand((V, D), device="cuda", generator=gen) * 2 - 1) * (8.0 / D) ** 0.5       # |h|^2 ~ 2.7: scores of a few units
    W = model.gnn_weights.edge_weights[0].contiguous()
    f = torch.tensor([1.0, 0.7, -0.5, 1.3][:T] + [1.0] * max(T - 4, 0), device="cuda")
    H = ops.msg_transform(h, W)
    Hc = ops.msg_transform_compact(h, W, comp)
    out = {n: torch.empty((V, D), device="cuda") for n in ARMS}
    fns = {"dense": lambda: ops.gather_segment_sum_attn(H, h, index, f, nin, None, True, out=out["dense"]),
           "compact": lambda: ops.gather_segment_sum_attn_compact(Hc, h, index, comp, f, nin, None, True, out=out["compact"])}
    for fn in fns.values():
        fn()
    diff = float((out["dense"] - out["compact"]).abs().max())
    res = _interleaved(fns, a.iters, a.rounds, unit=1e3)                                     # us
    b = M * 2 * D * 4 + V * 2 * D * 4 + (V + 1) * 4 + 2 * M * 4 + V * T * 4 + T * 4
    res.update({"unit": "us per launch", "V": V, "M": M, "R": R, "T": T, "D": D, "launches_per_round": a.iters,
                "max_abs_difference_of_outputs": diff, "max_abs_output": float(out["dense"].abs().max()),
                "compact_bytes_derived": int(b), "compact_roof_fraction": round(b / HBM_ROOF / (res["compact"]["median"] * 1e-6), 3),
                "dense_rows_transformed": V * T, "compact_rows_transformed": R})
    return res


def forward_leg(a, arms):
    feeds = {n: next(iter(m.make_minibatch_iterator(m.valid_data, is_training=False))) for n, m in arms.items()}
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
        res = _interleaved(fns, a.fwd_iters, a.rounds)
    V = feeds["dense"]["initial_node_representation"].shape[0]
    res.update({"unit": "ms per forward", "V": int(V), "timesteps": int(sum(arms["dense"].params["layer_timesteps"])),
                "forwards_per_round": a.fwd_iters, "max_abs_difference_of_final_states": diff})
    return res


def step_leg(a, arms):
    feeds = {}
    for n, m in arms.items():
        np.random.seed(0)
        feeds[n] = dict(next(iter(m.make_minibatch_iterator(m.train_data, is_training=True))), out_layer_dropout_keep_prob=1.0)
    fns = {n: (lambda n=n: arms[n].train_batch(feeds[n])) for n in ARMS}
    res = _interleaved(fns, a.step_iters, a.rounds)
    res.update({"unit": "ms per training step", "V": int(feeds["dense"]["initial_node_representation"].shape[0]),
                "steps_per_round": a.step_iters, "edge_weight_dropout_keep_prob": feeds["dense"]["edge_weight_dropout_keep_prob"]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=5600)
    ap.add_argument("--hidden", type=int, default=100)
    ap.add_argument("--leg", choices=("all", "kernel", "forward", "step"), default="all")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--fwd-iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "attention_bench needs a GPU"
    arms = _models(a)
    out = {"metric": "sparse GGNN with propagation attention, synthetic QM9: dense-transform route (key off) vs compacted route "
                     "(compact_attention)", "graphs": a.graphs, "hidden_size": a.hidden, "rounds": a.rounds,
           "layer_timesteps": arms["dense"].params["layer_timesteps"]}
    legs = {"kernel": kernel_leg, "forward": forward_leg, "step": step_leg}
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
