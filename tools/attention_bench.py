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
  step      one training step (train_batch; edge-weight dropout 0.8 as the reference trains), `--step-iters` steps per round.  A
            third arm, `native`, is the key-on model with compact_attention = 'native' (train_native.ROUTES, entry `attention`: two C
            calls for the propagation instead of the autograd loop); its yardstick is the `compact` arm of the same run.  Per arm
            also `host`: the wall-clock ms per step until the `--step-iters` train_batch calls have RETURNED (before the device is
            waited for) -- the launching thread's share of the step; where it is below the device-event time the step is bound by
            the GPU, where it equals it by the host.
  source    (`--leg source`, part of `all`) the source side of the attention backward alone: the two
            ggnn_weighted_segment_sum_f32 launches of variants._hip_backward against the one ggnn_attn_bwd_source_compact_f32
            launch of the native step, on the same resident batch; outputs compared bit for bit first.
An arm counts as faster only if its whole min .. max range lies below the other arm's.
Run from the repository root:  python tools/attention_bench.py [--graphs 5600] [--rounds 9] [--out profiles/attention_route.json]
(the native step's numbers: --leg step / --leg source, written to profiles/attention_native.json)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ggnn_amd  # noqa: E402

HBM_ROOF = 8.0e12
ARMS = ("dense", "compact")                                 # key off, key on


def _round(fn, iters):
    """(device-event ms, host ms until the calls returned) per call of `iters` back-to-back calls."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters, host / iters


def _stats(t):
    return {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4), "rounds": [round(x, 4) for x in t]}


def _interleaved(fns, iters, rounds, unit=1.0, pairs=(("dense", "compact"),), host=False):
    """fns: {arm: callable}.  -> {arm: {median, min, max, rounds}} (times * unit), plus per (old, new) pair of arms the verdict
    `<new>_faster` / `<old>_faster` and the ratio of medians (`speedup_median` for the first pair, `speedup_median_<new>` after)."""
    for fn in fns.values():                                 # warm-up: code objects, workspaces, the caching allocator, weight images
        _round(fn, 5)
    times = {n: [] for n in fns}
    hosts = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            dev, hst = _round(fn, iters)
            times[n].append(dev * unit)
            hosts[n].append(hst * unit)
    out = {n: _stats(t) for n, t in times.items()}
    if host:
        for n, t in hosts.items():
            out[n]["host"] = _stats(t)
    for i, (old, new) in enumerate(pairs):
        out[new + "_faster"] = bool(out[new]["max"] < out[old]["min"])
        if i == 0 or old + "_faster" not in out:
            out[old + "_faster"] = bool(out[old]["max"] < out[new]["min"])
        else:
            out["%s_faster_than_%s" % (old, new)] = bool(out[old]["max"] < out[new]["min"])
        out["speedup_median" if i == 0 else "speedup_median_" + new] = round(out[old]["median"] / out[new]["median"], 3)
    return out


def _models(a):
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0)
    cfg = {"hidden_size": a.hidden, "use_propagation_attention": True, "batch_size": 100000, "random_seed": 0}
    arms = {}
    for name in ARMS + ("native",):
        extra = {"dense": {}, "compact": {"compact_attention": True}, "native": {"compact_attention": "native"}}[name]
        model = ggnn_amd.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms,
                                              "--config": dict(cfg, **extra)})
        assert model.attention_route() == (name != "dense"), name
        assert ggnn_amd.train_native.attn_model_eligible(model) == (name == "native"), name
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
    assert ggnn_amd.train_native.attn_eligible(arms["native"], feeds["native"])
    fns = {n: (lambda n=n: arms[n].train_batch(feeds[n])) for n in arms}
    res = _interleaved(fns, a.step_iters, a.rounds, pairs=(("dense", "compact"), ("compact", "native")), host=True)
    res.update({"unit": "ms per training step", "V": int(feeds["dense"]["initial_node_representation"].shape[0]),
                "steps_per_round": a.step_iters, "edge_weight_dropout_keep_prob": feeds["dense"]["edge_weight_dropout_keep_prob"]})
    return res


def source_leg(a, arms):
    ops = ggnn_amd.ops
    model = arms["compact"]
    feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
    index = feed["message_index"]
    comp = index._compact
    bwd = ops.compact_backward(index, comp)
    slot_row = ops.source_slot_rows(index, comp)
    V, T, M, R = index.num_nodes, index.num_edge_types, index.num_messages, comp.num_rows
    D = model._kw
    gen = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: torch.rand(shape, device="cuda", generator=gen) * 2 - 1
    dinc, h, dh0 = rnd(V, D), rnd(V, D), rnd(V, D)
    coef_a, coef_s = rnd(M).abs(), rnd(M)
    sni, ri = bwd.source_node_index, bwd.rows_index
    dh = {n: dh0.clone() for n in ("two_launches", "fused")}
    dHc = {n: torch.empty((R, D), device="cuda") for n in dh}

    def two_launches():
        ops.weighted_segment_sum(dinc, ri, ri.msg, coef_a, out=dHc["two_launches"])
        ops.weighted_segment_sum(h, sni, sni.msg, coef_s, out=dh["two_launches"], accumulate=True)

    def fused():
        ops.attn_backward_source_compact(dinc, h, sni, slot_row, R, coef_a, coef_s, dh["fused"], out=dHc["fused"])
    two_launches(); fused()
    same = bool(torch.equal(dHc["two_launches"], dHc["fused"]) and torch.equal(dh["two_launches"], dh["fused"]))
    res = _interleaved({"two_launches": two_launches, "fused": fused}, a.iters, a.rounds, unit=1e3, pairs=(("two_launches", "fused"),))
    # algorithmic bytes of the fused pass: per message two rows read and four indices / coefficients, per node one dh row read and
    # written and one row pointer, per compact row one dHc row written
    b = M * 2 * D * 4 + M * 5 * 4 + V * 2 * D * 4 + (V + 1) * 4 + R * D * 4
    res.update({"unit": "us per source-side pass", "V": V, "M": M, "R": R, "T": T, "D": D, "passes_per_round": a.iters,
                "outputs_bit_identical": same, "fused_bytes_derived": int(b),
                "fused_roof_fraction": round(b / HBM_ROOF / (res["fused"]["median"] * 1e-6), 3)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=5600)
    ap.add_argument("--hidden", type=int, default=100)
    ap.add_argument("--leg", choices=("all", "kernel", "forward", "step", "source"), default="all")
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
    legs = {"kernel": kernel_leg, "forward": forward_leg, "step": step_leg, "source": source_leg}
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
