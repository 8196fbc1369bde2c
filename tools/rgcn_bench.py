"""R-GCN through the sparse GGNN (graph_rnn_cell = RNN, the reference README's fourth command), dense-transform route against the
compacted route (params['compact_rnn']): one JSON line for a synthetic QM9 batch at the benchmark size (~100k nodes, hidden 100,
eight layers of one timestep, ReLU, mean aggregation, no edge bias).

Two models in one process on the same resident batch -- key off and key on -- measured in `--rounds` interleaved rounds, so both
arms see the same clocks and the same neighbours; per arm the median and min .. max over the rounds of the device-event time.
Four legs (all by default, `--leg cell,step` for some):
  cell      the node update alone on the same inputs: ggnn_gather_segment_sum_f32 over the compact rows + ggnn_rnn_f32 (two
            launches, `incoming` through HBM, raw weights staged per call) against the one ggnn_rnn_packed_gather_f32 launch,
            `--iters` updates per round.  `incoming` is compared bit for bit first, h' by its largest difference.  For the fused
            launch also the algorithmic HBM bytes, computed from shapes -- per message one Hc row, per node one h row read and one
            h' row written, the indices (row_ptr, gather_row) and the in-degree table -- and the fraction of the 8 TB/s roof.
  forward   the inference forward (compute_final_node_representations under no_grad), `--fwd-iters` forwards per round
  step      one training step (train_batch; edge-weight dropout as the reference trains), `--step-iters` steps per round; per arm
            also `host`: the wall-clock ms per step until the train_batch calls have RETURNED (the launching thread's share).
            A third arm, `native`: the key 'native' (train_native.ROUTES, entry `rnn`: two native calls, no torch.autograd),
            judged against the `compact` arm (the key True).
  cell-bwd  the cell's backward alone on the same inputs: ggnn_act_bwd_f32 + ggnn_bwd_dx_f32 (`launches`) against the one
            ggnn_rnn_bwd_fused_f32 launch (`fused`), and with a deferred node sum ggnn_gather_segment_sum_heads_f32 in front of
            the two (`launches_sum`) against ggnn_rnn_bwd_fused_gather_f32 (`fused_gather`); dP is compared bit for bit first, the
            products by their largest difference.  For the fused launches also the algorithmic HBM bytes, computed from shapes
            -- g and out read, dP, d_incoming and dh written, the in-degree table; with the sum one Z row per compact row and
            a head record per node -- and the fraction of the 8 TB/s roof.
An arm counts as faster only if its whole min .. max range lies below the other arm's.
Run from the repository root:  python tools/rgcn_bench.py [--graphs 5600] [--rounds 9] [--out profiles/rgcn_route.json]

--hidden 128 / 192 / 256 (one or a comma-separated list): the PANEL comparison instead.  Per width two models on the compacted
route in the same process -- `compact` (compact_rnn True alone: segment sum over the compact rows + ggnn_rnn_f32) and `panel` (plus
rnn_panel_cell: the one ggnn_rnn_panel_gather_f32 launch) -- through the cell, forward and step legs above, `panel` judged against
`compact`.  The cell leg adds the panel launch's algorithmic HBM bytes and matrix flops (2 V (nx+1) D^2; six bf16 products per
exact product) against both roofs.      python tools/rgcn_bench.py --hidden 128,192,256 --out profiles/rgcn_panel.json
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

MATRIX_ROOF_BF16 = 2.5e15                                   # flop/s of v_mfma_f32_16x16x32_bf16 on the whole chip (tools/dense_bench.py)
PANEL_ARMS = ("compact", "panel")                           # compact_rnn True alone, plus rnn_panel_cell

ARMS = ("dense", "compact")                                 # key off, key on
NATIVE = "native"                                           # key 'native': the step leg's third arm
README = {"use_edge_bias": False, "use_edge_msg_avg_aggregation": True, "residual_connections": {},
          "layer_timesteps": [1, 1, 1, 1, 1, 1, 1, 1], "graph_rnn_cell": "RNN", "graph_rnn_activation": "ReLU"}


def _models(a):
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0)
    cfg = dict(README, hidden_size=a.hidden, batch_size=100000, random_seed=0)
    arms = {}
    for name in ARMS + (NATIVE,):
        extra = {"dense": {}, "compact": {"compact_rnn": True}, NATIVE: {"compact_rnn": "native"}}[name]
        model = ggnn_amd.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms,
                                              "--config": dict(cfg, **extra)})
        assert model.rnn_route() == (name != "dense"), name
        assert ggnn_amd.train_native.rnn_model_eligible(model) == (name == NATIVE), name
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


def _panel_models(a, hidden):
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0)
    cfg = dict(README, hidden_size=hidden, batch_size=100000, random_seed=0, compact_rnn=True)
    arms = {}
    for name in PANEL_ARMS:
        model = ggnn_amd.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms,
                                              "--config": dict(cfg, **({"rnn_panel_cell": True} if name == "panel" else {}))})
        assert model.rnn_route() and model.rnn_panel_route() == (name == "panel"), name
        arms[name] = model
    return arms


def panel_cell_leg(a, arms):
    ops = ggnn_amd.ops
    model = arms["panel"]
    feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
    index, nin = feed["message_index"], feed["num_incoming_edges_per_type"]
    comp = index._compact
    V, T, M, R = index.num_nodes, index.num_edge_types, index.num_messages, comp.num_rows
    D = model._kw
    assert ops.rnn_panel_supported(D, 1), "the panel cell leg needs a width with the panel cell at nx = 1"
    gen = torch.Generator(device="cuda").manual_seed(0)
    h = torch.rand((V, D), device="cuda", generator=gen) * 2 - 1
    cell = model.gnn_weights.rnn_cells[0]
    W, b = cell.kernel.detach().contiguous(), cell.bias.detach().contiguous()
    Hc = ops.msg_transform_compact(h, model.gnn_weights.edge_weights[0].detach().view(T, D, D).contiguous(), comp)
    packed = ops.rnn_panel_pack(W, 1)
    act = model.params["graph_rnn_activation"]
    results = {}

    def composed():
        inc = ops.gather_segment_sum_compact(Hc, index, comp, nin, None, True)
        results["compact"] = (ops.rnn([inc], h, W, b, act), inc)

    def panel():
        save = {}
        results["panel"] = (ops.rnn_panel_gather([], h, packed, b, Hc, index, comp.gather_row, nin, act, save=save), save["incoming"])

    def panel_inference():
        ops.rnn_panel_gather([], h, packed, b, Hc, index, comp.gather_row, nin, act)
    composed(); panel()
    same_incoming = bool(torch.equal(results["compact"][1], results["panel"][1]))
    diff = float((results["compact"][0] - results["panel"][0]).abs().max())
    res = _interleaved({"compact": composed, "panel": panel_inference}, a.iters, a.rounds, unit=1e3, pairs=(PANEL_ARMS,))   # us
    bts = M * D * 4 + V * 2 * D * 4 + (V + 1) * 4 + M * 4 + V * T * 4
    flops = 2 * V * 2 * D * D
    t = res["panel"]["median"] * 1e-6
    res.update({"unit": "us per node update (compact arm: segment sum over the compact rows + ggnn_rnn_f32; panel arm: the one launch)",
                "V": V, "M": M, "R": R, "T": T, "D": D, "updates_per_round": a.iters, "incoming_bit_identical": same_incoming,
                "max_abs_difference_of_outputs": diff, "max_abs_output": float(results["compact"][0].abs().max()),
                "panel_bytes_derived": int(bts), "panel_hbm_roof_fraction": round(bts / HBM_ROOF / t, 3),
                "panel_flops_derived": int(flops), "panel_bf16_products_per_product": 6,
                "panel_matrix_roof_fraction": round(6 * flops / MATRIX_ROOF_BF16 / t, 3)})
    return res


def panel_forward_leg(a, arms):
    feeds = {n: next(iter(arms[n].make_minibatch_iterator(arms[n].valid_data, is_training=False))) for n in PANEL_ARMS}
    finals = {}

    def make(n):
        model = arms[n]

        def run():
            model.feed(feeds[n])
            finals[n] = model.compute_final_node_representations()
        return run
    with torch.no_grad():
        fns = {n: make(n) for n in PANEL_ARMS}
        for fn in fns.values():
            fn()
        diff = float((finals["compact"] - finals["panel"]).abs().max())
        scale = float(finals["compact"].abs().max())
        res = _interleaved(fns, a.fwd_iters, a.rounds, pairs=(PANEL_ARMS,))
    V = feeds["compact"]["initial_node_representation"].shape[0]
    res.update({"unit": "ms per forward", "V": int(V), "timesteps": int(sum(arms["compact"].params["layer_timesteps"])),
                "forwards_per_round": a.fwd_iters, "max_abs_difference_of_final_states": diff, "max_abs_final_state": scale})
    return res


def panel_step_leg(a, arms):
    feeds = {}
    for n, m in arms.items():
        np.random.seed(0)
        feeds[n] = dict(next(iter(m.make_minibatch_iterator(m.train_data, is_training=True))), out_layer_dropout_keep_prob=1.0)
    fns = {n: (lambda n=n: arms[n].train_batch(feeds[n])) for n in arms}
    res = _interleaved(fns, a.step_iters, a.rounds, pairs=(PANEL_ARMS,), host=True)
    res.update({"unit": "ms per training step", "V": int(feeds["compact"]["initial_node_representation"].shape[0]),
                "steps_per_round": a.step_iters, "edge_weight_dropout_keep_prob": feeds["compact"]["edge_weight_dropout_keep_prob"]})
    return res


def panel_main(a, widths):
    out = {"metric": "sparse GGNN with the BasicRNNCell (R-GCN configuration), synthetic QM9, compacted route: composed cell "
                     "(compact_rnn alone) vs the column-panel cell (plus rnn_panel_cell)", "graphs": a.graphs, "rounds": a.rounds,
           "arms": {"compact": "compact_rnn True", "panel": "compact_rnn True, rnn_panel_cell True"}, "widths": {}}
    legs = {"cell": panel_cell_leg, "forward": panel_forward_leg, "step": panel_step_leg}
    chosen = list(legs) if a.leg == "all" else a.leg.split(",")
    assert all(n in legs for n in chosen), "the panel comparison has the legs cell, forward, step (got %r)" % a.leg
    for hidden in widths:
        arms = _panel_models(a, hidden)
        w = out["widths"][str(hidden)] = {"hidden_size": hidden, "layer_timesteps": arms["compact"].params["layer_timesteps"],
                                          "graph_rnn_activation": arms["compact"].params["graph_rnn_activation"]}
        for name, leg in legs.items():
            if name in chosen:
                w[name] = leg(a, arms)
        w["panel_faster_on_every_leg"] = all(w[n]["panel_faster"] for n in chosen)
        del arms
        torch.cuda.empty_cache()
    return out


def cell_bwd_leg(a, arms):
    ops = ggnn_amd.ops
    model = arms["compact"]
    feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
    index, nin = feed["message_index"], feed["num_incoming_edges_per_type"]
    comp = index._compact
    if getattr(comp, "_bwd", None) is None:
        ops.prepare_message_index(index, model._kw, True, training=True)
        comp = index._compact
    bwd = ops.compact_backward(index, comp)
    V, T, R = index.num_nodes, index.num_edge_types, comp.num_rows
    D = model._kw
    assert ops.rnn_bwd_fused_supported(D, 1), "the cell-bwd leg needs a width with the fused backward at nx = 1"
    gen = torch.Generator(device="cuda").manual_seed(0)
    g = torch.randn((V, D), device="cuda", generator=gen)
    out = torch.relu(torch.rand((V, D), device="cuda", generator=gen) * 2 - 1)          # a ReLU output: about half the entries 0
    Z = torch.randn((R, D), device="cuda", generator=gen)
    W = model.gnn_weights.rnn_cells[0].kernel.detach().contiguous()
    WT = ggnn_amd.backward.transposed(W)
    packed = ops.rnn_bwd_pack(W, 1)
    act = model.params["graph_rnn_activation"]
    ni = bwd.node_index
    heads = ops.slot_heads(ni, ni.row_ptr, ni.gather_row, V)
    lib = ggnn_amd._lib.load()
    results = {}
    dx = torch.empty((V, D), device="cuda"); dinc = torch.empty_like(g); dh = torch.empty_like(g); gs = torch.empty_like(g)

    def launches(grad=g, key="launches"):
        dP = ops.act_bwd(grad, out, act)
        ops.bwd_dx(dP, 1, WT, D, True, dx, dinc, nin, True, dh, False, False, D)
        results[key] = (dP, dinc, dh)

    def launches_sum():                                     # (the sum accumulates in place, as in the step: gs keeps growing while timed)
        ggnn_amd._lib.check(lib.ggnn_gather_segment_sum_heads_f32(Z.data_ptr(), ni.row_ptr.data_ptr(), ni.gather_row.data_ptr(), heads.data_ptr(),
                                                                  None, None, 0, gs.data_ptr(), V, D, 1, 1, torch.cuda.current_stream().cuda_stream))
        launches(gs, "launches_sum")

    def fused():
        dP, dh_f, dxs = ops.rnn_bwd_fused(g, out, packed, nin, True, 1, act)
        results["fused"] = (dP, dxs[0], dh_f)

    def fused_gather():
        dP, dh_f, dxs = ops.rnn_bwd_fused(g, out, packed, nin, True, 1, act, gather=(Z, heads))
        results["fused_gather"] = (dP, dxs[0], dh_f)
    cmp = {}
    for old, new in (("launches", "fused"), ("launches_sum", "fused_gather")):
        gs.copy_(g)
        {"launches": launches, "launches_sum": launches_sum}[old](); {"fused": fused, "fused_gather": fused_gather}[new]()
        a_, b_ = [tuple(t.clone() for t in results[k]) for k in (old, new)]
        finite = torch.isfinite(a_[1]).all(dim=1)           # (a node without incoming edges divides by 1e-7: compare the others)
        cmp[new] = {"dP_bit_identical": bool(torch.equal(a_[0], b_[0])),
                    "max_abs_difference_of_dinc": float((a_[1] - b_[1])[finite].abs().max()), "max_abs_dinc": float(a_[1][finite].abs().max()),
                    "max_abs_difference_of_dh": float((a_[2] - b_[2]).abs().max()), "max_abs_dh": float(a_[2].abs().max())}
    res = _interleaved({"launches": launches, "fused": fused, "launches_sum": launches_sum, "fused_gather": fused_gather}, a.iters, a.rounds,
                       unit=1e3, pairs=(("launches", "fused"), ("launches_sum", "fused_gather")))   # us
    bts = 5 * V * D * 4 + V * T * 4
    bts_g = bts + R * D * 4 + V * 16
    res.update({"unit": "us per cell backward (launches: ggnn_act_bwd_f32 + ggnn_bwd_dx_f32; launches_sum: "
                        "ggnn_gather_segment_sum_heads_f32 (accumulating in place) in front of them; fused / fused_gather: the one launch; every arm allocates its outputs)",
                "V": V, "R": R, "T": T, "D": D, "backwards_per_round": a.iters, "comparison": cmp,
                "fused_bytes_derived": int(bts), "fused_roof_fraction": round(bts / HBM_ROOF / (res["fused"]["median"] * 1e-6), 3),
                "fused_gather_bytes_derived": int(bts_g),
                "fused_gather_roof_fraction": round(bts_g / HBM_ROOF / (res["fused_gather"]["median"] * 1e-6), 3)})
    return res


def forward_leg(a, arms):
    arms = {n: arms[n] for n in ARMS}
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
    res = _interleaved(fns, a.step_iters, a.rounds, pairs=(("dense", "compact"), ("compact", NATIVE)), host=True)
    res.update({"unit": "ms per training step", "V": int(feeds["dense"]["initial_node_representation"].shape[0]),
                "steps_per_round": a.step_iters, "edge_weight_dropout_keep_prob": feeds["dense"]["edge_weight_dropout_keep_prob"]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=5600)
    ap.add_argument("--hidden", default="100", help="one hidden size, or 128 / 192 / 256 (a comma-separated list of them): the panel comparison")
    ap.add_argument("--leg", default="all", help="all, or a comma-separated list of cell, cell-bwd, forward, step")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--fwd-iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rgcn_bench needs a GPU"
    widths = [int(w) for w in str(a.hidden).split(",")]
    if all(w in (128, 192, 256) for w in widths):
        line = json.dumps(panel_main(a, widths))
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    assert len(widths) == 1, "several widths at once: the panel comparison only (128, 192, 256)"
    a.hidden = widths[0]
    arms = _models(a)
    out = {"metric": "sparse GGNN with the BasicRNNCell (R-GCN configuration), synthetic QM9: dense-transform route (key off) vs "
                     "compacted route (compact_rnn)", "graphs": a.graphs, "hidden_size": a.hidden, "rounds": a.rounds,
           "step_arms": {"dense": "key off", "compact": "compact_rnn True", NATIVE: "compact_rnn 'native'"},
           "layer_timesteps": arms["dense"].params["layer_timesteps"], "graph_rnn_activation": arms["dense"].params["graph_rnn_activation"]}
    legs = {"cell": cell_leg, "cell-bwd": cell_bwd_leg, "forward": forward_leg, "step": step_leg}
    chosen = list(legs) if a.leg == "all" else a.leg.split(",")
    assert all(n in legs for n in chosen), "unknown leg in %r" % a.leg
    for name, leg in legs.items():
        if name in chosen:
            out[name] = leg(a, arms)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
