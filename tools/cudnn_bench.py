"""The sparse GGNN with the CudnnCompatibleGRUCell (graph_rnn_cell = CudnnCompatibleGRUCell), dense-transform route against the
compacted route (params['compact_cudnn_gru']): one JSON line for a synthetic QM9 batch at the benchmark size (~100k nodes), the
default layer plan (timesteps [2, 2, 1, 2, 1], residual layers with nx = 2 and 3), per hidden size of `--hidden`.

Two models in one process on the same resident batch -- key off and key on -- measured in `--rounds` interleaved rounds, so both
arms see the same clocks and the same neighbours; per arm the median and min .. max over the rounds of the device-event time.
Three legs (all by default, `--leg cell,step` for some):
  cell      the node update alone on the same inputs, per nx = 1, 2, 3: the three GEMM launches of ggnn_cudnn_gru_f32 (`dense` arm;
            r, u, hc through HBM, raw weights staged per call) against the one ggnn_cudnn_gru_packed_f32 launch (`compact` arm),
            `--iters` updates per round.  h', r, u, c, hc are compared by their largest difference first (training forms of both).
            For the fused launch also the algorithmic HBM bytes, computed from shapes -- nx + 1 operand rows read and one h' row
            written per node, the 3 (nx + 1) weight images once -- and the matrix flops 2 V (3 nx + 3) D^2 (six bf16 products per exact
            product), against the 8 TB/s and the bf16 matrix roof.
  forward   the inference forward (compute_final_node_representations under no_grad), `--fwd-iters` forwards per round
  step      one training step (train_batch; edge-weight dropout as the reference trains), `--step-iters` steps per round; per arm
            also `host`: the wall-clock ms per step until the train_batch calls have RETURNED (the launching thread's share).
An arm counts as faster only if its whole min .. max range lies below the other arm's.
Run from the repository root:  python tools/cudnn_bench.py [--hidden 100,32,64] [--graphs 5600] [--rounds 9] [--out profiles/cudnn_route.json]
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
ARMS = ("dense", "compact")                                 # key off, key on
CELL = {"graph_rnn_cell": "CudnnCompatibleGRUCell"}


def _models(a, hidden):
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0)
    cfg = dict(CELL, hidden_size=hidden, batch_size=100000, random_seed=0)
    arms = {}
    for name in ARMS:
        model = ggnn_amd.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms,
                                              "--config": dict(cfg, **({"compact_cudnn_gru": True} if name == "compact" else {}))})
        assert model.cudnn_route() == (name == "compact"), name
        arms[name] = model
    return arms


def cell_leg(a, arms):
    ops = ggnn_amd.ops
    model = arms["compact"]
    feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
    V, D = feed["initial_node_representation"].shape[0], model._kw
    gen = torch.Generator(device="cuda").manual_seed(0)

    def u(*shape, s=1.0):
        return ((torch.rand(shape, device="cuda", generator=gen) * 2 - 1) * s).contiguous()
    out = {"unit": "us per node update (dense arm: the three launches of ggnn_cudnn_gru_f32; compact arm: the one fused launch)",
           "V": int(V), "D": int(D), "updates_per_round": a.iters, "per_nx": {}}
    for nx in (1, 2, 3):
        assert ops.cudnn_gru_fused_supported(D, nx), "the cell leg needs a width with the fused cell"
        K = (nx + 1) * D
        xs, h = [u(V, D) for _ in range(nx)], u(V, D)
        Wg, bg = u(K, 2 * D, s=2.0 / K ** 0.5), u(2 * D, s=0.3)
        Wcx, bcx = u(nx * D, D, s=2.0 / (nx * D) ** 0.5), u(D, s=0.3)
        Wch, bch = u(D, D, s=2.0 / D ** 0.5), u(D, s=0.3)
        packed = ops.cudnn_gru_pack(Wg, Wcx, Wch, nx)
        composed = ops.cudnn_gru_train(xs, h, Wg, bg, Wcx, bcx, Wch, bch)
        save = {}
        fused = (ops.cudnn_gru_packed(xs, h, packed, bg, bcx, bch, save=save), save["r"], save["u"], save["c"], save["hc"])
        diffs = {n: {"max_abs_difference": float((c - f).abs().max()), "max_abs": float(c.abs().max())}
                 for n, c, f in zip(("h_out", "r", "u", "c", "hc"), composed, fused)}
        res = _interleaved({"dense": lambda: ops.cudnn_gru(xs, h, Wg, bg, Wcx, bcx, Wch, bch),
                            "compact": lambda: ops.cudnn_gru_packed(xs, h, packed, bg, bcx, bch)}, a.iters, a.rounds, unit=1e3)   # us
        bts = (nx + 2) * V * D * 4 + packed.numel() * 4
        flops = 2 * V * (3 * nx + 3) * D * D
        t = res["compact"]["median"] * 1e-6
        res.update({"comparison": diffs, "fused_bytes_derived": int(bts), "fused_hbm_roof_fraction": round(bts / HBM_ROOF / t, 3),
                    "fused_flops_derived": int(flops), "fused_bf16_products_per_product": 6,
                    "fused_matrix_roof_fraction": round(6 * flops / MATRIX_ROOF_BF16 / t, 3)})
        out["per_nx"][str(nx)] = res
        del xs, h, composed, fused, save
    out["compact_faster"] = all(r["compact_faster"] for r in out["per_nx"].values())
    return out


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
    ap.add_argument("--hidden", default="100", help="one hidden size or a comma-separated list (32, 64, 100 and what pads to them)")
    ap.add_argument("--leg", default="all", help="all, or a comma-separated list of cell, forward, step")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--fwd-iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cudnn_bench needs a GPU"
    legs = {"cell": cell_leg, "forward": forward_leg, "step": step_leg}
    chosen = list(legs) if a.leg == "all" else a.leg.split(",")
    assert all(n in legs for n in chosen), "unknown leg in %r" % a.leg
    out = {"metric": "sparse GGNN with the CudnnCompatibleGRUCell, synthetic QM9: dense-transform route (key off) vs compacted route "
                     "(compact_cudnn_gru)", "graphs": a.graphs, "rounds": a.rounds,
           "arms": {"dense": "key off", "compact": "compact_cudnn_gru True"}, "widths": {}}
    for hidden in [int(w) for w in str(a.hidden).split(",")]:
        arms = _models(a, hidden)
        p = arms["dense"].params
        w = out["widths"][str(hidden)] = {"hidden_size": hidden, "layer_timesteps": p["layer_timesteps"],
                                          "residual_connections": p["residual_connections"]}
        for name, leg in legs.items():
            if name in chosen:
                w[name] = leg(a, arms)
        del arms
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
