"""One training step of the sparse model on the config-5 graph (100,000 nodes / 1,000,000 edges / 4 edge types / h = 256 / 8
timesteps) with the column-panel GRU backward on the compacted route, and with ops.gru_bwd_is_fused switched off (the route before
the panel kernel existed: dense-form transform, unfused GRU backward), interleaved in one process.  Prints one JSON line.
   python tools/wide_train_bench.py [--route both|fused|parent] [--rounds 7] [--steps 3] [--out FILE]"""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("gated-graph-neural-network-samples_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--route", default="both", choices=["both", "fused", "parent"])
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
V, M, T, D, G = 100000, 1000000, 4, 256, 1000
adj_np, nin_np = pkg.synthetic_large_graph(V, M, T, seed=5, power_law=False)
raw = [{"targets": [[0.0]], "graph": [[0, t + 1, 1] for t in range(T)], "node_features": [[1, 0, 0, 0, 0]] * 2}]
cfg = {"hidden_size": D, "layer_timesteps": [8], "residual_connections": {}, "tie_fwd_bkwd": True}
model = pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": None, "valid_data": raw, "--config": cfg})
rng = np.random.default_rng(6)
feed = {"initial_node_representation": torch.from_numpy(rng.uniform(-1, 1, (V, D)).astype(np.float32)).to(dev),
        "adjacency_lists": [torch.from_numpy(a).to(dev) for a in adj_np],
        "num_incoming_edges_per_type": torch.from_numpy(nin_np).to(dev),
        "graph_nodes_list": (torch.arange(V, device=dev) // (V // G)).to(torch.int32), "num_graphs": G,
        "graph_ptr": torch.arange(0, V + 1, V // G, device=dev).to(torch.int32), "graph_nodes_sorted": True,
        "target_values": torch.from_numpy(rng.normal(size=(1, G)).astype(np.float32)).to(dev), "target_mask": torch.ones((1, G), device=dev),
        "edge_weight_dropout_keep_prob": 1.0, "out_layer_dropout_keep_prob": 1.0}
is_fused = pkg.ops.gru_bwd_is_fused
routes = {"fused": is_fused, "parent": lambda D_: False}
names = ["fused", "parent"] if args.route == "both" else [args.route]


def run(name, steps):
    pkg.ops.gru_bwd_is_fused = routes[name]
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = model.train_batch(feed)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, float(loss)
    finally:
        pkg.ops.gru_bwd_is_fused = is_fused


for n in names:                                                   # warm-up: index, weight images, allocator
    run(n, 2)
t = {n: [] for n in names}
for _ in range(args.rounds):
    for n in names:
        t[n].append(run(n, args.steps)[0])
out = {"V": V, "M": M, "D": D, "timesteps": 8, "rounds": args.rounds, "steps_per_round": args.steps,
       "split_matrix_path": bool(pkg._lib.load().ggnn_matrix_path_is_split())}
for n in names:
    out[n] = {"median_ms": round(statistics.median(t[n]), 3), "min_ms": round(min(t[n]), 3), "max_ms": round(max(t[n]), 3)}
if len(names) == 2:
    out["ratio_parent_over_fused"] = round(out["parent"]["median_ms"] / out["fused"]["median_ms"], 3)
print(json.dumps(out), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
