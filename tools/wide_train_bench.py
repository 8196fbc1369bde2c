"""One training step of the sparse model on the config-5 graph (100,000 nodes / 1,000,000 edges / 4 edge types / h = 256 / 8
timesteps) with the column-panel GRU backward on the compacted route, and with ops.gru_bwd_is_fused switched off (the route before
the panel kernel existed: dense-form transform, unfused GRU backward), interleaved in one process.  Prints one JSON line.
--route native: the native two-call step (params['native_panel_training'], train_native.ROUTES, entry `panel`) against the
autograd step (`fused`) on a second model with the same config, interleaved in the same way; every arm then also reports the
launching thread's busy time per step (the time to enqueue a round's steps, before the device is waited for).
--shape qm9: a QM9-sized batch (~1e5 nodes, ~2e5 messages, h = 128, the default layer structure) instead of the config-5 graph.
   python tools/wide_train_bench.py [--route both|fused|parent|native] [--shape config5|qm9] [--rounds 7] [--steps 3] [--out FILE]"""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("gated-graph-neural-network-samples_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--route", default="both", choices=["both", "fused", "parent", "native"])
ap.add_argument("--shape", default="config5", choices=["config5", "qm9"])
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
def make_model(cfg, data):
    return pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": None, "valid_data": data, "--config": cfg})


if args.shape == "config5":
    V, M, T, D, G = 100000, 1000000, 4, 256, 1000
    adj_np, nin_np = pkg.synthetic_large_graph(V, M, T, seed=5, power_law=False)
    raw = [{"targets": [[0.0]], "graph": [[0, t + 1, 1] for t in range(T)], "node_features": [[1, 0, 0, 0, 0]] * 2}]
    cfg = {"hidden_size": D, "layer_timesteps": [8], "residual_connections": {}, "tie_fwd_bkwd": True}
    model = make_model(cfg, raw)
    rng = np.random.default_rng(6)
    feed = {"initial_node_representation": torch.from_numpy(rng.uniform(-1, 1, (V, D)).astype(np.float32)).to(dev),
            "adjacency_lists": [torch.from_numpy(a).to(dev) for a in adj_np],
            "num_incoming_edges_per_type": torch.from_numpy(nin_np).to(dev),
            "graph_nodes_list": (torch.arange(V, device=dev) // (V // G)).to(torch.int32), "num_graphs": G,
            "graph_ptr": torch.arange(0, V + 1, V // G, device=dev).to(torch.int32), "graph_nodes_sorted": True,
            "target_values": torch.from_numpy(rng.normal(size=(1, G)).astype(np.float32)).to(dev), "target_mask": torch.ones((1, G), device=dev),
            "edge_weight_dropout_keep_prob": 1.0, "out_layer_dropout_keep_prob": 1.0}
    # (the native step takes batches that come with their message index, as the model's own batches do)
    feed["message_index"] = pkg.ops.prepare_message_index(pkg.ops.build_message_index(feed["adjacency_lists"], V), D, True, training=True)
    timesteps = 8
else:
    D = 128
    raw = pkg.synthetic_qm9(5700, mean_nodes=18, seed=0)
    cfg = {"hidden_size": D}
    model = make_model(cfg, raw)
    feed = dict(next(iter(model.make_minibatch_iterator(model.valid_data, False))))
    feed["edge_weight_dropout_keep_prob"], feed["out_layer_dropout_keep_prob"] = model.params["edge_weight_dropout_keep_prob"], 1.0
    V, M = int(feed["initial_node_representation"].shape[0]), int(sum(a.shape[0] for a in feed["adjacency_lists"]))
    timesteps = int(sum(model.params["layer_timesteps"]))
models = {"fused": model, "parent": model}
if args.route == "native":
    models["native"] = make_model(dict(cfg, native_panel_training=True), raw)
    assert pkg.train_native.panel_eligible(models["native"], feed) and not pkg.train_native.panel_eligible(model, feed)
is_fused = pkg.ops.gru_bwd_is_fused
routes = {"fused": is_fused, "parent": lambda D_: False, "native": is_fused}
names = {"both": ["fused", "parent"], "native": ["native", "fused"]}.get(args.route, [args.route])


def run(name, steps):
    pkg.ops.gru_bwd_is_fused = routes[name]
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = models[name].train_batch(feed)
        t1 = time.perf_counter()                                  # (everything enqueued: the launching thread's busy time)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, (t1 - t0) * 1e3 / steps, float(loss)
    finally:
        pkg.ops.gru_bwd_is_fused = is_fused


for n in names:                                                   # warm-up: index, weight images, allocator
    run(n, 2)
t, busy = {n: [] for n in names}, {n: [] for n in names}
for _ in range(args.rounds):
    for n in names:
        step_ms, busy_ms, _ = run(n, args.steps)
        t[n].append(step_ms); busy[n].append(busy_ms)
out = {"shape": args.shape, "V": V, "M": M, "D": D, "timesteps": timesteps, "rounds": args.rounds, "steps_per_round": args.steps,
       "split_matrix_path": bool(pkg._lib.load().ggnn_matrix_path_is_split()),
       "merge_products_env": os.environ.get("GGNN_TRAIN_MERGE_PRODUCTS")}
for n in names:
    out[n] = {"median_ms": round(statistics.median(t[n]), 3), "min_ms": round(min(t[n]), 3), "max_ms": round(max(t[n]), 3),
              "host_busy_median_ms": round(statistics.median(busy[n]), 3), "host_busy_min_ms": round(min(busy[n]), 3),
              "host_busy_max_ms": round(max(busy[n]), 3)}
if args.route == "native":
    out["ratio_fused_over_native"] = round(out["fused"]["median_ms"] / out["native"]["median_ms"], 3)
if args.route == "both":
    out["ratio_parent_over_fused"] = round(out["parent"]["median_ms"] / out["fused"]["median_ms"], 3)
print(json.dumps(out), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
