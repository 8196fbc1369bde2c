"""Sparse GCN measurement: one JSON line for synthetic QM9 batches (~100k nodes, hidden 100, 4 layers).

  layer_us_fused / layer_us_composed   one ReLU layer, fused kernel (ggnn_gcn_layer_f32, weights pre-packed) against the composed
                                       path (weighted segment sum -> GEMM -> epilogue), device events over `--iters` launches
  forward_ms, node_updates_per_s       inference forward of all layers (ggnn_gcn_propagate_f32), V * layers / time
  train_step_ms                        one optimisation step through GCNLayerFn (forward, backward, clip + Adam)
  bytes_fused / bytes_composed         algorithmic HBM bytes of one layer (x read once, out written once, CSR; the composed path
                                       also writes and reads S and P), and the fraction of the 8 TB/s roof they reach.
Run from the repository root:  python tools/gcn_bench.py [--graphs 5600] [--iters 200]
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


def timed(fn, iters):
    for _ in range(5):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters          # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=5600)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gcn_bench needs a GPU"
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0)
    cfg = {"hidden_size": a.hidden, "num_timesteps": 4, "batch_size": 100000, "random_seed": 0}
    model = ggnn_amd.SparseGCNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms, "--config": cfg})
    feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
    g = feed['gcn_graph']
    h0 = feed['initial_node_representation']
    V, D = h0.shape
    x = torch.randn((V, D), device=h0.device)
    W = model.weights['edge_weights'][0]
    ops = ggnn_amd.ops
    img = ops.gcn_pack(W)
    fused_ms = timed(lambda: ops.gcn_layer(x, g, W, relu=True, img=img), a.iters)
    composed_ms = timed(lambda: ops.gcn_layer(x, g, W, relu=True, fused=False), a.iters)
    with torch.no_grad():
        model.feed(feed)
        fwd_ms = timed(model.compute_final_node_representations, a.iters // 4)
    tfeed = dict(next(iter(model.make_minibatch_iterator(model.train_data, is_training=True))), out_layer_dropout_keep_prob=1.0)
    step_ms = timed(lambda: model.train_batch(tfeed), 20)
    csr = (V + 1) * 4 + g.nnz * 8
    b_fused = 2 * V * D * 4 + csr
    b_comp = 6 * V * D * 4 + csr + g.nnz * 4
    print(json.dumps({
        "metric": "sparse GCN layer, synthetic QM9", "V": V, "nnz": g.nnz, "D": D, "layers": 4,
        "layer_us_fused": round(fused_ms * 1e3, 2), "layer_us_composed": round(composed_ms * 1e3, 2),
        "fused_speedup": round(composed_ms / fused_ms, 2),
        "forward_ms": round(fwd_ms, 4), "node_updates_per_s": V * 4 / (fwd_ms * 1e-3),
        "train_step_ms": round(step_ms, 3),
        "bytes_fused": b_fused, "bytes_composed": b_comp,
        "roof_fraction_fused": round(b_fused / HBM_ROOF / (fused_ms * 1e-3), 3),
        "roof_fraction_composed": round(b_comp / HBM_ROOF / (composed_ms * 1e-3), 3),
    }))


if __name__ == "__main__":
    main()
