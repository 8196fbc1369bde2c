"""Sparse GCN measurement: one JSON line for synthetic QM9 batches (~100k nodes, hidden 100, 4 layers).

  layer_us_fused / layer_us_composed   one ReLU layer, fused kernel (ggnn_gcn_layer_f32, weights pre-packed) against the composed
                                       path (weighted segment sum -> GEMM -> epilogue), device events over `--iters` launches
  forward_ms, node_updates_per_s       inference forward of all layers (ggnn_gcn_propagate_f32), V * layers / time
  train_step_ms                        one optimisation step through GCNLayerFn (forward, backward, clip + Adam)
  bytes_fused / bytes_composed         algorithmic HBM bytes of one layer (x read once, out written once, CSR; the composed path
                                       also writes and reads S and P), and the fraction of the 8 TB/s roof they reach.
Run from the repository root:  python tools/gcn_bench.py [--graphs 5600] [--iters 200]

--leg epoch: training epochs over synthetic QM9 (mean 18 atoms, batch_size 100000, `--epoch-graphs` molecules) with the batches
packed on the host (pack_batch + gcn_csr_host + upload) and on the device (pack_on_device: ggnn_gcn_assemble_batch), in one run:
  pack_ms_per_batch   packing alone, one epoch's batches produced back to back, device events around the loop
  epoch_graphs_per_s  run_epoch's graphs/s (second of two epochs), the device path with and without the producer thread
  ms_per_step         epoch time / steps;  step_ms: one training step on a resident batch
  assemble            one ggnn_gcn_assemble_batch launch: algorithmic HBM bytes, device-event time, fraction of the 8 TB/s roof
--leg pack: only device packing of `--iters` batches (for a kernel trace).
--leg step: one training step at the benchmark batch through torch.autograd (GCNLayerFn) and on the native sequences
(params['native_training'], csrc/ggnn_gcn_train.hip), two models in one process on the same resident batch, `--rounds` interleaved
rounds of `--step-iters` steps each:
  step_ms        per arm: median and min .. max over the rounds of the device-event time per step
  enqueue_ms     per arm: median host time per step to enqueue it (no synchronisation inside the timed loop)
  native_faster  True only if the native arm's whole range lies below the autograd arm's
--hidden 128 / 192 / 256 (the column-panel kernel, csrc/ggnn_gcn_panel.hip; opt-in params['gcn_panel_layers']): both legs compare the
panel route with the composed route (weighted segment sum -> GEMM -> epilogue, what these sizes run without the key) in one
process, `--rounds` interleaved rounds:
  --leg layer    one ReLU layer (images pre-packed), its transposed form (the backward's dx launch) and the inference forward of all
                 layers, per arm median and min .. max over the rounds of the device-event time of `--iters` launches
  --leg step     one training step through GCNLayerFn on either route, and a third arm panel_native: the panel route with
                 params['native_training'] too (ggnn_gcn_panel_train_forward_f32 / _backward_f32, no torch.autograd)
  panel_faster   True only if the panel arm's whole range lies below the composed arm's
  native_faster  (step leg) True only if the panel_native arm's whole range lies below the panel arm's -- the autograd step on the
                 panel route is the fastest route these sizes had; native_speedup_median is against that arm
--out FILE also writes the JSON there.
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


def _epoch_model(ms, cfg, pack_on_device, threaded):
    cfg = dict(cfg, pack_on_device=pack_on_device, threaded_batches=threaded)
    return ggnn_amd.SparseGCNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms, "--config": cfg})


def _pack_ms(model, epochs=2):
    """ms per batch of producing one training epoch's batches back to back (nothing else queued), last of `epochs` epochs."""
    for _ in range(epochs):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        n = 0
        for _b in model.make_minibatch_iterator(model.train_data, is_training=True):
            n += 1
        e.record()
        torch.cuda.synchronize()
    return s.elapsed_time(e) / n, n


def _epoch(model, epochs=2):
    for _ in range(epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, _, graphs_per_s, steps = model.run_epoch("bench", model.train_data, True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return graphs_per_s, dt * 1e3 / steps, steps


def epoch_leg(a):
    ms = ggnn_amd.synthetic_qm9(a.epoch_graphs, mean_nodes=18, seed=0)
    cfg = {"hidden_size": a.hidden, "num_timesteps": 4, "batch_size": 100000, "random_seed": 0}
    out = {"metric": "sparse GCN training epoch, synthetic QM9", "graphs": ms.num_graphs, "nodes": int(ms.node_ptr[-1]), "D": a.hidden,
           "layers": 4, "batch_size": 100000}
    for name, on_dev, threaded in (("host", False, True), ("device", True, False), ("device_threaded", True, True)):
        model = _epoch_model(ms, cfg, on_dev, threaded)
        pack_ms, batches = _pack_ms(model)
        gps, step_ms, steps = _epoch(model)
        out[name] = {"pack_ms_per_batch": round(pack_ms, 4), "epoch_graphs_per_s": round(gps, 1), "ms_per_step": round(step_ms, 3),
                     "batches": batches}
        if on_dev and not threaded:
            feed = dict(next(iter(model.make_minibatch_iterator(model.train_data, is_training=True))), out_layer_dropout_keep_prob=1.0)
            out["step_ms"] = round(timed(lambda: model.train_batch(feed), 20), 3)
            V, D = feed["initial_node_representation"].shape
            g, G = feed["gcn_graph"], feed["num_graphs"]
            # h0 written; annotations read; both CSRs read and written (row_ptr, col, val); gnl, node_uid written; labels
            A = model.train_data["molecules"].node_feat.shape[1]
            b = V * D * 4 + V * A * 4 + 2 * 2 * ((V + 1) * 4 + g.nnz * 8) + V * (4 + 8) + G * 4 * 4
            with ggnn_amd.ops.kernel_timing() as kt:
                for _ in range(20):
                    list(model.make_minibatch_iterator(model.train_data, is_training=True))
            us = float(np.median(kt.results()["gcn_assemble_batch"])) * 1e3
            out["assemble"] = {"V": int(V), "nnz": g.nnz, "bytes": int(b), "us_events": round(us, 2),
                               "roof_fraction": round(b / HBM_ROOF / (us * 1e-6), 3)}
        del model
        torch.cuda.empty_cache()
    out["pack_speedup"] = round(out["host"]["pack_ms_per_batch"] / out["device"]["pack_ms_per_batch"], 1)
    out["epoch_speedup"] = round(out["device"]["epoch_graphs_per_s"] / out["host"]["epoch_graphs_per_s"], 2)
    print(json.dumps(out))


def pack_leg(a):
    ms = ggnn_amd.synthetic_qm9(a.epoch_graphs, mean_nodes=18, seed=0)
    model = _epoch_model(ms, {"hidden_size": a.hidden, "num_timesteps": 4, "batch_size": 100000, "random_seed": 0}, True, False)
    n = 0
    while n < a.iters:
        for _b in model.make_minibatch_iterator(model.train_data, is_training=True):
            n += 1
    torch.cuda.synchronize()
    print(json.dumps({"metric": "GCN device packing", "batches": n}))


def _step_round(model, feed, iters):
    """(device ms per step, host enqueue ms per step) of `iters` back-to-back training steps."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record()
    for _ in range(iters):
        model.train_batch(feed)
    e.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters, host * 1e3 / iters


def _spread(values, digits=2):
    return {"median": round(float(np.median(values)), digits), "min": round(min(values), digits), "max": round(max(values), digits),
            "rounds": [round(v, digits) for v in values]}


def _emit(a, out):
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def _panel_models(a, ms, native=False):
    cfg = {"hidden_size": a.hidden, "num_timesteps": 4, "batch_size": 100000, "random_seed": 0}
    arms = (("composed", {}), ("panel", {"gcn_panel_layers": True}))
    if native:
        arms += (("panel_native", {"gcn_panel_layers": True, "native_training": True}),)
    return {name: ggnn_amd.SparseGCNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms,
                                               "--config": dict(cfg, **extra)})
            for name, extra in arms}


def panel_layer_leg(a):
    """One layer, its transposed form and the inference forward at a panel size: panel route against composed route, interleaved."""
    ops = ggnn_amd.ops
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0)
    models = _panel_models(a, ms)
    assert models["panel"].gcn_panel_route() and not models["composed"].gcn_panel_route()
    feed = next(iter(models["panel"].make_minibatch_iterator(models["panel"].valid_data, is_training=False)))
    g, h0 = feed['gcn_graph'], feed['initial_node_representation']
    V, D = h0.shape
    x = torch.randn((V, D), device=h0.device)
    W = models["panel"].weights['edge_weights'][0]
    img, img_t = ops.gcn_panel_pack(W), ops.gcn_panel_pack(W, True)
    for m in models.values():
        m.feed(feed)
    work = {
        "layer_us": {"panel": lambda: ops.gcn_layer(x, g, W, relu=True, img=img, panel=True),
                     "composed": lambda: ops.gcn_layer(x, g, W, relu=True)},
        "layer_transposed_us": {"panel": lambda: ops.gcn_layer(x, g, W, transpose=True, img=img_t, panel=True),
                                "composed": lambda: ops.gcn_layer(x, g, W, transpose=True)},
        "forward_us": {name: m.compute_final_node_representations for name, m in models.items()},
    }
    csr = (V + 1) * 4 + g.nnz * 8
    out = {"metric": "sparse GCN layer on column panels, synthetic QM9", "V": V, "nnz": g.nnz, "D": D, "layers": 4, "rounds": a.rounds,
           "launches_per_round": a.iters, "bytes_panel": 2 * V * D * 4 + csr, "bytes_composed": 6 * V * D * 4 + csr + g.nnz * 4}
    with torch.no_grad():
        for what, arms in work.items():
            iters = max(a.iters // 4, 1) if what == "forward_us" else a.iters
            times = {name: [] for name in arms}
            for _ in range(a.rounds):                       # interleaved: both arms see the same clocks and the same neighbours
                for name, fn in arms.items():
                    times[name].append(timed(fn, iters) * 1e3)
            out[what] = {name: _spread(t) for name, t in times.items()}
            out[what]["panel_faster"] = bool(max(times["panel"]) < min(times["composed"]))
            out[what]["speedup_median"] = round(float(np.median(times["composed"]) / np.median(times["panel"])), 3)
    out["roof_fraction_panel"] = round(out["bytes_panel"] / HBM_ROOF / (out["layer_us"]["panel"]["median"] * 1e-6), 3)
    out["roof_fraction_composed"] = round(out["bytes_composed"] / HBM_ROOF / (out["layer_us"]["composed"]["median"] * 1e-6), 3)
    _emit(a, out)


def panel_step_leg(a):
    """One training step at a panel size: composed route and panel route through GCNLayerFn, and the panel route on the native
    sequences, interleaved."""
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0)
    arms = {}
    for name, model in _panel_models(a, ms, native=True).items():
        np.random.seed(0)
        feed = dict(next(iter(model.make_minibatch_iterator(model.train_data, is_training=True))), out_layer_dropout_keep_prob=1.0)
        assert model.gcn_panel_route() == (name != "composed"), name
        assert ggnn_amd.train_native.gcn_eligible(model, feed) == (name == "panel_native"), name
        arms[name] = (model, feed)
    V, D = arms["panel"][1]["initial_node_representation"].shape
    for model, feed in arms.values():                       # warm-up: workspaces, caching allocator, LDS attributes
        _step_round(model, feed, 5)
    dev = {n: [] for n in arms}
    host = {n: [] for n in arms}
    for _ in range(a.rounds):
        for name, (model, feed) in arms.items():
            d, h = _step_round(model, feed, a.step_iters)
            dev[name].append(d); host[name].append(h)
    out = {"metric": "sparse GCN training step on column panels, synthetic QM9", "V": int(V), "nnz": arms["panel"][1]["gcn_graph"].nnz,
           "D": int(D), "layers": 4, "rounds": a.rounds, "steps_per_round": a.step_iters}
    for name in arms:
        out[name] = {"step_ms": _spread(dev[name], 4), "enqueue_ms_median": round(float(np.median(host[name])), 4)}
    out["panel_faster"] = bool(max(dev["panel"]) < min(dev["composed"]))
    out["speedup_median"] = round(float(np.median(dev["composed"]) / np.median(dev["panel"])), 3)
    out["native_faster"] = bool(max(dev["panel_native"]) < min(dev["panel"]))
    out["native_speedup_median"] = round(float(np.median(dev["panel"]) / np.median(dev["panel_native"])), 3)
    _emit(a, out)


def step_leg(a):
    if ggnn_amd.ops.gcn_panel_supported(a.hidden):
        return panel_step_leg(a)
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0)
    cfg = {"hidden_size": a.hidden, "num_timesteps": 4, "batch_size": 100000, "random_seed": 0}
    arms = {}
    for name, extra in (("autograd", {}), ("native", {"native_training": True})):
        model = ggnn_amd.SparseGCNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms,
                                             "--config": dict(cfg, **extra)})
        np.random.seed(0)
        feed = dict(next(iter(model.make_minibatch_iterator(model.train_data, is_training=True))), out_layer_dropout_keep_prob=1.0)
        assert ggnn_amd.train_native.gcn_eligible(model, feed) == (name == "native"), name
        arms[name] = (model, feed)
    V, D = arms["native"][1]["initial_node_representation"].shape
    for model, feed in arms.values():                       # warm-up: workspaces, caching allocator, LDS attributes
        _step_round(model, feed, 5)
    dev = {n: [] for n in arms}
    host = {n: [] for n in arms}
    for _ in range(a.rounds):                               # interleaved: both arms see the same clocks and the same neighbours
        for name, (model, feed) in arms.items():
            d, h = _step_round(model, feed, a.step_iters)
            dev[name].append(d); host[name].append(h)
    out = {"metric": "sparse GCN training step, synthetic QM9", "V": int(V), "nnz": arms["native"][1]["gcn_graph"].nnz, "D": int(D),
           "layers": 4, "rounds": a.rounds, "steps_per_round": a.step_iters}
    for name in arms:
        out[name] = {"step_ms_median": round(float(np.median(dev[name])), 4), "step_ms_min": round(min(dev[name]), 4),
                     "step_ms_max": round(max(dev[name]), 4), "enqueue_ms_median": round(float(np.median(host[name])), 4),
                     "step_ms_rounds": [round(x, 4) for x in dev[name]]}
    out["native_faster"] = bool(out["native"]["step_ms_max"] < out["autograd"]["step_ms_min"])
    out["speedup_median"] = round(out["autograd"]["step_ms_median"] / out["native"]["step_ms_median"], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=5600)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=100)
    ap.add_argument("--leg", choices=("layer", "epoch", "pack", "step"), default="layer")
    ap.add_argument("--epoch-graphs", type=int, default=33600)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--step-iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gcn_bench needs a GPU"
    if a.leg == "step":
        return step_leg(a)
    if a.leg != "layer":
        return (epoch_leg if a.leg == "epoch" else pack_leg)(a)
    if ggnn_amd.ops.gcn_panel_supported(a.hidden):
        return panel_layer_leg(a)
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
