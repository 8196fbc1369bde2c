"""Dense GGNN training epoch with batches packed on the host (pack_dense_batch + upload) and on the device (pack_on_device:
ggnn_dense_assemble_batch), in one run: one JSON line.  Synthetic QM9 (mean 18 atoms, `--graphs` molecules, the same set for
training and validation), the dense model's default params (batch_size 256, hidden 100, 4 timesteps).

  pack_ms_per_batch       packing alone: one training epoch's batches produced back to back, device events around the loop
  epoch_graphs_per_s      run_epoch's graphs/s for training and for validation, second of two epochs (validation batches are packed
                          on the first pass and stay resident); the device path inline and on the producer thread
  ms_per_step             training epoch time / steps
  assemble                one training-batch ggnn_dense_assemble_batch launch: algorithmic HBM bytes, device-event time, fraction of
                          the 8 TB/s roof
Run from the repository root:  python tools/dense_bench.py [--graphs 50000]
--leg pack: only device packing of `--iters` batches (for a kernel trace).
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
REFERENCE = {"train_graphs_per_s": 6758, "valid_graphs_per_s": 9902,
             "source": "the reference's README (chem_tensorflow_dense.py), hardware not stated"}


def _model(ms, cfg, pack_on_device, threaded):
    cfg = dict(cfg, pack_on_device=pack_on_device, threaded_batches=threaded)
    return ggnn_amd.DenseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms, "--config": cfg})


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


def _epoch(model, data, training, epochs=2):
    for _ in range(epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, _, graphs_per_s, steps = model.run_epoch("bench", data, training)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return graphs_per_s, dt * 1e3 / max(steps, 1), steps


def _assemble_bytes(feed, A_ann, T):
    """Algorithmic HBM bytes of one training-batch assembly: every output written once, the graphs' table entries and annotations
    read once."""
    b, v, D = feed["initial_node_representation"].shape
    _, index, nin = feed["_sparse_form"]
    V, M = b * v, index.num_messages
    comp = getattr(index, "_compact", None)
    R = comp.num_rows if comp is not None else 0
    n = int(feed["node_mask"].sum().item())
    K = feed["target_values"].shape[0]
    written = 4 * (V * D + b * T * v * v + V + 2 * K * b + V * T + (V + 1) + 2 * M + 2 * M)
    read = 4 * (n * A_ann + n * T + n + 2 * M + M) + 8 * K * b
    if comp is not None:
        written += 4 * (R + M + (V * T + 1) + 2 * M + (R + 1) + 2 * M + (V + 1) + R)
        read += 4 * (M + n * T + 2 * M + 3 * R + n)
    return int(written + read), {"b": int(b), "v": int(v), "M": int(M), "R": int(R)}


def epoch_leg(a):
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0)
    cfg = {"random_seed": 0}
    out = {"metric": "dense GGNN training epoch, synthetic QM9", "graphs": ms.num_graphs, "nodes": int(ms.node_ptr[-1]), "D": 100,
           "timesteps": 4, "batch_size": 256, "reference_dense_epoch": REFERENCE}
    for name, on_dev, threaded in (("host", False, "auto"), ("device", True, False), ("device_threaded", True, True)):
        model = _model(ms, cfg, on_dev, threaded)
        pack_ms, batches = _pack_ms(model)
        gps, step_ms, steps = _epoch(model, model.train_data, True)
        vgps, _, vsteps = _epoch(model, model.valid_data, False)
        out[name] = {"pack_ms_per_batch": round(pack_ms, 4), "epoch_graphs_per_s": {"train": round(gps, 1), "valid": round(vgps, 1)},
                     "ms_per_step": round(step_ms, 3), "batches": batches, "valid_batches": vsteps}
        if on_dev and not threaded:
            feed = next(iter(model.make_minibatch_iterator(model.train_data, is_training=True)))
            b_alg, shape = _assemble_bytes(feed, ms.node_feat.shape[1], model.num_edge_types)
            with ggnn_amd.ops.kernel_timing() as kt:
                for _ in range(3):
                    list(model.make_minibatch_iterator(model.train_data, is_training=True))
            us = float(np.median(kt.results()["dense_assemble_batch"])) * 1e3
            out["assemble"] = dict(shape, bytes=b_alg, us_events=round(us, 2), roof_fraction=round(b_alg / HBM_ROOF / (us * 1e-6), 3))
        del model
        torch.cuda.empty_cache()
    out["pack_speedup"] = round(out["host"]["pack_ms_per_batch"] / out["device"]["pack_ms_per_batch"], 1)
    out["train_epoch_speedup"] = round(out["device"]["epoch_graphs_per_s"]["train"] / out["host"]["epoch_graphs_per_s"]["train"], 2)
    print(json.dumps(out))


def pack_leg(a):
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0)
    model = _model(ms, {"random_seed": 0}, True, False)
    n = 0
    while n < a.iters:
        for _b in model.make_minibatch_iterator(model.train_data, is_training=True):
            n += 1
    torch.cuda.synchronize()
    print(json.dumps({"metric": "dense device packing", "batches": n}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=50000)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--leg", choices=("epoch", "pack"), default="epoch")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dense_bench needs a GPU"
    (epoch_leg if a.leg == "epoch" else pack_leg)(a)


if __name__ == "__main__":
    main()
