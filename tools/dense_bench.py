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
--graph-resident: the epoch leg with params['graph_resident_training'] (the graph-resident forward and backward launches).
--leg step: one training step of a 256-graph batch at v = 16 and v = 29 (D 100, 4 edge types, 4 timesteps) on today's per-timestep
  route and on the graph-resident route, in ONE process with the routes alternating in interleaved rounds; device events around whole
  steps that end in a synchronise; median / min / max per route -> one JSON line (and --out FILE).
--leg trace: `--iters` graph-resident steps at v = 29 (for rocprofv3 --kernel-trace --stats, the program after `--`).
--leg roof --kernel-stats FILE: the saving forward's and the backward launch's average time from that run's kernel-stats CSV against
  their algorithmic bytes and flops (computed here from the shapes) -> the share of the bounding roof.
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
    cfg = {"random_seed": 0, "graph_resident_training": True} if a.graph_resident else {"random_seed": 0}
    out = {"metric": "dense GGNN training epoch, synthetic QM9", "graph_resident_training": bool(a.graph_resident), "graphs": ms.num_graphs, "nodes": int(ms.node_ptr[-1]), "D": 100,
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


def _step_feed(model, ms, v, batch=256):
    """A training feed of `batch` graphs with at most v vertices in a bucket of v (pack_dense_batch, as make_minibatch_iterator's)."""
    ids = np.nonzero(ms.nodes_per_graph() <= v)[0][:batch]
    assert len(ids) == batch, "not enough graphs of <= %d vertices" % v
    db = ggnn_amd.data.pack_dense_batch(ms, ids, v, model.num_edge_types, model.params['hidden_size'], model.params['tie_fwd_bkwd'],
                                        model.params['task_ids'])
    feed = model.to_device_batch(db)
    feed['graph_state_keep_prob'] = feed['edge_weight_dropout_keep_prob'] = 1.0
    return feed


def _timed_step(model, feed):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    model.train_batch(feed)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def _step_models(ms):
    cfg = {"random_seed": 0}
    return {"per_timestep": _model(ms, cfg, False, False), "graph_resident": _model(ms, dict(cfg, graph_resident_training=True), False, False)}


def step_leg(a):
    ms = ggnn_amd.synthetic_qm9(max(a.graphs, 4000), mean_nodes=14, seed=0)
    models = _step_models(ms)
    out = {"metric": "dense GGNN training step, 256 graphs, D 100, 4 edge types, 4 timesteps", "unit": "ms per step (device events)",
           "rounds": a.rounds, "steps_per_round": a.reps, "shapes": {}}
    for v in (16, 29):
        feeds = {k: _step_feed(m, ms, v) for k, m in models.items()}
        for k, m in models.items():                                    # warm up every shape on every route
            for _ in range(5):
                _timed_step(m, feeds[k])
        ms_ = {k: [] for k in models}
        for r in range(a.rounds):                                      # interleaved rounds, the order alternating
            for k in (list(models) if r % 2 == 0 else list(models)[::-1]):
                ms_[k] += [_timed_step(models[k], feeds[k]) for _ in range(a.reps)]
        res = {k: {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for k, t in ms_.items()}
        res["speedup_median"] = round(res["per_timestep"]["median"] / res["graph_resident"]["median"], 2)
        res["node_rows"] = 256 * v
        out["shapes"]["v%d" % v] = res
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def trace_leg(a):
    ms = ggnn_amd.synthetic_qm9(4000, mean_nodes=14, seed=0)
    model = _step_models(ms)["graph_resident"]
    feed = _step_feed(model, ms, 29)
    for _ in range(a.iters):
        model.train_batch(feed)
    torch.cuda.synchronize()
    print(json.dumps({"metric": "graph-resident dense training steps", "steps": a.iters}))


MATRIX_ROOF_BF16 = 2.5e15          # flop/s of v_mfma_f32_16x16x32_bf16 on the whole chip (csrc/ggnn_split.hpp)


def roof_leg(a):
    """Algorithmic traffic and work of the two launches at b 256, v 29, E 4, D 100, 4 timesteps.  A D x D product runs on 32-row
    tiles as six bf16 MFMA products in the exact format (the backward, and a forward launched with fmt 3) or as three f16 ones (a
    forward launched with fmt 2: the format is read from the traced instantiation's name), so the matrix-pipe time is 6 x or 3 x the
    padded flops at the 16-bit rate; the adjacency products are f32 MFMAs and are left out.  Only the SAVING instantiation
    <100, 4, 8, fmt, true> of the forward counts; a trace that holds it in both formats is refused."""
    import csv
    import re
    b, v, E, D, steps = 256, 29, 4, 100, 4
    rows = b * v
    f = 4
    w_bytes = (E * D * D + 4 * D * D + 2 * D * D) * f
    fwd_bytes = (2 * rows * D + b * E * v * v + 6 * steps * rows * D) * f + w_bytes
    bwd_bytes = (2 * rows * D + b * E * v * v + 4 * steps * rows * D + steps * rows * (4 + E) * D) * f + w_bytes
    flops = 2.0 * b * steps * (6 + E) * v * D * D                       # algorithmic, either direction
    padded = 2.0 * b * steps * (6 + E) * 32 * 112 * 112                # one product on 32-row tiles, 7 x 16 columns
    pats = {"forward_save": re.compile(r"ggnn_dense_graph_split_kernel<\s*%d,\s*%d,\s*8,\s*([23]),\s*true\s*>" % (D, E)),
            "backward": re.compile(r"ggnn_dense_graph_bwd_kernel<\s*%d,\s*%d,\s*8\s*>" % (D, E))}
    found = {}
    with open(a.kernel_stats) as fh:
        for row in csv.DictReader(fh):
            for key, pat in pats.items():
                m = pat.search(row.get("Name", ""))
                if m:
                    assert key not in found, "the trace holds more than one instantiation of the %s launch" % key
                    found[key] = (float(row["AverageNs"]) * 1e-9, int(row["Calls"]), int(m.group(1)) if m.groups() else 3)
    out = {"shape": {"b": b, "v": v, "E": E, "D": D, "steps": steps}}
    for key, nbytes in (("forward_save", fwd_bytes), ("backward", bwd_bytes)):
        t, calls, fmt = found[key]
        products = 6 if fmt == 3 else 3
        hbm, mat = nbytes / HBM_ROOF / t, products * padded / MATRIX_ROOF_BF16 / t
        out[key] = {"kernel_us": round(t * 1e6, 2), "calls": calls, "operand_format": "bf16x3" if fmt == 3 else "f16x2",
                    "algorithmic_bytes": int(nbytes), "algorithmic_flops": int(flops), "hbm_roof_share": round(hbm, 3),
                    "matrix_roof_share": round(mat, 3), "bounding_roof": "hbm" if hbm > mat else "16-bit matrix pipe"}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=50000)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--leg", choices=("epoch", "pack", "step", "trace", "roof"), default="epoch")
    ap.add_argument("--graph-resident", action="store_true", help="epoch leg: params['graph_resident_training']")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.leg == "roof":
        return roof_leg(a)
    assert torch.cuda.is_available(), "dense_bench needs a GPU"
    {"epoch": epoch_leg, "pack": pack_leg, "step": step_leg, "trace": trace_leg}[a.leg](a)


if __name__ == "__main__":
    main()
