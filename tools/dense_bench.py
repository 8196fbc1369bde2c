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
--graph-resident [native]: the epoch leg with params['graph_resident_training'] True (the graph-resident forward and backward
  launches under torch.autograd) or 'native' (the native step, train_native.ROUTES, entry `dense`).
--leg step: one training step of a 256-graph batch at v = 16 and v = 29 (D 100, 4 edge types, 4 timesteps) on the per-timestep
  route, on the graph-resident route and on the native step, in ONE process with the routes alternating in interleaved rounds; device
  events around whole steps that end in a synchronise; median / min / max per route and the median of every round, plus the host time
  to enqueue a step (as tools/host_profile.py measures it) -> one JSON line (and --out FILE).
--leg trace: `--iters` graph-resident steps at v = 29 (for rocprofv3 --kernel-trace --stats, the program after `--`); with
  --graph-resident native the native step's.
--leg edge-grad: ggnn_dense_edge_grad_f32 against what it replaces on the same operands (two ggnn_gemm_tn_f32 calls and the permute
  copy) at N = 29 696 and N = 16 384 rows (D 100, 4 edge types): HIP events, warm-up, interleaved rounds in alternating order.
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
    cfg = {"random_seed": 0, "graph_resident_training": a.graph_resident} if a.graph_resident else {"random_seed": 0}
    out = {"metric": "dense GGNN training epoch, synthetic QM9", "graph_resident_training": a.graph_resident, "graphs": ms.num_graphs, "nodes": int(ms.node_ptr[-1]), "D": 100,
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
    return {"per_timestep": _model(ms, cfg, False, False), "graph_resident": _model(ms, dict(cfg, graph_resident_training=True), False, False),
            "native": _model(ms, dict(cfg, graph_resident_training="native"), False, False)}


def _enqueue_ms(model, feed, n=30):
    """Host time to enqueue a step (tools/host_profile.py): n steps back to back, the clock stopped before the device is drained."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        model.train_batch(feed)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / n * 1e3


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
        per_round = {k: [] for k in models}
        for r in range(a.rounds):                                      # interleaved rounds, the order alternating
            for k in (list(models) if r % 2 == 0 else list(models)[::-1]):
                t = [_timed_step(models[k], feeds[k]) for _ in range(a.reps)]
                ms_[k] += t
                per_round[k].append(round(float(np.median(t)), 4))
        res = {k: {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4),
                   "round_medians": per_round[k], "host_enqueue_ms": round(_enqueue_ms(models[k], feeds[k]), 4)} for k, t in ms_.items()}
        res["speedup_median"] = round(res["per_timestep"]["median"] / res["graph_resident"]["median"], 2)
        res["native_speedup_median"] = round(res["graph_resident"]["median"] / res["native"]["median"], 2)
        res["native_below_graph_resident_in_every_round"] = all(n < g for n, g in zip(per_round["native"], per_round["graph_resident"]))
        res["node_rows"] = 256 * v
        out["shapes"]["v%d" % v] = res
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def trace_leg(a):
    ms = ggnn_amd.synthetic_qm9(4000, mean_nodes=14, seed=0)
    route = "native" if a.graph_resident == "native" else "graph_resident"
    model = _model(ms, {"random_seed": 0, "graph_resident_training": "native" if route == "native" else True}, False, False)
    feed = _step_feed(model, ms, 29)
    for _ in range(a.iters):
        model.train_batch(feed)
    torch.cuda.synchronize()
    print(json.dumps({"metric": "%s dense training steps" % route.replace("_", "-"), "steps": a.iters}))


MATRIX_ROOF_F32 = 157e12           # flop/s of v_mfma_f32_16x16x4_f32 on the whole chip


def edge_grad_leg(a):
    """ggnn_dense_edge_grad_f32 against the two ggnn_gemm_tn_f32 calls + permute copy it replaces, on the same operands."""
    ops = ggnn_amd.ops
    E, D = 4, 100
    out = {"metric": "dense edge-weight + edge-bias gradients, E 4, D 100", "unit": "us per call group (device events)",
           "rounds": a.rounds, "calls_per_round": a.reps, "shapes": {}}
    gen = torch.Generator(device="cpu").manual_seed(0)
    for N, rps in ((4 * 256 * 29, 256 * 29), (4 * 256 * 16, 256 * 16)):
        h = torch.rand((N, D), generator=gen).cuda() * 2 - 1
        dM, dx = torch.randn((N, E * D), generator=gen).cuda(), torch.randn((N, D), generator=gen).cuda()
        nin = torch.randint(0, 4, (rps, E), generator=gen).float().cuda()
        ws = torch.empty(ggnn_amd._lib.load().ggnn_dense_edge_grad_workspace_bytes(N, E, D), dtype=torch.uint8, device="cuda")
        dW, db = torch.empty((E, D, D), device="cuda"), torch.empty((E, D), device="cuda")
        nin_rows = nin.repeat(N // rps, 1)                           # (the autograd route's copy is made outside the timed region)

        def new():
            ops.dense_edge_grad(h, dM, nin, dx, dW=dW, db=db, ws=ws)

        def replaced():                                              # backward.DensePropagateFn's edge products
            ops.gemm_tn(h, dM).view(D, E, D).permute(1, 0, 2).contiguous()
            ops.gemm_tn(nin_rows, dx)

        def timed(fn):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / a.reps

        arms = {"dense_edge_grad": new, "gemm_tn_x2_permute": replaced}
        for fn in arms.values():
            timed(fn)
        rounds = {k: [] for k in arms}
        for r in range(a.rounds):
            for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
                rounds[k].append(round(timed(arms[k]), 2))
        nbytes = 4 * (N * D * (2 + E) + rps * E + E * D * D + E * D)
        flops = 2.0 * N * D * (E * D + E)
        med = float(np.median(rounds["dense_edge_grad"]))
        out["shapes"]["N%d" % N] = {
            "round_us": rounds, "median_us": {k: round(float(np.median(t)), 2) for k, t in rounds.items()},
            "lower_in_every_round": all(x < y for x, y in zip(rounds["dense_edge_grad"], rounds["gemm_tn_x2_permute"])),
            "operand_bytes": nbytes, "flops": int(flops), "hbm_roof_us": round(nbytes / HBM_ROOF * 1e6, 2),
            "f32_mfma_roof_us": round(flops / MATRIX_ROOF_F32 * 1e6, 2),
            "share_of_f32_mfma_roof": round(flops / MATRIX_ROOF_F32 * 1e6 / med, 3),
            "note": "events around back-to-back calls on one stream: launch gaps and the reduce launch are inside the figure"}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


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
    ap.add_argument("--leg", choices=("epoch", "pack", "step", "trace", "roof", "edge-grad"), default="epoch")
    ap.add_argument("--graph-resident", nargs="?", const=True, default=False, choices=(True, "native"),
                    help="epoch / trace leg: params['graph_resident_training'] (no value: True; 'native': the native step)")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.leg == "roof":
        return roof_leg(a)
    assert torch.cuda.is_available(), "dense_bench needs a GPU"
    {"epoch": epoch_leg, "pack": pack_leg, "step": step_leg, "trace": trace_leg, "edge-grad": edge_grad_leg}[a.leg](a)


if __name__ == "__main__":
    main()
