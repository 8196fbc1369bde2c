"""Multi-task readout measurement (ggnn_readout_multi_*, params['multitask_readout']): JSON lines, one per measurement.

--leg kernel: at V ~ 1e5 nodes, D = 100, G ~ 5500 graphs and K in {1, 2, 4, 8, 13, 16} tasks, forward + backward of the per-task
loop (K calls of ops.readout_loss_fwd and K of ops.readout_loss_bwd, the later ones accumulating into d_hT) against one
ops.readout_multi_fwd and one ops.readout_multi_bwd call on the same inputs.
--leg step: one optimisation step of the native sparse GCN (params['native_training']) with 13 tasks, with and without the key, two
models in one process on the same resident batch.
Both arms run in one process in `--rounds` interleaved rounds of `--iters` repetitions, timed by device events:
  ms             per arm: median and min .. max over the rounds of the device-event time per repetition
  enqueue_ms     per arm: median host time per repetition to enqueue it (no synchronisation inside the timed loop)
  multi_faster   True only if the multi arm's whole range lies below the per-task arm's
--out FILE appends the JSON lines there.
Run from the repository root:  python tools/readout_bench.py --leg kernel
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


def _round(fn, iters):
    """(device ms, host enqueue ms) per call of `iters` back-to-back calls."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters, host * 1e3 / iters


def _interleaved(arms, rounds, iters, warmup=3):
    for fn in arms.values():                                # warm-up: caching allocator, LDS attributes
        _round(fn, warmup)
    dev = {n: [] for n in arms}
    host = {n: [] for n in arms}
    for _ in range(rounds):                                 # interleaved: both arms see the same clocks and the same neighbours
        for name, fn in arms.items():
            d, h = _round(fn, iters)
            dev[name].append(d); host[name].append(h)
    return {n: {"ms_median": round(float(np.median(dev[n])), 4), "ms_min": round(min(dev[n]), 4), "ms_max": round(max(dev[n]), 4),
                "enqueue_ms_median": round(float(np.median(host[n])), 4), "ms_rounds": [round(x, 4) for x in dev[n]]} for n in arms}


def _emit(out, path):
    out["multi_faster"] = bool(out["multi"]["ms_max"] < out["per_task"]["ms_min"])
    out["speedup_median"] = round(out["per_task"]["ms_median"] / out["multi"]["ms_median"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def kernel_leg(a):
    ops = ggnn_amd.ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    V, D, G = a.nodes, a.hidden, a.graphs
    sizes = rng.multinomial(V, np.ones(G) / G)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    gnl = t(np.repeat(np.arange(G), sizes).astype(np.int32))
    gptr = t(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
    hT, h0 = t(rng.uniform(-1, 1, (V, D)).astype(np.float32)), t(rng.uniform(-1, 1, (V, D)).astype(np.float32))
    for K in a.tasks:
        gW = [t(rng.uniform(-0.3, 0.3, 2 * D).astype(np.float32)) for _ in range(K)]
        tW = [t(rng.uniform(-0.3, 0.3, D).astype(np.float32)) for _ in range(K)]
        gb = [t(rng.uniform(-0.2, 0.2, 1).astype(np.float32)) for _ in range(K)]
        tb = [t(rng.uniform(-0.2, 0.2, 1).astype(np.float32)) for _ in range(K)]
        y, m = t(rng.normal(0, 1, (K, G)).astype(np.float32)), t((rng.random((K, G)) < 0.8).astype(np.float32))
        d_stats = t(np.tile(np.array([[1e-3, 0.0]], np.float32), (K, 1)))
        ys, ms_, ds = [y[k].contiguous() for k in range(K)], [m[k].contiguous() for k in range(K)], [d_stats[k].contiguous() for k in range(K)]

        def per_task():
            d = None
            for k in range(K):
                out, gate, val, _stats = ops.readout_loss_fwd(hT, h0, gnl, gptr, None, G, gW[k], gb[k], tW[k], tb[k], ys[k], ms_[k])
                d = ops.readout_loss_bwd(hT, h0, gnl, None, G, gW[k], tW[k], gate, val, out, ys[k], ms_[k], None, ds[k], d_last_h=d)[0]
            return d

        def multi():
            out, node_gv, _stats = ops.readout_multi_fwd(hT, h0, gnl, gptr, None, G, gW, gb, tW, tb, y, m)
            return ops.readout_multi_bwd(hT, h0, gnl, None, G, gW, tW, node_gv, out, y, m, None, d_stats)[0]

        apart = float((per_task() - multi()).abs().max())
        out = {"metric": "readout + loss, forward + backward", "V": V, "D": D, "G": G, "K": K, "rounds": a.rounds, "iters": a.iters,
               "d_hT_max_abs_apart": apart}
        out.update(_interleaved({"per_task": per_task, "multi": multi}, a.rounds, a.iters))
        _emit(out, a.out)


def step_leg(a):
    K = a.step_tasks
    ms = ggnn_amd.synthetic_qm9(a.graphs, mean_nodes=18, seed=0, num_tasks=K)
    cfg = {"hidden_size": a.hidden, "num_timesteps": 4, "batch_size": 100000, "random_seed": 0, "native_training": True,
           "task_ids": list(range(K))}
    arms, calls = {}, {}
    for name, extra in (("per_task", {}), ("multi", {"multitask_readout": True})):
        model = ggnn_amd.SparseGCNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms,
                                             "--config": dict(cfg, **extra)})
        np.random.seed(0)
        feed = dict(next(iter(model.make_minibatch_iterator(model.train_data, is_training=True))), out_layer_dropout_keep_prob=1.0)
        assert ggnn_amd.train_native.gcn_eligible(model, feed), name
        arms[name] = (lambda model=model, feed=feed: model.train_batch(feed))
        calls[name] = (model, feed)
    V, D = calls["multi"][1]["initial_node_representation"].shape
    out = {"metric": "native sparse GCN training step, synthetic QM9", "V": int(V), "D": int(D), "G": int(calls["multi"][1]["num_graphs"]),
           "K": K, "layers": 4, "rounds": a.rounds, "iters": a.iters}
    out.update(_interleaved(arms, a.rounds, a.iters, warmup=5))
    _emit(out, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("kernel", "step"), default="kernel")
    ap.add_argument("--nodes", type=int, default=100000)
    ap.add_argument("--graphs", type=int, default=5500)
    ap.add_argument("--hidden", type=int, default=100)
    ap.add_argument("--tasks", type=int, nargs="+", default=[1, 2, 4, 8, 13, 16])
    ap.add_argument("--step-tasks", type=int, default=13)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "readout_bench needs a GPU"
    with torch.no_grad():
        (kernel_leg if a.leg == "kernel" else step_leg)(a)


if __name__ == "__main__":
    main()
