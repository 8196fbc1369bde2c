"""The column-panel GRU backward (one launch: ggnn_gru_bwd_fused_f32 at D = 128 / 192 / 256) against the three launches it
replaces (gru_bwd_stage1 + gru_bwd_dx_cand + gru_bwd_dx_gates; the weight-gradient products are excluded on both sides), in ONE
process, interleaved rounds, at V = 100,000 and nx = 1, 2.  Prints one JSON line per shape: median / min / max over the rounds in
microseconds, and the fused launch's rate over its algorithmic bytes (10 + nx) V D 4.
   python tools/gru_bwd_panel_bench.py [--rounds 9] [--inner 10] [--out FILE]"""
import argparse, importlib, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("gated-graph-neural-network-samples_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ops, backward, lib = pkg.ops, pkg.backward, pkg._lib.load()
dev, V, T = "cuda:0", 100000, 4
torch.manual_seed(0)
rnd = lambda *s: torch.rand(*s, device=dev) * 2 - 1


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


lines = []
for D in (128, 192, 256):
    for nx in (1, 2):
        g, h, c = rnd(V, D), rnd(V, D), rnd(V, D)
        r, u = torch.rand(V, D, device=dev), torch.rand(V, D, device=dev)
        Wg, Wc = rnd((nx + 1) * D, 2 * D) * 0.1, rnd((nx + 1) * D, D) * 0.1
        nin = torch.randint(0, 3, (V, T), device=dev).float()
        packed = ops.PackedWeights().gru_bwd(Wg, Wc, nx, D)
        WcT, WgT = backward.transposed(Wc), backward.transposed(Wg)
        dpc, dh, rh, dinc = (torch.empty_like(h) for _ in range(4))
        dpg = torch.empty((V, 2 * D), device=dev)
        dx = torch.empty((V, nx * D), device=dev)
        st = torch.cuda.current_stream().cuda_stream
        p = lambda t: t.data_ptr()
        stage1 = lambda: pkg._lib.check(lib.ggnn_gru_bwd_stage1_f32(p(g), p(h), p(r), p(u), p(c), 0, p(dpc), p(dpg), p(dh), p(rh), D, 0, V, D, st))
        dx_cand = lambda: pkg._lib.check(lib.ggnn_gru_bwd_dx_cand_f32(p(dpc), p(WcT), p(h), p(r), p(dx), p(dh), p(dpg), nx, V, D, st))
        dx_gates = lambda: pkg._lib.check(lib.ggnn_gru_bwd_dx_gates_f32(p(dpg), p(WgT), p(dx), p(dinc), p(nin), T, 1, p(dh), nx, V, D, st))
        fused = lambda: ops.gru_bwd_fused(g, h, r, u, c, packed, nin, True, nx, "tanh")
        legs = {"fused": fused, "stage1": stage1, "dx_cand": dx_cand, "dx_gates": dx_gates}
        for fn in legs.values():                                  # warm-up
            timed(fn, 3)
        t = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                t[k].append(timed(fn, args.inner))
        stat = lambda v: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
        three = [a + b + c_ for a, b, c_ in zip(t["stage1"], t["dx_cand"], t["dx_gates"])]
        alg = (10 + nx) * V * D * 4
        line = {"V": V, "D": D, "nx": nx, "split_matrix_path": bool(lib.ggnn_matrix_path_is_split()), "rounds": args.rounds, "inner": args.inner,
                "fused": stat(t["fused"]), "unfused_sum": stat(three), "stage1": stat(t["stage1"]), "dx_cand": stat(t["dx_cand"]),
                "dx_gates": stat(t["dx_gates"]), "ratio_unfused_over_fused": round(statistics.median(three) / statistics.median(t["fused"]), 3),
                "fused_faster_beyond_spread": bool(max(t["fused"]) < min(three)),
                "algorithmic_bytes": alg, "fused_TB_per_s": round(alg / statistics.median(t["fused"]) / 1e6, 3)}
        print(json.dumps(line), flush=True)
        lines.append(line)
if args.out:
    with open(args.out, "w") as f:
        json.dump(lines, f, indent=1)
