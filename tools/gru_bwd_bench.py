"""Stand-alone timing of the fused GRU backward launch of one shape (V = 99990, mean aggregation, tanh), on the matrix path of
the process (GGNN_MATRIX) and the library GGNN_LIB_VARIANT names -- e.g. the parent commit's, for an A/B of one launch.
   python tools/gru_bwd_bench.py [D=100] [nx=1] [--rounds 5] [--inner 50]        prints one JSON line"""
import argparse, importlib, json, os, statistics, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("gated-graph-neural-network-samples_amd")
ap = argparse.ArgumentParser()
ap.add_argument("D", nargs="?", type=int, default=100)
ap.add_argument("nx", nargs="?", type=int, default=1)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--inner", type=int, default=50)
a = ap.parse_args()
V, D, nx, T = 99990, a.D, a.nx, 4
dev = "cuda:0"
torch.manual_seed(0)
r = lambda *s: torch.rand(*s, device=dev) * 2 - 1
g, h, c = r(V, D), r(V, D), r(V, D)
rr, u = torch.rand(V, D, device=dev), torch.rand(V, D, device=dev)
Wg, Wc = r((nx + 1) * D, 2 * D) * 0.2, r((nx + 1) * D, D) * 0.2
nin = torch.ones(V, T, device=dev)
packed = pkg.ops.PackedWeights().gru_bwd(Wg, Wc, nx, D)
run = lambda: pkg.ops.gru_bwd_fused(g, h, rr, u, c, packed, nin, True, nx, "tanh")
for _ in range(5): run()
torch.cuda.synchronize()
us = []
for _ in range(a.rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.inner): run()
    e1.record(); torch.cuda.synchronize()
    us.append(e0.elapsed_time(e1) * 1e3 / a.inner)
print(json.dumps({"D": D, "nx": nx, "V": V, "library": os.path.basename(pkg._lib.LIB_PATH), "matrix": os.environ.get("GGNN_MATRIX", "default"),
                  "rounds_us": [round(x, 2) for x in us], "median_us": round(statistics.median(us), 2)}), flush=True)
