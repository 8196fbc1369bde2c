"""Multi-task fused readout + masked loss (ggnn_readout_multi_{fwd,bwd}_f32, autograd.readout_loss_multi): all K tasks in one pass
against a float64 torch restatement (test_gpu_readout._reference looped over the tasks) under test_gpu_readout's bounds -- the same
quantities from the same f32 arithmetic --, against the per-task kernels, and its determinism, its independence of K, the
accumulate form and the fall-back for (D, K) outside the supported set."""
import functools
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

#          V     G   D    K  node_mask  empty graph id
SHAPES = [(1, 1, 32, 1, False, False),
          (17, 3, 100, 2, False, False),                 # a partial node tile
          (1000, 37, 100, 13, False, False),
          (5003, 300, 100, 16, False, True),             # a graph id that has no nodes; more tiles than one block's share at 16/tile
          (29 * 64, 64, 64, 5, True, False),
          (700, 1, 32, 16, False, False),
          (0, 4, 100, 3, False, False),
          (20000, 130, 256, 16, True, True)]             # the widest kernels (4 column slots, 12 accumulator slots, > 48 KB of LDS)
                                                         # and more nodes than one pass of either grid: the grid-stride loops go round again
IDS = ["V%d-G%d-D%d-K%d" % s[:4] for s in SHAPES]
NAMES = ("d_hT", "d_gate_W", "d_gate_b", "d_transform_W", "d_transform_b")


@functools.lru_cache(maxsize=None)
def _case(shape):
    V, G, D, K, with_node_mask, empty = shape
    rng = np.random.default_rng(1000 * V + 10 * G + K)
    sizes = rng.multinomial(V, np.ones(G) / G)
    if empty and G > 2:
        sizes[1] += sizes[2]; sizes[2] = 0                       # a graph id without nodes
    c = {"gnl": np.repeat(np.arange(G), sizes).astype(np.int32),
         "hT": rng.uniform(-1, 1, (V, D)).astype(np.float32), "h0": rng.uniform(-1, 1, (V, D)).astype(np.float32),
         "gW": rng.uniform(-0.3, 0.3, (K, 2 * D, 1)).astype(np.float32), "gb": rng.uniform(-0.2, 0.2, (K, 1)).astype(np.float32),
         "tW": rng.uniform(-0.3, 0.3, (K, D, 1)).astype(np.float32), "tb": rng.uniform(-0.2, 0.2, (K, 1)).astype(np.float32),
         "y": rng.normal(0, 1, (K, G)).astype(np.float32), "m": (rng.random((K, G)) < 0.8).astype(np.float32),
         "nm": (rng.random(V) < 0.85).astype(np.float32) if with_node_mask else None,
         "a": rng.uniform(0.2, 1.0, K), "b": rng.uniform(0.1, 0.5, K), "w": rng.normal(0, 1, (K, G)).astype(np.float32)}
    if K >= 2:
        c["m"][K // 2] = 0.0                                     # one task whose mask is all zero
    c["gptr"] = np.concatenate([[0], np.cumsum(np.bincount(c["gnl"], minlength=G))]).astype(np.int32)
    return c


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """float64: test_gpu_readout._reference for every task, one hT leaf; -> (out [K,G], num, ab, ms [K], gradients of
    total = sum_k a_k num_k + b_k ab_k + (out_k . w_k) as NumPy: d_hT [V,D], d_gate_W [K,2D,1], d_gate_b [K,1], ...)."""
    V, G, D, K = shape[:4]
    c = _case(shape)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    hT = t(c["hT"]).requires_grad_(True)
    gW, gb, tW, tb = (t(c[n]).requires_grad_(True) for n in ("gW", "gb", "tW", "tb"))
    outs, nums, abss, mss, total = [], [], [], [], 0.0
    for k in range(K):
        gate = torch.sigmoid(torch.cat([hT, t(c["h0"])], dim=-1).matmul(gW[k]) + gb[k])
        gated = gate * (hT.matmul(tW[k]) + tb[k])
        if c["nm"] is not None:
            gated = gated * t(c["nm"])[:, None]
        out = torch.zeros(G, 1, dtype=torch.float64).index_add_(0, torch.from_numpy(c["gnl"]).long(), gated)[:, 0]
        diff = (out - t(c["y"][k])) * t(c["m"][k])
        num, ab, ms = (0.5 * diff * diff).sum(), diff.abs().sum(), t(c["m"][k]).sum()
        total = total + c["a"][k] * num + c["b"][k] * ab + (out * t(c["w"][k])).sum()
        outs.append(out.detach()); nums.append(float(num)); abss.append(float(ab)); mss.append(float(ms))
    total.backward()
    grads = tuple(x.grad.numpy() for x in (hT, gW, gb, tW, tb))
    return torch.stack(outs).numpy(), np.array(nums), np.array(abss), np.array(mss), grads


def _device_inputs(shape, cuda, use_ptr=True):
    c = _case(shape)
    K = shape[3]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    leaves = {"hT": dev(c["hT"]).requires_grad_(True)}
    for n in ("gW", "gb", "tW", "tb"):
        leaves[n] = [dev(c[n][k]).requires_grad_(True) for k in range(K)]
    fixed = {"h0": dev(c["h0"]), "gnl": dev(c["gnl"]), "gptr": dev(c["gptr"]) if use_ptr else None, "nm": dev(c["nm"]),
             "y": dev(c["y"]), "m": dev(c["m"]), "w": dev(c["w"]),
             "a": torch.from_numpy(c["a"].astype(np.float32)).to(cuda), "b": torch.from_numpy(c["b"].astype(np.float32)).to(cuda)}
    return leaves, fixed


def _collect(shape, leaves, out, num, ab, ms):
    K = shape[3]
    n = lambda t: t.detach().cpu().numpy()
    g = lambda ts, shp: np.stack([n(t.grad) for t in ts]).reshape(shp)
    D = shape[2]
    return (n(out), n(num), n(ab), n(ms),
            (n(leaves["hT"].grad), g(leaves["gW"], (K, 2 * D, 1)), g(leaves["gb"], (K, 1)), g(leaves["tW"], (K, D, 1)),
             g(leaves["tb"], (K, 1))))


def _run_multi(pkg, shape, cuda, use_ptr=True):
    ag = import_module(pkg.__name__ + ".autograd")
    G = shape[1]
    leaves, f = _device_inputs(shape, cuda, use_ptr)
    out, num, ab, ms = ag.readout_loss_multi(leaves["hT"], f["h0"], f["gnl"], f["gptr"], f["nm"], G, leaves["gW"], leaves["gb"],
                                             leaves["tW"], leaves["tb"], f["y"], f["m"])
    ((f["a"] * num).sum() + (f["b"] * ab).sum() + (out * f["w"]).sum()).backward()
    return _collect(shape, leaves, out, num, ab, ms)


def _run_per_task(pkg, shape, cuda, use_ptr=True):
    ag = import_module(pkg.__name__ + ".autograd")
    G, K = shape[1], shape[3]
    leaves, f = _device_inputs(shape, cuda, use_ptr)
    res = [ag.readout_loss(leaves["hT"], f["h0"], f["gnl"], f["gptr"], f["nm"], G, leaves["gW"][k], leaves["gb"][k], leaves["tW"][k],
                           leaves["tb"][k], f["y"][k].contiguous(), f["m"][k].contiguous()) for k in range(K)]
    out, num, ab, ms = (torch.stack([r[i] for r in res]) for i in range(4))
    ((f["a"] * num).sum() + (f["b"] * ab).sum() + (out * f["w"]).sum()).backward()
    return _collect(shape, leaves, out, num, ab, ms)


def _assert_within_bounds(got, want, what):
    """test_gpu_readout's bounds: out atol 2e-5 rtol 1e-5; num, ab 1e-5 max(1, |ref|); ms exact; gradients atol 2e-5 max(1, max|ref|),
    rtol 1e-4."""
    out, num, ab, ms, grads = got
    r_out, r_num, r_ab, r_ms, r_grads = want
    np.testing.assert_allclose(out, r_out, atol=2e-5, rtol=1e-5, err_msg=what)
    assert (np.abs(num - r_num) <= 1e-5 * np.maximum(1.0, np.abs(r_num))).all(), (what, num, r_num)
    assert (np.abs(ab - r_ab) <= 1e-5 * np.maximum(1.0, np.abs(r_ab))).all(), (what, ab, r_ab)
    assert (ms == r_ms).all(), what
    for n, a, ref in zip(NAMES, grads, r_grads):
        scale = max(1.0, float(np.abs(ref).max())) if ref.size else 1.0
        np.testing.assert_allclose(a, ref, atol=2e-5 * scale, rtol=1e-4, err_msg="%s %s" % (what, n))


def _same_bits(a, b):
    flat = lambda r: list(r[:4]) + list(r[4])
    return all(np.array_equal(x, y) for x, y in zip(flat(a), flat(b)))


@pytest.mark.parametrize("use_ptr", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_float64_and_deterministic(pkg, cuda, shape, use_ptr):
    assert pkg.ops.readout_multi_supported(shape[2], shape[3])
    got = _run_multi(pkg, shape, cuda, use_ptr)
    want = _reference(shape)
    V, G, D, K = shape[:4]
    assert got[0].shape == (K, G) and got[1].shape == got[2].shape == got[3].shape == (K,)
    _assert_within_bounds(got, want, "multi")
    if K >= 2:
        assert got[3][K // 2] == 0.0 and got[1][K // 2] == 0.0          # the task whose mask is all zero
    if V == 0:
        c = _case(shape)
        assert not got[0].any() and np.allclose(got[1], (0.5 * (c["y"] * c["m"]) ** 2).sum(1), rtol=1e-6)
        assert all(not g.any() for g in got[4])
    else:
        assert all(g.any() for g in got[4])
    assert _same_bits(got, _run_multi(pkg, shape, cuda, use_ptr))           # two evaluations agree bit for bit


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_the_per_task_kernels(pkg, cuda, shape):
    """The K per-task calls on the same inputs: ms equal exactly; for every other output the multi route's error against float64 is
    at most twice the per-task route's plus one f32 epsilon of that output's scale (max |ref|).

    Measured on an MI355X, worst multi error / per-task error over the shapes: out 1.16 (D = 256; bit-identical at D <= 128, where the
    forward sums run in the per-task kernel's order), num 1.19, ab 1.00, d_hT 1.08, d_gate_W 1.38, d_gate_b 1.00, d_transform_W 1.10,
    d_transform_b 1.00.  With the block's loss sums added sequentially instead of by the pairwise tree, ab missed the
    rule at G = 64 with 2.32."""
    multi, task, want = _run_multi(pkg, shape, cuda), _run_per_task(pkg, shape, cuda), _reference(shape)
    _assert_within_bounds(task, want, "per-task")
    assert np.array_equal(multi[3], task[3])
    eps = float(np.finfo(np.float32).eps)
    flat = lambda r: [("out", r[0]), ("num", r[1]), ("ab", r[2])] + list(zip(NAMES, r[4]))
    worst = []
    for (n, a), (_, b), (_, ref) in zip(flat(multi), flat(task), flat(want)):
        if not ref.size:
            continue
        em, et = float(np.abs(a - ref).max()), float(np.abs(b - ref).max())
        scale = float(np.abs(ref).max())
        print("%-14s multi %.3e  per-task %.3e  scale %.3e  ratio %.2f" % (n, em, et, scale, em / max(et, eps * scale, 1e-300)))
        worst.append((n, em, et, scale))
    bad = [(n, em, et) for n, em, et, scale in worst if em > 2 * et + eps * scale]
    assert not bad, bad


def test_outputs_of_a_task_do_not_depend_on_K(pkg, cuda):
    """K = 13, then K = 5 on its first five tasks: out, the three sums and the weight and bias gradients of those five agree bit for
    bit (d_hT is the sum over the tasks present and differs by definition)."""
    shape = SHAPES[2]
    assert shape[3] == 13
    ag = import_module(pkg.__name__ + ".autograd")
    G = shape[1]
    res = {}
    for K in (13, 5):
        leaves, f = _device_inputs(shape, cuda)
        out, num, ab, ms = ag.readout_loss_multi(leaves["hT"], f["h0"], f["gnl"], f["gptr"], f["nm"], G, leaves["gW"][:K], leaves["gb"][:K],
                                                 leaves["tW"][:K], leaves["tb"][:K], f["y"][:K].contiguous(), f["m"][:K].contiguous())
        ((f["a"][:K] * num).sum() + (f["b"][:K] * ab).sum() + (out * f["w"][:K]).sum()).backward()
        res[K] = [out[:5], num[:5], ab[:5], ms[:5]] + [leaves[n][k].grad for n in ("gW", "gb", "tW", "tb") for k in range(5)]
        assert leaves["gW"][K - 1].grad is not None and (K == 13 or leaves["gW"][5].grad is None)
    assert len(res[13]) == len(res[5]) == 24
    for a, b in zip(res[13], res[5]):
        assert torch.equal(a, b)


def test_accumulate_adds_to_d_hT(pkg, cuda):
    """ops.readout_multi_bwd with a non-zero d_last_h: exactly base + the fresh gradient (one f32 add per element), the weight
    gradients unchanged; the fresh gradient within the float64 bound."""
    shape = SHAPES[1]
    V, G, D, K = shape[:4]
    ops = pkg.ops
    leaves, f = _device_inputs(shape, cuda)
    flat = lambda n: [t.detach().reshape(-1).contiguous() for t in leaves[n]]
    hT = leaves["hT"].detach()
    out, node_gv, stats = ops.readout_multi_fwd(hT, f["h0"], f["gnl"], f["gptr"], None, G, flat("gW"), flat("gb"), flat("tW"), flat("tb"),
                                                f["y"], f["m"])
    assert tuple(node_gv.shape) == (V, 2 * K) and tuple(stats.shape) == (K, 3)
    d_stats = torch.stack([f["a"], f["b"]], dim=1).contiguous()
    args = (hT, f["h0"], f["gnl"], None, G, flat("gW"), flat("tW"), node_gv, out, f["y"], f["m"], f["w"], d_stats)
    fresh = ops.readout_multi_bwd(*args)
    np.testing.assert_allclose(fresh[0].cpu().numpy(), _reference(shape)[4][0], atol=2e-5, rtol=1e-4)
    base = torch.from_numpy(np.random.default_rng(3).normal(0, 1, (V, D)).astype(np.float32)).to(cuda)
    acc = ops.readout_multi_bwd(*args, d_last_h=base.clone())
    assert torch.equal(acc[0], base + fresh[0]) and not torch.equal(acc[0], fresh[0])
    for a, b in zip(acc[1:], fresh[1:]):
        assert torch.equal(a, b)


def test_unsupported_shapes_take_the_per_task_loop(pkg, cuda):
    """autograd.readout_loss_multi outside ops.readout_multi_supported(D, K) returns what the per-task loop returns: K = 17 (more
    than 16 tasks) bit for bit, since it IS the loop.  D = 84 -- a width the models run zero-padded to 100, but a multiple of 4 that
    the multi-task kernels take as it is -- agrees with the loop within the float64 bounds."""
    assert not pkg.ops.readout_multi_supported(100, 17) and not pkg.ops.readout_multi_supported(30, 2)
    s17 = (300, 11, 100, 17, False, False)
    a, b = _run_multi(pkg, s17, cuda), _run_per_task(pkg, s17, cuda)
    assert a[0].shape == (17, 11) and _same_bits(a, b)
    _assert_within_bounds(a, _reference(s17), "K=17")
    s84 = (300, 11, 84, 3, False, False)
    _assert_within_bounds(_run_multi(pkg, s84, cuda), _reference(s84), "D=84 multi")
    _assert_within_bounds(_run_per_task(pkg, s84, cuda), _reference(s84), "D=84 per-task")


_FIRST_CALL_SCRIPT = """
import importlib, sys
import numpy as np, torch
pkg = importlib.import_module(sys.argv[1])
ops = pkg.ops
dev = torch.device("cuda:0")
rng = np.random.default_rng(5)
V, G, D = 300, 7, 256
t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
gnl = torch.from_numpy(np.sort(rng.integers(0, G, V)).astype(np.int32)).to(dev)
hT, h0 = t(rng.uniform(-1, 1, (V, D))), t(rng.uniform(-1, 1, (V, D)))
gW = [t(rng.uniform(-0.3, 0.3, 2 * D)) for _ in range(16)]; tW = [t(rng.uniform(-0.3, 0.3, D)) for _ in range(16)]
gb = [t(rng.uniform(-0.2, 0.2, 1)) for _ in range(16)]; tb = [t(rng.uniform(-0.2, 0.2, 1)) for _ in range(16)]
y, m = t(rng.normal(0, 1, (16, G))), t(rng.random((16, G)) < 0.8)
ds = t(np.tile([[0.5, 0.25]], (16, 1)))
res = {}
for K in (5, 16):                                      # the SMALL dynamic-LDS request first, then the largest
    out, gv, stats = ops.readout_multi_fwd(hT, h0, gnl, None, None, G, gW[:K], gb[:K], tW[:K], tb[:K], y[:K].contiguous(), m[:K].contiguous())
    grads = ops.readout_multi_bwd(hT, h0, gnl, None, G, gW[:K], tW[:K], gv, out, y[:K].contiguous(), m[:K].contiguous(), None, ds[:K].contiguous())
    torch.cuda.synchronize()
    res[K] = [out[:5], stats[:5]] + [g[:5] for g in grads[1:]]
    assert all(bool(torch.isfinite(x).all()) for x in res[K]) and bool(torch.isfinite(grads[0]).all()) and bool(grads[0].any())
assert all(torch.equal(a, b) for a, b in zip(res[5], res[16]))
print("FIRST_CALL_OK")
"""


def test_small_K_before_large_K_in_a_fresh_process(pkg, cuda):
    """The kernels' dynamic-LDS limit is raised once per process and device: a process whose FIRST D = 256 call has 5 tasks (50 KB in
    the backward) must still be able to launch 16 tasks (82 KB) afterwards.  Needs a process that has launched neither, hence the
    child; its first five tasks agree bit for bit between the two calls."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _FIRST_CALL_SCRIPT, pkg.__name__], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FIRST_CALL_OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_backward_without_graphs_zeroes_d_hT(pkg, cuda):
    """G == 0 with nodes present: ggnn_readout_multi_bwd_f32 itself writes d_hT = 0 (accumulate = 0) or leaves it (accumulate = 1),
    and the weight gradients are zero -- called through the C ABI, since ops.readout_multi_bwd hands it a zeroed buffer anyway."""
    import ctypes
    lib, ops = pkg._lib.load(), pkg.ops
    V, D, K = 37, 32, 3
    ones = lambda *shape: torch.ones(*shape, device=cuda)
    hT, gnl = ones(V, D), torch.zeros(V, dtype=torch.int32, device=cuda)
    W = [ones(2 * D) for _ in range(K)]
    ptrs = lambda ts: (ctypes.c_void_p * K)(*[t.data_ptr() for t in ts])
    grads = [[ones(n) * 7 for _ in range(K)] for n in (2 * D, 1, D, 1)]
    ws_bytes = lib.ggnn_readout_multi_workspace_bytes(V, D, K, 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=cuda)
    for accumulate in (0, 1):
        d_hT = ones(V, D) * 3
        pkg._lib.check(lib.ggnn_readout_multi_bwd_f32(
            hT.data_ptr(), hT.data_ptr(), gnl.data_ptr(), None, ptrs(W), ptrs(W), hT.data_ptr(), None, None, None, None, None,
            d_hT.data_ptr(), accumulate, ptrs(grads[0]), ptrs(grads[1]), ptrs(grads[2]), ptrs(grads[3]), ws.data_ptr(), ws_bytes,
            V, D, K, 0, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert bool((d_hT == (3.0 if accumulate else 0.0)).all())
        assert all(not bool(g.any()) for gs in grads for g in gs)
