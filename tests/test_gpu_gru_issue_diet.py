"""The gather-fused GRU launch after its experiment switches became compile-time and its hot inference launches got instantiations of
their own (csrc/ggnn_gru_fused.hip: ticket source and gather parameters as template arguments, inference on the inference
instantiation): every launch still computes, BIT FOR BIT, what the unfused sequence ggnn_gather_segment_sum_f32 + ggnn_gru_packed_f32
computes -- on the specialised instantiations (T = 4, mean aggregation, hidden size 100) and on the generic one (T = 3, or plain sums),
with static and with counter-driven tickets, with and without the training stores.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 100
SMALL_V = (1, 15, 16, 17, 63, 65)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _sizes():
    # one full round of the four-wave form (two workgroups per CU, four 16-row tiles each) plus a thin tail
    full = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 4 * 16
    return SMALL_V + (full + 40,)


@functools.lru_cache(maxsize=None)
def _graph(V, T):
    """Adjacency lists [E_t, 2] and in-degree table [V, T]: ~2.5 random edges per node; node 0 receives nothing (in-degree 0: a zero
    row of the in-degree table, so the mean divides by 1e-7), node V - 1 receives five messages (one more than the gather pipelines)."""
    rng = np.random.default_rng(1000 * T + V)
    M = (5 * V) // 2
    types = rng.integers(0, T, M)
    src = rng.integers(0, V, M).astype(np.int32)
    dst = rng.integers(0, V, M).astype(np.int32)
    hub = V - 1
    keep = (dst != 0) & (dst != hub)
    types, src, dst = types[keep], src[keep], dst[keep]
    types = np.concatenate([types, np.arange(5) % T])
    src = np.concatenate([src, rng.integers(0, V, 5).astype(np.int32)])
    dst = np.concatenate([dst, np.full(5, hub, np.int32)])
    adj = [np.stack([src[types == t], dst[types == t]], axis=1).astype(np.int32).reshape(-1, 2) for t in range(T)]
    nin = np.zeros((V, T), np.float32)
    for t in range(T):
        np.add.at(nin[:, t], adj[t][:, 1], 1.0)
    assert nin[hub].sum() == 5 and (V == 1 or nin[0].sum() == 0)
    return adj, nin


@functools.lru_cache(maxsize=None)
def _inputs(V, T):
    """Device tensors shared by every case at (V, T); never written."""
    cuda = torch.device("cuda:0")
    rng = np.random.default_rng(77 * V + T)
    adj, nin = _graph(V, T)
    return dict(h=dev(rng.uniform(-1, 1, (V, D)).astype(np.float32), cuda),
                res=[dev(rng.uniform(-1, 1, (V, D)).astype(np.float32), cuda) for _ in range(2)],
                H=dev(rng.uniform(-1, 1, (V, T * D)).astype(np.float32), cuda),
                adj=[dev(a, cuda) for a in adj], nin=dev(nin, cuda))


@functools.lru_cache(maxsize=None)
def _weights(nx):
    cuda = torch.device("cuda:0")
    rng = np.random.default_rng(nx)
    K = (nx + 1) * D
    return (dev(rng.uniform(-0.2, 0.2, (K, 2 * D)).astype(np.float32), cuda), dev(rng.uniform(0.5, 1.5, 2 * D).astype(np.float32), cuda),
            dev(rng.uniform(-0.2, 0.2, (K, D)).astype(np.float32), cuda), dev(rng.uniform(-0.5, 0.5, D).astype(np.float32), cuda))


def _gru_fp64(xs, h, Wg, bg, Wc, bc, act):
    """chem_tensorflow_sparse.py:211-216 (TF-1.3 GRUCell) in fp64: returns h' and the candidate's operand [x | r*h]."""
    f = lambda t: t.double().cpu()
    x, h, Wg, bg, Wc, bc = torch.cat([f(t) for t in xs], 1), f(h), f(Wg), f(bg), f(Wc), f(bc)
    r, u = torch.sigmoid(torch.cat([x, h], 1) @ Wg + bg).split(D, dim=1)
    a = torch.cat([x, r * h], 1)
    c = a @ Wc + bc
    c = torch.tanh(c) if act == "tanh" else torch.relu(c)
    return u * h + (1 - u) * c, a, Wc


@pytest.mark.parametrize("save", [False, True], ids=["infer", "save"])
@pytest.mark.parametrize("T", [4, 3])
@pytest.mark.parametrize("use_avg", [1, 0])
@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("fmt", [2, 3], ids=["f16x2", "bf16x3"])
@pytest.mark.parametrize("nx", [1, 2, 3])
def test_gather_fused_gru_equals_unfused_sequence(pkg, cuda, nx, fmt, act, use_avg, T, save):
    Wg, bg, Wc, bc = _weights(nx)
    packed = pkg.ops.PackedWeights().gru(Wg, Wc, nx, D, fmt)
    for V in _sizes():
        i = _inputs(V, T)
        h, res, H = i["h"], i["res"][:nx - 1], i["H"]
        nin = i["nin"] if use_avg else None
        index = pkg.ops.build_message_index(i["adj"], V)
        incoming = pkg.ops.gather_segment_sum(H, index, nin, None, bool(use_avg))
        want_s = {} if save else None
        want = pkg.ops.gru_packed(res + [incoming], h, packed, bg, bc, activation=act, fmt=fmt, save=want_s)
        cnt = torch.zeros(1, dtype=torch.int32, device=cuda)
        for counter in (None, cnt):                                  # static tickets | a zeroed device counter
            got_s = {} if save else None
            got = pkg.ops.gru_packed_gather(res, h, packed, bg, bc, H.view(V * T, D), index, None, nin, activation=act,
                                            tile_counter=counter, save=got_s, fmt=fmt)
            assert torch.equal(got, want), (V, counter is not None)
            if save:
                for k in ("r", "u", "c"):
                    assert torch.equal(got_s[k], want_s[k]), (V, k)
                assert torch.equal(got_s["incoming"], incoming), V
        assert int(cnt[0]) > 0
        if V > 1:
            assert torch.all(incoming[0] == 0)                       # the node without incoming messages
        if fmt == 3 and act == "tanh" and use_avg and T == 4 and not save:
            # one case per nx against fp64.  The gathered segment against a numpy segment mean of the same rows (the tolerance of
            # test_gpu_parity.py::test_gather_segment_sum), so that the reference below does not lean on the kernel under test ...
            adj, nin64 = _graph(V, T)
            H64 = H.cpu().numpy().astype(np.float64).reshape(V, T, D)
            seg = np.zeros((V, D))
            for t in range(T):
                np.add.at(seg, adj[t][:, 1], H64[adj[t][:, 0], t])
            seg /= nin64.astype(np.float64).sum(-1, keepdims=True) + 1e-7
            np.testing.assert_allclose(incoming.cpu().numpy(), seg, atol=5e-6, rtol=1e-5)
            # ... and the GRU on it against the fp64 formula, at test_gpu_parity.py::test_gru's tolerance
            ref, a, Wc64 = _gru_fp64(res + [incoming], h, Wg, bg, Wc, bc, act)
            atol_c = max(3e-6, 4e-7 * float((a.abs() @ Wc64.abs()).max()))
            np.testing.assert_allclose(want.cpu().numpy(), ref.numpy(), atol=atol_c, rtol=1e-5)
            np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), atol=atol_c, rtol=1e-5)


@pytest.mark.parametrize("fmt", [2, 3], ids=["f16x2", "bf16x3"])
def test_forward_with_and_without_fused_gather(pkg, cuda, fmt):
    """ggnn_sparse_propagate_f32 on 300 nodes, layers of [2, 1, 1] steps, layer 2 with a residual input from the initial states: every
    layer's output with the gather fused into the GRU launches == the same call with fuse_gather = 0, exactly."""
    from conftest import random_graph_batch
    V, T = 300, 4
    steps, residuals = [2, 1, 1], [[], [], [0]]
    rng = np.random.default_rng(300)
    h, adj, nin = random_graph_batch(rng, V, 750, T, D, sorted_src=True)
    index = pkg.ops.build_message_index([dev(a, cuda) for a in adj], V)
    comp = pkg.ops.build_compact_sources(index)
    pw = pkg.ops.PackedWeights()
    edge_w, Wg, bg, Wc, bc, gru_packed, edge_packed = [], [], [], [], [], [], []
    for l in range(len(steps)):
        nx = len(residuals[l]) + 1
        edge_w.append(dev(rng.uniform(-0.3, 0.3, (T, D, D)).astype(np.float32), cuda))
        Wg.append(dev(rng.uniform(-0.2, 0.2, ((nx + 1) * D, 2 * D)).astype(np.float32), cuda))
        bg.append(dev(rng.uniform(-0.5, 1.0, 2 * D).astype(np.float32), cuda))
        Wc.append(dev(rng.uniform(-0.2, 0.2, ((nx + 1) * D, D)).astype(np.float32), cuda))
        bc.append(dev(rng.uniform(-0.5, 0.5, D).astype(np.float32), cuda))
        gru_packed.append(pw.gru(Wg[l], Wc[l], nx, D, fmt))
        edge_packed.append(pw.edge(edge_w[l], fmt))
    run = lambda fuse: pkg.ops.sparse_propagate(dev(h, cuda), index, comp, dev(nin, cuda), True, steps, residuals, edge_w, edge_packed,
                                                None, Wg, bg, Wc, bc, gru_packed, "tanh", fuse_gather=fuse,
                                                gru_fmt=[fmt] * len(steps), edge_fmt=[fmt] * len(steps))
    fused, unfused = run(True), run(False)
    assert len(fused) == len(steps)
    for l, (a, b) in enumerate(zip(fused, unfused)):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), l
