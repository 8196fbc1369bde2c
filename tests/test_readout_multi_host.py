"""Host-side checks of the multi-task readout (ggnn_readout_multi_*, params['multitask_readout']): the symbols, the supported set,
the workspace size, the argument checks (found before anything is launched, so no GPU is needed to observe them), and the config
key's absence from every default_params and its fall-back on a CPU device."""
import ctypes as c

import numpy as np
import pytest
import torch

KEY = "multitask_readout"


def test_symbols_supported_set_and_workspace(pkg):
    lib = pkg._lib.load()
    for name in ("ggnn_readout_multi_supported", "ggnn_readout_multi_workspace_bytes", "ggnn_readout_multi_fwd_f32",
                 "ggnn_readout_multi_bwd_f32"):
        assert name in pkg._lib.SYMBOLS and getattr(lib, name) is not None
    for D in (32, 64, 100):
        for K in (1, 13, 16):
            assert lib.ggnn_readout_multi_supported(D, K) == 1 and pkg.ops.readout_multi_supported(D, K)
    for D, K in ((100, 0), (100, 17), (0, 4), (30, 4), (-4, 1), (100, -1)):
        assert lib.ggnn_readout_multi_supported(D, K) == 0, (D, K)
    ws = lib.ggnn_readout_multi_workspace_bytes
    assert ws(0, 32, 1, 0) > 0 and ws(100000, 100, 16, 5500) > 0
    for lo, hi in (((10, 100, 4, 50), (5000, 100, 4, 50)), ((5000, 100, 4, 50), (100000, 100, 4, 50)),      # V
                   ((5000, 100, 1, 50), (5000, 100, 2, 50)), ((5000, 100, 2, 50), (5000, 100, 16, 50)),     # K
                   ((0, 100, 4, 1), (0, 100, 4, 100000)), ((16, 32, 1, 64), (16, 32, 1, 1 << 20))):         # G
        assert ws(*lo) <= ws(*hi), (lo, hi)
    assert ws(0, 100, 4, 100000) > ws(0, 100, 4, 1)


def test_argument_checks_need_no_launch(pkg):
    lib = pkg._lib.load()
    fake, K = 4096, 3
    arr = lambda *v: (c.c_void_p * len(v))(*v)
    W = arr(fake, fake, fake)
    big = 1 << 30

    def fwd(hT=fake, gW=W, K=K, D=64, V=5, G=2, ws_bytes=big, stats=fake, out=fake):
        return lib.ggnn_readout_multi_fwd_f32(hT, fake, fake, None, None, gW, W, W, W, fake, fake, out, fake, stats, fake, ws_bytes,
                                              V, D, K, G, None)

    def bwd(hT=fake, gW=W, dgW=W, K=K, D=64, V=5, G=2, ws_bytes=big, d_hT=fake):
        return lib.ggnn_readout_multi_bwd_f32(hT, fake, fake, None, gW, W, fake, fake, fake, fake, None, fake, d_hT, 0, dgW, W, W, W,
                                              fake, ws_bytes, V, D, K, G, None)

    for call in (fwd, bwd):
        assert call(hT=None) == -1 and lib.ggnn_last_error()                 # GGNN_E_INVALID: null pointer
        assert call(gW=None) == -1
        assert call(gW=arr(fake, None, fake)) == -1                           # one task's weight pointer is null
        assert b"task 1" in lib.ggnn_last_error()
        assert call(gW=arr(fake, fake + 4, fake)) == -1                       # misaligned weights
        assert call(hT=fake + 4) == -1
        assert call(V=-1) == -1
        assert call(K=17, gW=None) == -2                                      # GGNN_E_UNSUPPORTED, whatever else is wrong
        assert b"tasks" in lib.ggnn_last_error()
        assert call(K=0) != 0 and call(D=30) == -2 and call(D=260) == -2
        assert call(ws_bytes=1) == -3                                         # GGNN_E_WORKSPACE
        assert b"workspace" in lib.ggnn_last_error()
        assert call(ws_bytes=lib.ggnn_readout_multi_workspace_bytes(5, 64, K, 2) - 1) == -3
    assert fwd(out=None) == -1
    assert bwd(dgW=None) == -1 and bwd(dgW=arr(fake, fake, None)) == -1 and bwd(d_hT=None) == -1
    assert fwd(stats=None, ws_bytes=0, K=17) == -2


def test_key_is_in_no_default_params(pkg):
    for cls in (pkg.SparseGGNNChemModel, pkg.DenseGGNNChemModel, pkg.SparseGCNChemModel):
        assert KEY not in cls.default_params()


def _plain_gated_regression(self, last_h, regression_gate, regression_transform):
    """chem_tensorflow_sparse.py:220-231 / chem_tensorflow_dense.py:119-129 in plain torch: the package's MLP runs on its HIP GEMMs
    and has no CPU implementation, so a CPU forward_batch needs this stand-in for the model's own op-by-op gated_regression."""
    ph = self.placeholders
    h0 = ph['initial_node_representation']
    g, t = regression_gate.params, regression_transform.params
    gate = torch.sigmoid(torch.cat([last_h, h0], dim=-1).matmul(g["weights"][0]) + g["biases"][0])
    gated = gate * (last_h.matmul(t["weights"][0]) + t["biases"][0])
    if last_h.dim() == 3:
        out = (gated[..., 0] * ph['node_mask']).sum(dim=1)
    else:
        out = torch.zeros(int(ph['num_graphs']), 1).index_add_(0, ph['graph_nodes_list'].long(), gated)[:, 0]
    self.output = out
    return out


@pytest.mark.parametrize("cls", ["SparseGGNNChemModel", "DenseGGNNChemModel", "SparseGCNChemModel"])
def test_cpu_model_takes_the_per_task_loop(pkg, monkeypatch, cls):
    """On a CPU device the key changes nothing: forward_batch asks the multi-task method, gets None and runs the per-task loop -- the
    same loss bit for bit, the same per-task entries.  (use_graph = False, chem_tensorflow.py:147, and _plain_gated_regression: the
    propagation and the MLP have no CPU implementation; the task loop and the loss under test are the model's own.)"""
    ms = pkg.synthetic_qm9(24, mean_nodes=6, seed=3, num_tasks=3)
    monkeypatch.setattr(getattr(pkg, cls), "gated_regression", _plain_gated_regression)
    rng = np.random.default_rng(0)
    V, G, D = 40, 6, 32
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if cls.startswith("Dense"):
        feed = {"initial_node_representation": t(rng.uniform(-1, 1, (G, 7, D))), "node_mask": t(rng.random((G, 7)) < 0.8),
                "num_vertices": 7, "adjacency_matrix": None}
    else:
        feed = {"initial_node_representation": t(rng.uniform(-1, 1, (V, D))),
                "graph_nodes_list": torch.from_numpy(np.sort(rng.integers(0, G, V)).astype(np.int32))}
    feed.update({"num_graphs": G, "target_values": t(rng.normal(0, 1, (3, G))), "target_mask": t(rng.random((3, G)) < 0.8),
                 "out_layer_dropout_keep_prob": 1.0})
    results, asked = [], []
    for key in (False, True):
        cfg = {"task_ids": [0, 1, 2], "hidden_size": D, "random_seed": 4, "use_graph": False}
        if key:
            cfg[KEY] = True
        m = getattr(pkg, cls)({"--quiet": True, "--device": "cpu", "train_data": None, "valid_data": ms, "--config": cfg})
        assert bool(m.params.get(KEY)) == key
        multi = m.gated_regression_with_loss_multi
        monkeypatch.setattr(m, "gated_regression_with_loss_multi", lambda final: asked.append(key) or multi(final), raising=False)
        with torch.no_grad():
            loss = m.forward_batch(dict(feed))
        assert len(m.ops["losses"]) == 3 and np.isfinite(float(loss)) and float(loss) > 0
        results.append((float(loss), [float(m.ops["accuracy_task%i" % k]) for k in (0, 1, 2)], m.output.clone()))
    assert asked == [True]                                        # consulted only under the key -- and it declined
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1] and torch.equal(results[0][2], results[1][2])
