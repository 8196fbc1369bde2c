"""Sparse GCN (chem_tensorflow_gcn.py) on the host: the model's variables and seeded init, the minibatch rule, argument
validation of the new C entry points, and the fp64 restatement of the forward / backward pass against torch.autograd.
The packer is pinned against the reference's own run in test_gcn_reference_golden.py.  No GPU needed."""
import numpy as np
import pytest
import torch

import gcn_reference_math as ref


def _molecules(pkg, graphs):
    """MoleculeSet from [(num_nodes, bonds [(src, type, dst)])]."""
    raw = [{"targets": [[0.5], [1.5]], "graph": [list(b) for b in bonds], "node_features": [[1, 0, 0, 0, 0]] * n}
           for n, bonds in graphs]
    return pkg.MoleculeSet.from_json(raw)


def _model(pkg, ms, **config):
    params = {"hidden_size": 32, "num_timesteps": 3, "random_seed": 7}
    params.update(config)
    return pkg.SparseGCNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms, "--config": params})


def test_variables_and_seeded_init(pkg):
    from importlib import import_module
    ms = pkg.synthetic_qm9(40, seed=2)
    m = _model(pkg, ms, gcn_use_bias=True)
    names = list(m.graph_model_variables())
    assert names == ["graph_model/gcn_scope/gcn_weights_%i:0" % i for i in range(3)] + ["graph_model/gcn_scope/gcn_bias_%i:0" % i for i in range(3)]
    for n, t in m.graph_model_variables().items():
        assert tuple(t.shape) == ((32, 32) if "weights" in n else (32,))
    # the reference's creation order from the NumPy stream: training-set shuffle, then the layer weights (biases are zeros)
    np.random.seed(7)
    np.random.permutation(ms.num_graphs)
    utils = import_module(pkg.__name__ + ".utils")
    for i in range(3):
        np.testing.assert_array_equal(m.weights['edge_weights'][i].numpy(), utils.glorot_init((32, 32)))
        assert not m.weights['edge_biases'][i].any()
    assert "graph_model/gcn_scope/gcn_bias_0:0" not in _model(pkg, ms).graph_model_variables()
    frozen = pkg.SparseGCNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms,
                                     "--freeze-graph-model": True, "--config": {"hidden_size": 32}})
    assert not any(k.startswith("graph_model/") for k in frozen.trainable_variables)
    with pytest.raises(ValueError):
        _model(pkg, ms, hidden_size=30)


def test_minibatches_follow_reference_rule(pkg):
    ms = _molecules(pkg, [(3, [(0, 1, 1)]), (4, [(0, 1, 2), (2, 3, 1)]), (2, []), (5, [(1, 4, 1)])])
    m = _model(pkg, ms, batch_size=10)
    batches = list(m.make_minibatch_iterator(m.valid_data, is_training=False))
    # 3 + 4 = 7 < 10, 7 + 2 = 9 < 10, 9 + 5 >= 10  ->  [3, 4, 2], [5];  a graph that exactly hits batch_size starts a new batch
    assert [b['num_graphs'] for b in batches] == [3, 1]
    b = batches[0]
    entry_ptr, adj, w = pkg.gcn_model.gcn_adjacency(m.valid_data["molecules"])
    np.testing.assert_array_equal(b['adjacency_list'][:entry_ptr[1]], adj[:entry_ptr[1]])
    np.testing.assert_array_equal(b['adjacency_list'][entry_ptr[1]:entry_ptr[2]], adj[entry_ptr[1]:entry_ptr[2]] + 3)
    assert b['adjacency_weights'].dtype == np.float32
    np.testing.assert_array_equal(b['graph_nodes_list'].numpy(), [0, 0, 0, 1, 1, 1, 1, 2, 2])
    g = b['gcn_graph']
    np.testing.assert_array_equal(g.row_ptr.numpy(), np.searchsorted(b['adjacency_list'][:, 0], np.arange(10)))
    assert b['initial_node_representation'].shape == (9, 32)
    m2 = _model(pkg, ms, batch_size=9)
    assert [b['num_graphs'] for b in m2.make_minibatch_iterator(m2.valid_data, is_training=False)] == [2, 2]


def test_task_sample_ratios_mask_training_labels(pkg):
    ms = pkg.synthetic_qm9(20, seed=3)
    m = _model(pkg, ms, task_ids=[0, 1], task_sample_ratios={"1": 0.25})
    mask = m.train_data["label_mask"]
    assert mask[:, 0].all() and mask[:5, 1].all() and not mask[5:, 1].any()


def test_transposed_csr(pkg):
    rng = np.random.default_rng(0)
    V = 30
    adj = rng.integers(0, V, (200, 2))
    adj = adj[np.lexsort((adj[:, 1], adj[:, 0]))]
    w = rng.standard_normal(200).astype(np.float32)
    rp, c, v, rpt, ct, vt = pkg.ops.gcn_csr_host(adj, w, V)
    x = rng.standard_normal((V, 4))
    dense = np.zeros((V, V))
    np.add.at(dense, (adj[:, 0], adj[:, 1]), w.astype(np.float64))
    for ptr, col, val, M in ((rp, c, v, dense), (rpt, ct, vt, dense.T)):
        got = np.zeros((V, 4))
        for i in range(V):
            for k in range(ptr[i], ptr[i + 1]):
                got[i] += val[k] * x[col[k]]
        np.testing.assert_allclose(got, M @ x, atol=1e-12)
    for i in range(V):                                        # transposed rows keep the source rows in ascending order
        assert (np.diff(adj[:, 0][np.flatnonzero(adj[:, 1] == i)]) >= 0).all()
        assert (np.diff(ct[rpt[i]:rpt[i + 1]]) >= 0).all()
    with pytest.raises(IndexError):
        pkg.ops.gcn_csr_host(np.array([[0, V]]), np.ones(1), V)


def test_gcn_entry_points_validate_without_gpu(pkg):
    lib = pkg._lib.load()
    fake = 16
    assert [lib.ggnn_gcn_fused_supported(d) for d in (32, 48, 64, 100, 128)] == [1, 0, 1, 1, 0]
    assert lib.ggnn_gcn_image_bytes(48) == 0 and lib.ggnn_gcn_image_bytes(100) > 0
    layer = lambda x, V, D, keep=1.0: lib.ggnn_gcn_layer_f32(x, fake, fake, fake, 4, fake, None, 1, None, 0, 0, keep, 32, None, V, D, None)
    assert layer(None, 5, 64) == -1                       # null pointer
    assert layer(fake, 5, 48) == -2                       # no fused kernel for 48
    assert layer(None, 0, 64) == 0                        # V == 0: nothing to do
    assert layer(fake, 5, 64, keep=0.0) == -1             # keep_prob outside (0, 1]
    assert layer(fake, -1, 64) == -1
    assert lib.ggnn_gcn_pack_weights_f32(None, 64, 0, fake, None) == -1
    assert lib.ggnn_gcn_pack_weights_f32(fake, 48, 0, fake, None) == -2
    assert lib.ggnn_gcn_epilogue_f32(None, None, 1, None, 0, 0, 1.0, fake, 5, 64, None) == -1
    assert lib.ggnn_gcn_epilogue_f32(fake, None, 1, None, 0, 0, 1.0, fake, 5, 30, None) == -1
    assert lib.ggnn_gcn_epilogue_f32(None, None, 1, None, 0, 0, 1.0, None, 0, 64, None) == 0
    W = (pkg.ops.ctypes.c_void_p * 2)(fake, fake)
    prop = lambda h0, V, D, ws_bytes: lib.ggnn_gcn_propagate_f32(h0, V, D, 2, fake, fake, fake, 4, W, None, 32, fake, ws_bytes, None)
    assert prop(None, 5, 64, 1 << 30) == -1
    assert prop(fake, 5, 48, 1 << 30) == -2
    assert prop(None, 0, 64, 0) == 0
    assert prop(fake, 5, 64, 16) == -3                    # workspace too small
    assert lib.ggnn_gcn_workspace_bytes(1000, 100, 4) >= 4 * lib.ggnn_gcn_image_bytes(100) + 2 * 1000 * 100 * 4
    assert b"GCN" in lib.ggnn_last_error() or b"workspace" in lib.ggnn_last_error()


def test_reference_math_against_autograd():
    """The fp64 restatement's forward and backward against torch.autograd on CPU: asymmetric A_hat with duplicates, negative
    weights and an empty row, bias, a dropout mask on the hidden layers."""
    rng = np.random.default_rng(1)
    V, D, L = 23, 8, 3
    adj = rng.integers(0, V - 1, (70, 2))                 # (node V-1 has no entries: an empty row and column)
    adj = np.concatenate([adj, adj[:5]])                  # duplicate (i, j) entries
    w = rng.standard_normal(len(adj))
    h0 = rng.standard_normal((V, D))
    Ws = [rng.standard_normal((D, D)) * 0.5 for _ in range(L)]
    bs = [rng.standard_normal(D) * 0.1 for _ in range(L)]
    masks = [(rng.random((V, D)) < 0.7) / 0.7 for _ in range(L - 1)] + [None]
    final, saved = ref.forward(h0, adj, w, Ws, bs, masks)
    d_final = rng.standard_normal((V, D))
    dWs, dbs = ref.backward(adj, w, Ws, saved, d_final, masks)

    A = torch.zeros((V, V), dtype=torch.float64)
    A.index_put_((torch.from_numpy(adj[:, 0]), torch.from_numpy(adj[:, 1])), torch.from_numpy(w), accumulate=True)
    tW = [torch.tensor(x, requires_grad=True) for x in Ws]
    tb = [torch.tensor(x, requires_grad=True) for x in bs]
    h = torch.from_numpy(h0)
    for l in range(L):
        h = A @ h @ tW[l] + tb[l]
        if l < L - 1:
            h = torch.relu(h) * torch.from_numpy(masks[l])
    np.testing.assert_allclose(final, h.detach().numpy(), rtol=1e-12, atol=1e-12)
    (h * torch.from_numpy(d_final)).sum().backward()
    for l in range(L):
        np.testing.assert_allclose(dWs[l], tW[l].grad.numpy(), rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(dbs[l], tb[l].grad.numpy(), rtol=1e-10, atol=1e-10)


def test_native_step_is_not_taken_by_gcn(pkg):
    ms = pkg.synthetic_qm9(10, seed=1)
    m = _model(pkg, ms)
    assert pkg.train_native.model_eligible(m) is False
