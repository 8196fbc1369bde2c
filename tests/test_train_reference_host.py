"""CPU check of the checker: the float64 autograd gradients of tests/train_reference.py (the reference the training-gradient GPU
tests hold the package to) against central finite differences of the same oracle loss, on a tiny batch with two tasks, a task
loss factor, edge-weight dropout and readout-weight dropout."""
import numpy as np
import pytest
import torch

import train_reference as tr


def _tiny_batch(oracle, rng, D, T, use_edge_bias):
    sizes = [5, 7, 4, 8]                                           # 24 nodes in 4 graphs
    V, G = sum(sizes), len(sizes)
    gnl = np.repeat(np.arange(G), sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    adj = [[] for _ in range(T)]
    for g, (s, n) in enumerate(zip(starts, sizes)):
        for i in range(1, n):                                       # a tree plus one ring bond per graph, both directions
            j = int(rng.integers(0, i))
            t = int(rng.integers(0, T))
            adj[t] += [(s + i, s + j), (s + j, s + i)]
        adj[int(rng.integers(0, T))] += [(s, s + n - 1)]
    adj = [torch.tensor(np.asarray(a, np.int32).reshape(-1, 2)) for a in adj]
    nin = np.zeros((V, T), np.float32)
    for t, a in enumerate(adj):
        np.add.at(nin[:, t], a[:, 1].numpy(), 1.0)
    targets = rng.normal(size=(2, G)).astype(np.float32)
    tmask = np.ones((2, G), np.float32); tmask[1, 2] = 0
    feed = {"initial_node_representation": torch.from_numpy(rng.uniform(-1, 1, (V, D)).astype(np.float32)),
            "adjacency_lists": adj, "num_incoming_edges_per_type": torch.from_numpy(nin),
            "graph_nodes_list": torch.from_numpy(gnl), "num_graphs": G,
            "target_values": torch.from_numpy(targets * tmask), "target_mask": torch.from_numpy(tmask)}
    params = {"hidden_size": D, "layer_timesteps": [1, 2], "residual_connections": {"1": [0]}, "use_edge_bias": use_edge_bias,
              "use_edge_msg_avg_aggregation": not use_edge_bias, "graph_rnn_activation": "tanh", "graph_rnn_cell": "GRU",
              "task_ids": [0, 1], "task_sample_ratios": {1: 0.25}}
    layers = oracle.make_sparse_layers(rng, params, T, random_bias=True)
    readouts = {t: (oracle.glorot_init(rng, [2 * D, 1]), rng.normal(0, 0.1, 1).astype(np.float32),
                    oracle.glorot_init(rng, [D, 1]), rng.normal(0, 0.1, 1).astype(np.float32)) for t in (0, 1)}
    keep = 0.7
    m01 = lambda shape, seed: (oracle.counter_dropout(np.ones(shape, np.float32), keep, seed) != 0).astype(np.float64)
    masks = {"edge_keep": keep, "edge": [m01((T * D, D), 11 + l) for l in range(2)], "readout_keep": keep,
             "readout": {(k, t): m01((2 * D if k == "regression_gate" else D, 1), 100 + 10 * t + i)
                         for t in (0, 1) for i, k in enumerate(("regression_gate", "regression_transform"))}}
    return params, layers, readouts, feed, masks


@pytest.mark.parametrize("use_edge_bias", [False, True], ids=["mean-aggregation", "edge-bias-sum"])
def test_oracle_gradients_equal_central_differences(oracle, oracle_torch, use_edge_bias):
    rng = np.random.default_rng(3)
    D, T = 4, 2
    params, layers, readouts, feed, masks = _tiny_batch(oracle, rng, D, T, use_edge_bias)
    for m in masks["edge"]:
        assert 0 < m.mean() < 1
    loss, leaves = tr.oracle_loss_from_weights(oracle_torch, params, layers, readouts, feed, masks)
    loss.backward()
    names = set(leaves)
    assert sum("/gnn_edge_weights_" in n for n in names) == 2 and sum("MLP_W_layer0" in n for n in names) == 4
    assert any(n.startswith("out_layer_task1/") for n in names)
    assert use_edge_bias == any("/gnn_edge_biases_" in n for n in names)
    eps = 1e-6
    for name, leaf in leaves.items():
        grad = leaf.grad.clone()
        fd = torch.zeros_like(grad)
        flat = leaf.detach().view(-1)
        with torch.no_grad():
            for i in range(flat.numel()):
                x0 = float(flat[i])
                out = []
                for x in (x0 + eps, x0 - eps):
                    flat[i] = x
                    out.append(float(_loss_with(oracle_torch, params, layers, readouts, feed, masks, leaves)))
                flat[i] = x0
                fd.view(-1)[i] = (out[0] - out[1]) / (2 * eps)
        scale = float(grad.abs().max())
        assert scale > 0, name
        np.testing.assert_allclose(grad.numpy(), fd.numpy(), rtol=0, atol=1e-6 * max(scale, 1.0), err_msg=name)
        if "/gnn_edge_weights_" in name:                               # the chain rule through the mask: dropped entries get 0
            l = int(name.split("_")[-1].split(":")[0])
            assert (grad.numpy()[masks["edge"][l] == 0] == 0).all()
        if "MLP_W_layer0" in name:
            kind = "regression_gate" if "/regression_gate/" in name else "regression_transform"
            assert (grad.numpy()[masks["readout"][(kind, int(name[len("out_layer_task")]))] == 0] == 0).all()


def _loss_with(oracle_torch, params, layers, readouts, feed, masks, leaves):
    """The oracle loss at the current values of `leaves` (perturbed in place by the caller)."""
    T, D = len(feed["adjacency_lists"]), params["hidden_size"]
    cur = lambda name: leaves[name].detach().numpy()
    lay = []
    for l, L in enumerate(layers):
        scope = "graph_model/gnn_layer_%i" % l
        base = scope + "/timestep_0/gru_cell"
        n = dict(L, edge_weights=cur("%s/gnn_edge_weights_%i:0" % (scope, l)).reshape(T, D, D), Wg=cur(base + "/gates/kernel:0"),
                 bg=cur(base + "/gates/bias:0"), Wc=cur(base + "/candidate/kernel:0"), bc=cur(base + "/candidate/bias:0"))
        if params["use_edge_bias"]:
            n["edge_biases"] = cur("%s/gnn_edge_biases_%i:0" % (scope, l))
        lay.append(n)
    ro = {t: tuple(cur("out_layer_task%i/%s:0" % (t, k)) for k in ("regression_gate/MLP_W_layer0", "regression_gate/MLP_b_layer0",
                                                                      "regression/MLP_W_layer0", "regression/MLP_b_layer0"))
          for t in params["task_ids"]}
    return tr.oracle_loss_from_weights(oracle_torch, params, lay, ro, feed, masks)[0]


def test_task_factor_and_masks_enter_the_loss(oracle, oracle_torch):
    """The 1/ratio factor of chem_tensorflow.py:168 multiplies the second task's loss, and the masks change the loss."""
    rng = np.random.default_rng(5)
    params, layers, readouts, feed, masks = _tiny_batch(oracle, rng, 4, 2, False)
    base, _ = tr.oracle_loss_from_weights(oracle_torch, params, layers, readouts, feed, masks)
    one = dict(params, task_sample_ratios={})
    plain, _ = tr.oracle_loss_from_weights(oracle_torch, one, layers, readouts, feed, masks)
    only0, _ = tr.oracle_loss_from_weights(oracle_torch, dict(one, task_ids=[0]), layers, readouts,
                                           dict(feed, target_values=feed["target_values"][:1], target_mask=feed["target_mask"][:1]), masks)
    base, plain, only0 = (float(x.detach()) for x in (base, plain, only0))
    t1 = plain - only0
    assert t1 > 0 and abs(base - (only0 + 4 * t1)) <= 1e-12 * base
    nomask, _ = tr.oracle_loss_from_weights(oracle_torch, params, layers, readouts, feed, None)
    assert abs(float(nomask.detach()) - base) > 1e-6
