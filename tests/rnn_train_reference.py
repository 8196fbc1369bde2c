"""float64 reference gradients of the sparse model's training step with the BasicRNNCell (graph_rnn_cell = RNN,
chem_tensorflow_sparse.py:109-110): train_reference.oracle_loss_from_weights restated with the cell's kernel and bias as leaves.
A plain module (imported by the tests), not a conftest."""
import numpy as np
import torch

import train_reference as TR


def model_layers(model):
    """The model's graph weights in the oracle layout of an RNN-cell model (ggnn_oracle.make_sparse_layers: 'W', 'b')."""
    f = lambda t: t.detach().cpu().numpy()
    T, D = model.num_edge_types, model.params["hidden_size"]
    assert model.cell_type == "rnn" and not model.params["use_edge_bias"]
    return [{"edge_weights": f(model._edge_weight_vars[l]).reshape(T, D, D), "W": f(cell.kernel), "b": f(cell.bias)}
            for l, cell in enumerate(model.gnn_weights.rnn_cells)]


def oracle_loss_from_weights(oracle_torch, params, layers, readouts, feed, masks=None, device="cpu"):
    """-> (loss tensor, {variable name: leaf tensor}); the layout of train_reference.oracle_loss_from_weights, every layer with its
    'basic_rnn_cell' kernel and bias."""
    assert params.get("graph_rnn_cell", "GRU").lower() == "rnn" and not params.get("use_edge_bias", False)
    assert not params.get("use_propagation_attention", False)
    dev = torch.device(device)
    d64 = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a.detach()).to(dev, torch.float64)
    masks = masks or {"edge": None, "readout": None}
    leaves, tl = {}, []
    for l, L in enumerate(layers):
        scope = "graph_model/gnn_layer_%i" % l
        T, D = np.asarray(L["edge_weights"]).shape[0], np.asarray(L["edge_weights"]).shape[-1]
        ew = d64(L["edge_weights"]).reshape(T * D, D).requires_grad_(True)
        leaves["%s/gnn_edge_weights_%i:0" % (scope, l)] = ew
        W = ew if masks["edge"] is None else ew * d64(masks["edge"][l]) / masks["edge_keep"]      # :91
        cell = {"edge_weights": W.reshape(T, D, D)}
        base = "%s/timestep_0/basic_rnn_cell" % scope
        cell["W"] = leaves[base + "/kernel:0"] = d64(L["W"]).requires_grad_(True)
        cell["b"] = leaves[base + "/bias:0"] = d64(L["b"]).requires_grad_(True)
        tl.append(cell)
    h0 = d64(feed["initial_node_representation"])
    adj = [a.to(dev) for a in feed["adjacency_lists"]]
    last = oracle_torch.sparse_propagate(h0, adj, d64(feed["num_incoming_edges_per_type"]), tl, params)
    gnl = feed["graph_nodes_list"].to(dev)
    targets, tmask = d64(feed["target_values"]), d64(feed["target_mask"])
    loss = 0.0
    for internal_id, task_id in enumerate(params["task_ids"]):
        gW, gb, tW, tb = (d64(a).requires_grad_(True) for a in readouts[task_id])
        for name, leaf in zip(("regression_gate/MLP_W_layer0", "regression_gate/MLP_b_layer0", "regression/MLP_W_layer0",
                               "regression/MLP_b_layer0"), (gW, gb, tW, tb)):
            leaves["out_layer_task%i/%s:0" % (task_id, name)] = leaf
        if masks["readout"] is not None:                                                            # utils.py:68
            gW = gW * d64(masks["readout"][("regression_gate", task_id)]) / masks["readout_keep"]
            tW = tW * d64(masks["readout"][("regression_transform", task_id)]) / masks["readout_keep"]
        pred = oracle_torch.gated_regression(last, h0, gnl, int(feed["num_graphs"]), gW, gb, tW, tb)
        task_loss, _ = oracle_torch.task_loss(pred, targets[internal_id], tmask[internal_id])
        loss = loss + task_loss * (1.0 / (params["task_sample_ratios"].get(task_id) or 1.0))       # chem_tensorflow.py:168
    return loss, leaves


def oracle_loss_and_grads(oracle_torch, model, feed, masks=None, device="cpu"):
    """(loss, {variable name: d loss / d variable}) in float64 for the model's own weights."""
    loss, leaves = oracle_loss_from_weights(oracle_torch, model.params, model_layers(model), TR.readout_weights(model), feed, masks, device)
    loss.backward()
    return float(loss), {k: v.grad for k, v in leaves.items()}
