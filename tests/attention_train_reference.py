"""float64 reference gradients of the sparse model's training step WITH propagation attention (chem_tensorflow_sparse.py:147-149,
170-196): train_reference.oracle_loss_from_weights restated with the per-layer edge_type_attention_weights (:94-96) as leaves, so
that their gradient is checked like every other variable's.  A plain module (imported by the tests), not a conftest."""
import numpy as np
import torch

import train_reference as TR


def model_layers(model):
    """train_reference.model_layers plus the attention factors [T] of every layer."""
    layers = TR.model_layers(model)
    for L, a in zip(layers, model.gnn_weights.edge_type_attention_weights):
        L["edge_type_attention_weights"] = a.detach().cpu().numpy()
    return layers


def oracle_loss_from_weights(oracle_torch, params, layers, readouts, feed, masks=None, device="cpu"):
    """-> (loss tensor, {variable name: leaf tensor}); the layout of train_reference.oracle_loss_from_weights, every layer with its
    'edge_type_attention_weights'."""
    assert params.get("use_propagation_attention") and not params.get("use_edge_bias", False)
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
        cell["edge_type_attention_weights"] = leaves["%s/edge_type_attention_weights_%i:0" % (scope, l)] = \
            d64(L["edge_type_attention_weights"]).requires_grad_(True)                            # :94-96
        base = "%s/timestep_0/gru_cell" % scope
        for key, name in (("Wg", "/gates/kernel:0"), ("bg", "/gates/bias:0"), ("Wc", "/candidate/kernel:0"), ("bc", "/candidate/bias:0")):
            cell[key] = leaves[base + name] = d64(L[key]).requires_grad_(True)
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
    """(loss, {variable name: d loss / d variable}) in float64 for the model's own weights, attention factors included."""
    loss, leaves = oracle_loss_from_weights(oracle_torch, model.params, model_layers(model), TR.readout_weights(model), feed, masks, device)
    loss.backward()
    return float(loss), {k: v.grad for k, v in leaves.items()}
