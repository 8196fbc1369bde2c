"""float64 reference of one training step of the sparse GCN: loss and d loss / d every variable.  The layer stack and its backward
are gcn_reference_math's (NumPy, written from chem_tensorflow_gcn.py:62-82); the gated regression and the masked task losses are
oracle/ggnn_oracle_torch.py's (chem_tensorflow_gcn.py:84-93, chem_tensorflow.py:161-169) with the 1/ratio factor of :168; the two
meet at d loss / d final states.  A plain module (imported by the tests), not a conftest."""
import numpy as np
import torch

import gcn_reference_math as ref

READOUT_NAMES = ("regression_gate/MLP_W_layer0", "regression_gate/MLP_b_layer0", "regression/MLP_W_layer0", "regression/MLP_b_layer0")


def fp64_step(oracle_torch, params, h0, adj, w, Ws, bs, masks, readouts, graph_nodes_list, num_graphs, targets, target_mask):
    """h0 [V, D], (adj [nnz, 2], w [nnz]) = A_hat, Ws / bs (bs None: no bias) per layer, masks: per layer None or the dropout FACTOR
    [V, D] (0 or 1/keep) of the hidden layers; readouts {task_id: (gate W, gate b, transform W, transform b)}; targets / target_mask
    [tasks, G].  -> (loss, {variable name: gradient as float64 tensor})."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    L = len(Ws)
    final, saved = ref.forward(f64(h0), adj, f64(w), [f64(W) for W in Ws], None if bs is None else [f64(b) for b in bs], masks)
    last = torch.from_numpy(final).requires_grad_(True)
    h0_t = torch.from_numpy(f64(h0))
    gnl = torch.as_tensor(np.asarray(graph_nodes_list)).long()
    t_values, t_mask = torch.from_numpy(f64(targets)), torch.from_numpy(f64(target_mask))
    grads, leaves = {}, {}
    loss = 0.0
    for internal_id, task_id in enumerate(params["task_ids"]):
        leaf = [torch.from_numpy(f64(a)).requires_grad_(True) for a in readouts[task_id]]
        for name, t in zip(READOUT_NAMES, leaf):
            leaves["out_layer_task%i/%s:0" % (task_id, name)] = t
        pred = oracle_torch.gated_regression(last, h0_t, gnl, int(num_graphs), *leaf)
        task_loss, _ = oracle_torch.task_loss(pred, t_values[internal_id], t_mask[internal_id])
        loss = loss + task_loss * (1.0 / (params["task_sample_ratios"].get(task_id) or 1.0))       # chem_tensorflow.py:168
    loss.backward()
    dWs, dbs = ref.backward(adj, f64(w), [f64(W) for W in Ws], saved, last.grad.numpy(), masks)
    for l in range(L):
        grads["graph_model/gcn_scope/gcn_weights_%i:0" % l] = torch.from_numpy(dWs[l])
        if bs is not None:
            grads["graph_model/gcn_scope/gcn_bias_%i:0" % l] = torch.from_numpy(dbs[l])
    grads.update({k: t.grad for k, t in leaves.items()})
    return float(loss.detach()), grads


def model_fp64_step(oracle_torch, model, feed, masks=None):
    """fp64_step on a SparseGCNChemModel's weights and one of its feeds (host-packed: with 'adjacency_list' / 'adjacency_weights')."""
    n = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    readouts = {}
    for task_id in model.params["task_ids"]:
        g, t = model.weights["regression_gate_task%i" % task_id], model.weights["regression_transform_task%i" % task_id]
        readouts[task_id] = (n(g.params["weights"][0]), n(g.params["biases"][0]), n(t.params["weights"][0]), n(t.params["biases"][0]))
    Ws = [n(W) for W in model.weights["edge_weights"]]
    bs = [n(b) for b in model.weights["edge_biases"]] if model.params["gcn_use_bias"] else None
    return fp64_step(oracle_torch, model.params, n(feed["initial_node_representation"]), n(feed["adjacency_list"]),
                     n(feed["adjacency_weights"]), Ws, bs, masks, readouts, n(feed["graph_nodes_list"]), feed["num_graphs"],
                     n(feed["target_values"]), n(feed["target_mask"]))
