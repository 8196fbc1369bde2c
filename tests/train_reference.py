"""fp64 reference gradients of the sparse model's training step, a hook on the gradient the optimiser consumes, and the comparison
the training-gradient tests use.  A plain module (imported by the tests), not a conftest.

* capture_step_gradients(model): clones every variable's view of the flat gradient buffer just before TFAdam.clip_and_apply --
  the one place that sees the native step (train_native.py), the autograd path with its weight-gradient sink, and the
  all-reduced buffer under data parallelism.
* dropout_masks(oracle, model, ...): the 0/1 weight masks the NEXT train_batch draws (take them before train_batch: it advances
  model.dropout_step), restated with oracle.counter_dropout from the model's own seeds.
* oracle_loss_and_grads(...): loss and d loss / d every variable by torch autograd of oracle/ggnn_oracle_torch.py in float64 --
  every task of task_ids with the 1/ratio factor of chem_tensorflow.py:168, the edge-weight masks of
  chem_tensorflow_sparse.py:91 and the readout-weight masks of utils.py:68, on the CPU or on a device.
"""
import contextlib

import numpy as np
import torch

SMALL_NUMBER = 1e-7                 # utils.py:8


@contextlib.contextmanager
def capture_step_gradients(model):
    """Within the block every optimiser step appends {variable name: clone of its pre-clip gradient} to the yielded list.  The
    original clip_and_apply then runs unchanged."""
    opt = model.optimizer
    assert opt.fused, "the capture reads the flat gradient buffer of the fused optimiser"
    names = {v.data_ptr(): n for n, v in model.named_variables().items()}
    steps = []
    original = opt.clip_and_apply

    def clip_and_apply(clip_norm):
        steps.append({names[v.data_ptr()]: g.detach().clone() for v, g in zip(opt.vars, opt._flat["g_views"])})
        return original(clip_norm)

    opt.clip_and_apply = clip_and_apply
    try:
        yield steps
    finally:
        del opt.clip_and_apply          # (the class's method again)


def _mask01(oracle, shape, keep, seed):
    return (oracle.counter_dropout(np.ones(shape, np.float32), keep, seed) != 0).astype(np.float64)


def dropout_masks(oracle, model, edge_keep=1.0, readout_keep=1.0):
    """The weight masks of the step model.train_batch is about to take: {"edge_keep", "edge": [0/1 [T*D, D] per layer] or None,
    "readout_keep", "readout": {(kind, task_id): 0/1 [rows, 1]} or None}.  Seeds and row keys as the model derives them:
    model.dropout_seed('edge_weights', l) over the [T*D, D] variable; MLP.dropped_weight (utils.py) draws
    model.dropout_seed(kind, task_id, 0) over the [rows, 1] weight, row keys 0..rows-1."""
    out = {"edge_keep": float(edge_keep), "edge": None, "readout_keep": float(readout_keep), "readout": None}
    if edge_keep < 1.0:
        out["edge"] = [_mask01(oracle, tuple(w.shape), edge_keep, model.dropout_seed("edge_weights", l))
                       for l, w in enumerate(model._edge_weight_vars)]
    if readout_keep < 1.0:
        out["readout"] = {}
        for task_id in model.params["task_ids"]:
            for kind in ("regression_gate", "regression_transform"):
                W = model.weights["%s_task%i" % (kind, task_id)].params["weights"][0]
                out["readout"][(kind, task_id)] = _mask01(oracle, tuple(W.shape), readout_keep, model.dropout_seed(kind, task_id, 0))
    return out


def readout_weights(model):
    """{task_id: (gate W, gate b, transform W, transform b)} as float32 NumPy arrays."""
    f = lambda t: t.detach().cpu().numpy()
    out = {}
    for task_id in model.params["task_ids"]:
        g, t = model.weights["regression_gate_task%i" % task_id], model.weights["regression_transform_task%i" % task_id]
        out[task_id] = (f(g.params["weights"][0]), f(g.params["biases"][0]), f(t.params["weights"][0]), f(t.params["biases"][0]))
    return out


def oracle_loss_from_weights(oracle_torch, params, layers, readouts, feed, masks=None, device="cpu"):
    """float64 autograd of the oracle on explicit weights.  layers: ggnn_oracle.make_sparse_layers layout; readouts:
    readout_weights layout; feed: the model's feed (tensors on any device); masks: dropout_masks layout or None.
    -> (loss tensor, {variable name: leaf tensor}) -- call loss.backward() for the gradients."""
    dev = torch.device(device)
    d64 = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a.detach()).to(dev, torch.float64)
    masks = masks or {"edge": None, "readout": None}
    leaves = {}
    tl = []
    for l, L in enumerate(layers):
        scope = "graph_model/gnn_layer_%i" % l
        T, D = np.asarray(L["edge_weights"]).shape[0], np.asarray(L["edge_weights"]).shape[-1]
        ew = d64(L["edge_weights"]).reshape(T * D, D).requires_grad_(True)
        leaves["%s/gnn_edge_weights_%i:0" % (scope, l)] = ew
        W = ew if masks["edge"] is None else ew * d64(masks["edge"][l]) / masks["edge_keep"]      # :91
        cell = {"edge_weights": W.reshape(T, D, D)}
        base = "%s/timestep_0/gru_cell" % scope
        for key, name in (("Wg", "/gates/kernel:0"), ("bg", "/gates/bias:0"), ("Wc", "/candidate/kernel:0"), ("bc", "/candidate/bias:0")):
            cell[key] = leaves[base + name] = d64(L[key]).requires_grad_(True)
        if params.get("use_edge_bias", False):
            cell["edge_biases"] = leaves["%s/gnn_edge_biases_%i:0" % (scope, l)] = d64(L["edge_biases"]).requires_grad_(True)
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


def oracle_loss_and_grads(oracle_torch, model, layers, feed, masks=None, device="cpu"):
    """float64 torch autograd of the oracle for `model`'s params and readout weights: (loss, {variable name: d loss / d
    variable}), each gradient in the variable's shape (edge weights [T*D, D])."""
    loss, leaves = oracle_loss_from_weights(oracle_torch, model.params, layers, readout_weights(model), feed, masks, device)
    loss.backward()
    return float(loss), {k: v.grad for k, v in leaves.items()}


def model_layers(model):
    """The model's graph weights in the oracle layout (as float32 NumPy)."""
    f = lambda t: t.detach().cpu().numpy()
    T, D = model.num_edge_types, model.params["hidden_size"]
    out = []
    for l, cell in enumerate(model.gnn_weights.rnn_cells):
        L = {"edge_weights": f(model._edge_weight_vars[l]).reshape(T, D, D), "Wg": f(cell.gates_kernel), "bg": f(cell.gates_bias),
             "Wc": f(cell.candidate_kernel), "bc": f(cell.candidate_bias)}
        if model.params["use_edge_bias"]:
            L["edge_biases"] = f(model.gnn_weights.edge_biases[l])
        out.append(L)
    return out


# ---- comparison ----------------------------------------------------------------------------------------------------------------
def gradient_failures(got, want, rtol=2e-4, atol=1e-7):
    """Per variable: max |got - want| <= rtol * max |want| + atol.  -> [(name, err, scale)] of the variables that fail (a
    missing variable or a shape mismatch fails too)."""
    bad = []
    if set(got) != set(want):
        return [(n, float("inf"), 0.0) for n in sorted(set(got) ^ set(want))]
    for name, w in want.items():
        w = w.detach().double()
        g = got[name].detach().to(w.device, torch.float64)
        if g.numel() != w.numel():
            bad.append((name, float("inf"), 0.0))
            continue
        scale = float(w.abs().max()) if w.numel() else 0.0
        err = float((g.reshape(w.shape) - w).abs().max()) if w.numel() else 0.0
        if not err <= rtol * scale + atol:
            bad.append((name, err, scale))
    return bad


def assert_gradients_match(got, want, rtol=2e-4, atol=1e-7):
    bad = gradient_failures(got, want, rtol, atol)
    assert not bad, bad


def assert_comparison_has_teeth(got, want, rtol=2e-4, atol=1e-7):
    """The comparison rejects the captured gradients (i) with the variable of the largest gradient scaled by 1 + 10 rtol and (ii)
    with the row holding the largest entry of the largest edge-weight gradient zeroed."""
    big = max(want, key=lambda k: float(want[k].abs().max()))
    scaled = dict(got); scaled[big] = got[big] * (1 + 10 * rtol)
    assert any(n == big for n, _, _ in gradient_failures(scaled, want, rtol, atol)), big
    ew = [k for k in want if "/gnn_edge_weights_" in k]
    big = max(ew, key=lambda k: float(want[k].abs().max()))
    g = got[big].detach().clone().reshape(want[big].shape)
    row = int(want[big].abs().max(dim=1).values.argmax())
    g[row] = 0
    assert any(n == big for n, _, _ in gradient_failures(dict(got, **{big: g}), want, rtol, atol)), big


def normwise_errors(got, want):
    """{name: (||got - want|| / ||want||, max |got - want| / max |want|)}."""
    out = {}
    for name, w in want.items():
        w = w.detach().double()
        g = got[name].detach().to(w.device, torch.float64).reshape(w.shape)
        out[name] = (float((g - w).norm() / w.norm().clamp_min(1e-300)), float((g - w).abs().max() / w.abs().max().clamp_min(1e-300)))
    return out
