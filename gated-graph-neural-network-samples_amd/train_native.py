"""The optimisation step of the default sparse model on the native launch sequences of csrc/ggnn_train.hip
(ggnn_sparse_train_forward_f32 / ggnn_sparse_train_backward_f32): what chem_tensorflow.py:183-191 runs through sess.run --
forward (chem_tensorflow_sparse.py:117-218), gated regression + masked loss (:220-231, chem_tensorflow.py:158-170),
compute_gradients, per-variable clip_by_norm, Adam -- without torch.autograd in between.

train.train_step takes this path when the model is the default one (GRU cell, no attention, no edge bias, state keep-prob 1, a
hidden size with the gather-fused kernels, at most two residual inputs per layer, every graph variable trainable); everything
else keeps the autograd path (backward.PropagationStepFn, variants.py), which is also what this one is tested against.

Per step the host makes two C calls for the propagation, one ops call per task for the readout forward and one for its backward
(params['multitask_readout']: one of each for all tasks), a
handful of launches for the weight images and masks, and the optimizer's two launches: ~1 ms of host time instead of ~4.4 ms.

The dense model (chem_tensorflow_dense.py:93-117) has the same step on csrc/ggnn_dense_train.hip (ggnn_dense_train_forward_f32 /
ggnn_dense_train_backward_f32) when its config asks for it with graph_resident_training = 'native': dense_eligible /
native_dense_train_step below.  The sparse GCN (chem_tensorflow_gcn.py:62-82) has it on csrc/ggnn_gcn_train.hip
(ggnn_gcn_train_forward_f32 / ggnn_gcn_train_backward_f32; at hidden sizes 128 / 192 / 256 with gcn_panel_layers = True their panel
twins ggnn_gcn_panel_train_forward_f32 / ggnn_gcn_panel_train_backward_f32) under native_training = True: gcn_eligible /
native_gcn_train_step at the end of this file.

The sparse model with propagation attention on the compacted route (chem_tensorflow_sparse.py:147-149, 170-196;
SparseGGNNChemModel.attention_route) has it on ggnn_sparse_attn_train_forward_f32 / ggnn_sparse_attn_train_backward_f32 when its
config says compact_attention = 'native' (True keeps variants.CompactAttentionStepFn): attn_eligible / native_attn_train_step, the
default model's step below with the attention arguments added.

The default sparse model at the column-panel hidden sizes 128 / 192 / 256 has it on ggnn_sparse_train_panel_forward_f32 /
ggnn_sparse_train_panel_backward_f32 (the same driver on its panel route, csrc/ggnn_train.hip) when its config says
native_panel_training = True: panel_eligible / native_panel_train_step, again the default model's step below with a route argument.
Without the key these sizes keep the autograd step (backward.PropagationStepFn on the panel kernels).

The sparse model with the BasicRNNCell on the compacted route (graph_rnn_cell = RNN, the R-GCN configuration;
SparseGGNNChemModel.rnn_route) has it on ggnn_sparse_rnn_train_forward_f32 / ggnn_sparse_rnn_train_backward_f32 when its config says
compact_rnn = 'native' (True keeps variants.CompactRnnStepFn): rnn_eligible / native_rnn_train_step, the default model's step below
with the cell's arguments in place of the GRU's.  Its weight images come layer by layer from ops.PACKED (one entry per weight
version): there is no one-launch prepare for this cell.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Optional

import torch

from . import _lib, backward, ops
from ._lib import check
from .utils import SMALL_NUMBER


import os

# the hidden sizes of the column-panel kernels (the native step's panel route: params['native_panel_training'])
PANEL_SIZES = (128, 192, 256)

# all of a step's weight images in one launch (GGNN_FUSED_PREPARE=0: mask / transpose / pack layer by layer through the caches of ops.py)
USE_FUSED_PREPARE = os.environ.get("GGNN_FUSED_PREPARE", "1") != "0"


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _i32(xs):
    return (ctypes.c_int32 * max(len(xs), 1))(*[int(x) for x in xs])


# ---- the readout + loss of a native step: per task (one forward and one backward ops call each), or all tasks at once -------------
def _readout_per_task_forward(model, final, h0, gnl, gptr, node_mask, G: int):
    """Gated regression + masked loss per task (chem_tensorflow_sparse.py:220-231 / chem_tensorflow_dense.py:119-129,
    chem_tensorflow.py:158-170); fills model.ops / model.output.  -> (what the backward needs, the loss, the [K] mask counts)."""
    p, ph = model.params, model.placeholders
    per_task, losses = [], []
    for internal_id, task_id in enumerate(p['task_ids']):
        gate, tr = model.weights['regression_gate_task%i' % task_id], model.weights['regression_transform_task%i' % task_id]
        gW, tW = gate.dropped_weight(0).reshape(-1).contiguous(), tr.dropped_weight(0).reshape(-1).contiguous()    # utils.py:68
        target = ph['target_values'][internal_id, :].contiguous()
        mask = ph['target_mask'][internal_id, :].contiguous()
        out, ngate, nval, stats = ops.readout_loss_fwd(final, h0, gnl, gptr, node_mask, G, gW, gate.params["biases"][0].reshape(-1), tW,
                                                       tr.params["biases"][0].reshape(-1), target, mask)
        per_task.append((gate, tr, gW, tW, ngate, nval, out, target, mask))
        num, ab, ms = stats[0], stats[1], stats[2]
        den = ms + SMALL_NUMBER
        ratio = model.task_ratio(task_id)                                           # chem_tensorflow.py:168
        model.ops['accuracy_task%i' % task_id] = ab / den
        model.ops['loss_numerator_task%i' % task_id] = num
        model.ops['abs_error_sum_task%i' % task_id] = ab
        model.ops['loss_denominator_task%i' % task_id] = ms
        losses.append(num / den * ratio)
        model.output = out
    model.ops['losses'] = losses
    loss = torch.stack(losses).sum()
    model.ops['loss'] = loss
    dens = torch.stack([model.ops['loss_denominator_task%i' % t] for t in p['task_ids']]).to(torch.float32)
    return (per_task, final, h0, gnl, node_mask, G), loss, dens


def _readout_per_task_backward(model, saved, dens, gviews):
    """d loss / d stats[0] = ratio / (dens + eps) per task, the weight gradients straight into the optimizer's flat gradient views,
    d_final accumulated over the tasks.  -> d_final [V,D]."""
    per_task, final, h0, gnl, node_mask, G = saved
    p, ph = model.params, model.placeholders
    d_final = None
    for internal_id, task_id in enumerate(p['task_ids']):
        gate, tr, gW, tW, ngate, nval, out, target, mask = per_task[internal_id]
        ratio = model.task_ratio(task_id)
        d_stats = torch.stack([ratio / (dens[internal_id] + SMALL_NUMBER), torch.zeros((), dtype=torch.float32, device=final.device)]).contiguous()
        dst = [gviews[gate.params["weights"][0].data_ptr()], gviews[gate.params["biases"][0].data_ptr()],
               gviews[tr.params["weights"][0].data_ptr()], gviews[tr.params["biases"][0].data_ptr()]]
        d_final = ops.readout_loss_bwd(final, h0, gnl, node_mask, G, gW, tW, ngate, nval, out, target, mask, None, d_stats,
                                       d_last_h=d_final, grad_out=dst)[0]
        keep = float(ph.get('out_layer_dropout_keep_prob', 1.0))
        if keep < 1.0:                                                              # utils.py:68: the masks of the forward
            ops.dropout(dst[0], keep, gate.dropout_seed(0), out=dst[0])
            ops.dropout(dst[2], keep, tr.dropout_seed(0), out=dst[2])
    return d_final


# ---- params['multitask_readout']: the readout of EVERY task in one forward and one backward call (ops.readout_multi_*) ------------
def _multitask_readout(model, width: int) -> bool:
    """The step's readout runs on the multi-task kernels: the key is set (read with .get: not a key of default_params), two or
    more tasks, and kernels for (width, K); anything else keeps the per-task loop."""
    p = model.params
    K = len(p['task_ids'])
    return bool(p.get('multitask_readout')) and K >= 2 and ops.readout_multi_supported(width, K)


def _readout_multi_forward(model, final, h0, gnl, gptr, node_mask, G: int):
    """One forward call for all tasks; model.ops' per-task entries become views of the [K,3] stats (ChemModel.publish_task_stats).
    -> (what the backward needs, its last entry the [K,3] stats; the loss; a copy of the [K] mask counts)."""
    p, ph = model.params, model.placeholders
    gates = [model.weights['regression_gate_task%i' % t] for t in p['task_ids']]
    trs = [model.weights['regression_transform_task%i' % t] for t in p['task_ids']]
    gWs = [m.dropped_weight(0).reshape(-1).contiguous() for m in gates]                          # utils.py:68, one mask per task
    tWs = [m.dropped_weight(0).reshape(-1).contiguous() for m in trs]
    targets, masks = ph['target_values'].contiguous(), ph['target_mask'].contiguous()
    out, node_gv, stats = ops.readout_multi_fwd(final, h0, gnl, gptr, node_mask, G, gWs, [m.params["biases"][0].reshape(-1) for m in gates],
                                                tWs, [m.params["biases"][0].reshape(-1) for m in trs], targets, masks)
    loss = model.publish_task_stats(out, stats[:, 0], stats[:, 1], stats[:, 2])
    return (gates, trs, gWs, tWs, node_gv, out, targets, masks, final, h0, gnl, node_mask, G, stats), loss, stats[:, 2].clone()


def _readout_multi_backward(model, saved, dens, gviews):
    """One backward call for all tasks: d loss / d stats[k,0] = ratio_k / (dens_k + eps), the weight gradients straight into the
    optimizer's flat gradient views (then the forward's weight-dropout masks, per task).  -> d_final [V,D]."""
    gates, trs, gWs, tWs, node_gv, out, targets, masks, final, h0, gnl, node_mask, G, _stats = saved
    d_num = model.task_ratio_factors(dens.device) / (dens + SMALL_NUMBER)
    d_stats = torch.stack([d_num, torch.zeros_like(d_num)], dim=1).contiguous()
    dst = ([gviews[m.params["weights"][0].data_ptr()] for m in gates], [gviews[m.params["biases"][0].data_ptr()] for m in gates],
           [gviews[m.params["weights"][0].data_ptr()] for m in trs], [gviews[m.params["biases"][0].data_ptr()] for m in trs])
    d_final = ops.readout_multi_bwd(final, h0, gnl, node_mask, G, gWs, tWs, node_gv, out, targets, masks, None, d_stats, grad_out=dst)[0]
    keep = float(model.placeholders.get('out_layer_dropout_keep_prob', 1.0))
    if keep < 1.0:                                                                           # utils.py:68: the masks of the forward
        for gate, tr, dgW, dtW in zip(gates, trs, dst[0], dst[2]):
            ops.dropout(dgW, keep, gate.dropout_seed(0), out=dgW)
            ops.dropout(dtW, keep, tr.dropout_seed(0), out=dtW)
    return d_final


def model_eligible(model) -> bool:
    """The part of `eligible` that depends on the model only (run_epoch uses it to choose how batches are prefetched)."""
    return _sparse_model_eligible(model, False)


def attn_model_eligible(model) -> bool:
    """The part of `attn_eligible` that depends on the model only: a sparse model whose config asks for the native step with
    params['compact_attention'] == 'native' (read with .get: not a key of default_params, whose keys a reference checkpoint must
    match; True keeps the autograd step) and whose attention runs on the compacted route (attention_route()), under the default
    model's conditions otherwise -- hidden size 32 / 64 / 100 unpadded, no edge bias, no graph-state dropout, at most two residual
    inputs per layer, the fused optimizer over exactly the trainable variables, nothing frozen, one-layer readout MLPs -- and no
    active data-parallel context."""
    return _sparse_model_eligible(model, True)


def panel_model_eligible(model) -> bool:
    """The part of `panel_eligible` that depends on the model only: a sparse model whose config asks for the native step at the
    column-panel sizes with params['native_panel_training'] (read with .get: not a key of default_params, whose keys a reference
    checkpoint must match) and whose hidden size is 128 / 192 / 256 unpadded (116, which pads to 128, keeps autograd), under the
    default model's conditions otherwise -- GRU cell, no attention, no edge bias, no graph-state dropout, at most two residual inputs
    per layer, the fused optimizer over exactly the trainable variables, nothing frozen, one-layer readout MLPs -- and no active
    data-parallel context."""
    return _sparse_model_eligible(model, False, panel=True)


def rnn_model_eligible(model) -> bool:
    """The part of `rnn_eligible` that depends on the model only: a sparse model whose config asks for the native step with
    params['compact_rnn'] == 'native' (read with .get: not a key of default_params, whose keys a reference checkpoint must match;
    True keeps the autograd step) and whose BasicRNNCell runs on the compacted route (rnn_route()), hidden size unpadded, every
    layer's (hidden size, inputs) in ops.rnn_fused_supported -- 32 / 64 with at most two residual inputs, 100 with none -- no edge
    bias, no graph-state dropout, the fused optimizer over exactly the trainable variables, nothing frozen, one-layer readout MLPs,
    and no active data-parallel context."""
    p = getattr(model, "params", None)
    if p is None or not hasattr(model, "_edge_weight_vars") or not hasattr(model, "rnn_route") or not torch.cuda.is_available():
        return False
    if not backward.USE_NATIVE_STEP or not backward.USE_COMPACT_TRANSFORM:
        return False
    if p.get('compact_rnn') != 'native' or not model.rnn_route() or p['use_edge_bias'] or not p['use_graph']:
        return False
    dist = getattr(model, "dist", None)
    if (dist is not None and dist.active) or torch.device(model.device).type != 'cuda':
        return False
    D = p['hidden_size']
    if model._kw != D or float(p.get('graph_state_dropout_keep_prob', 1.0)) < 1.0:
        return False
    L = len(p['layer_timesteps'])
    if L > 60 or any(int(s) < 1 for s in p['layer_timesteps']):
        return False
    if any(not ops.rnn_fused_supported(D, len(p['residual_connections'].get(str(l)) or []) + 1) for l in range(L)):
        return False
    return _optimizer_and_readout_eligible(model)


def rnn_eligible(model, batch_data: Dict[str, Any]) -> bool:
    """True when this step of a model with the BasicRNNCell can run on the native sequences: rnn_model_eligible, no per-launch
    timing, and a batch on the GPU, sorted by graph, with at least one message."""
    return ops._timing is None and rnn_model_eligible(model) and _sparse_batch_eligible(model, batch_data)


def _optimizer_and_readout_eligible(model) -> bool:
    """The fused optimizer over exactly the trainable variables, nothing frozen, one-layer readout MLPs."""
    p = model.params
    opt = model.optimizer
    variables = list(model.trainable_variables.values())
    if not (opt.fused and len(opt.vars) == len(variables) and all(a is b for a, b in zip(opt.vars, variables))):
        return False
    have = {v.data_ptr() for v in variables}
    if any(v.data_ptr() not in have for v in model.named_variables().values()):        # (--freeze-graph-model)
        return False
    for task_id in p['task_ids']:
        if len(model.weights['regression_gate_task%i' % task_id].params["weights"]) != 1:
            return False
    return True


def _sparse_model_eligible(model, attention: bool, panel: bool = False) -> bool:
    p = getattr(model, "params", None)
    if p is None or not hasattr(model, "_edge_weight_vars") or not torch.cuda.is_available():
        return False
    if not backward.USE_NATIVE_STEP or not backward.USE_COMPACT_TRANSFORM or not (panel or backward.TRAIN_GATHER_IN_GRU):
        return False
    D = p['hidden_size']
    if getattr(model, "cell_type", None) != 'gru' or bool(p['use_propagation_attention']) != attention or p['use_edge_bias'] \
            or not p['use_graph']:
        return False
    if attention:
        dist = getattr(model, "dist", None)
        if p.get('compact_attention') != 'native' or not model.attention_route() or (dist is not None and dist.active):
            return False
    if panel:
        dist = getattr(model, "dist", None)
        if not p.get('native_panel_training') or (dist is not None and dist.active):
            return False
    if torch.device(model.device).type != 'cuda':
        return False
    if panel:
        if model._kw != D or D not in PANEL_SIZES or not _lib.load().ggnn_sparse_train_panel_supported(D) \
                or not ops.compact_supported(D) or not ops.gru_bwd_is_fused(D):
            return False
    elif model._kw != D or not ops.gru_gather_fused(D) or not ops.compact_supported(D) or D > 104 or not ops.gru_bwd_is_fused(D):
        return False
    if float(p.get('graph_state_dropout_keep_prob', 1.0)) < 1.0:
        return False
    L = len(p['layer_timesteps'])
    if L > 60 or any(int(s) < 1 for s in p['layer_timesteps']):
        return False
    if any(len(p['residual_connections'].get(str(l)) or []) + 1 > ops.GRU_FUSED_MAX_INPUTS for l in range(L)):
        return False
    return _optimizer_and_readout_eligible(model)


def eligible(model, batch_data: Dict[str, Any]) -> bool:
    """True when this step can run on the native sequences (see the module docstring)."""
    return _sparse_eligible(model, batch_data, False)


def attn_eligible(model, batch_data: Dict[str, Any]) -> bool:
    """True when this step of a model with propagation attention can run on the native sequences: attn_model_eligible, no
    per-launch timing, and a batch on the GPU, sorted by graph, with at least one message."""
    return _sparse_eligible(model, batch_data, True)


def panel_eligible(model, batch_data: Dict[str, Any]) -> bool:
    """True when this step of the default model at hidden size 128 / 192 / 256 can run on the native sequences' panel route:
    panel_model_eligible, no per-launch timing, and a batch on the GPU, sorted by graph, with at least one message."""
    return _sparse_eligible(model, batch_data, False, panel=True)


def _sparse_eligible(model, batch_data: Dict[str, Any], attention: bool, panel: bool = False) -> bool:
    if ops._timing is not None or not _sparse_model_eligible(model, attention, panel):
        return False
    return _sparse_batch_eligible(model, batch_data)


def _sparse_batch_eligible(model, batch_data: Dict[str, Any]) -> bool:
    """A batch the native sequences take: on the GPU, sorted by graph, at least one message, no graph-state dropout."""
    D = model.params['hidden_size']
    if float(batch_data.get('graph_state_keep_prob', 1.0)) < 1.0:
        return False
    h0 = batch_data.get('initial_node_representation')
    index = batch_data.get('message_index')
    if h0 is None or index is None or not h0.is_cuda or h0.shape[0] == 0 or h0.shape[1] != D or index.num_messages == 0:
        return False
    if batch_data.get('graph_nodes_sorted') is not True or int(batch_data['num_graphs']) == 0:
        return False
    return True


class _Workspace:
    """One growing device buffer per model: the saved tensors and temporaries of a step (ggnn_sparse_train_workspace_bytes) and the
    layer-input gradient accumulators.  Allocated on the training stream, reused by every step."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.dstate: Optional[torch.Tensor] = None

    def get(self, nbytes: int, L: int, V: int, D: int, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(int(nbytes * 1.05) + 256, dtype=torch.uint8, device=device)
        if self.dstate is None or self.dstate.numel() < L * V * D or self.dstate.device != device:
            self.dstate = torch.empty(int(L * V * D * 1.05) + 64, dtype=torch.float32, device=device)
        return self.buf, [self.dstate[l * V * D:(l + 1) * V * D].view(V, D) for l in range(L)]


def native_train_step(model, batch_data: Dict[str, Any]) -> torch.Tensor:
    return _native_sparse_step(model, batch_data, False)


def native_attn_train_step(model, batch_data: Dict[str, Any]) -> torch.Tensor:
    """native_train_step with propagation attention: the same two C calls in their attention form, the same readout, loss, clip and
    Adam; the attention factors' gradients arrive in the optimizer's gradient views like every other graph variable's."""
    return _native_sparse_step(model, batch_data, True)


def native_panel_train_step(model, batch_data: Dict[str, Any]) -> torch.Tensor:
    """native_train_step at the column-panel hidden sizes 128 / 192 / 256: the same two C calls on the driver's panel route
    (ggnn_sparse_train_panel_forward_f32 / ggnn_sparse_train_panel_backward_f32), the images of the step from
    ggnn_sparse_train_panel_prepare_f32, the same readout, loss, clip and Adam."""
    return _native_sparse_step(model, batch_data, False, panel=True)


def native_rnn_train_step(model, batch_data: Dict[str, Any]) -> torch.Tensor:
    """native_train_step for the BasicRNNCell on the compacted route: the same two C calls in their RNN form
    (ggnn_sparse_rnn_train_forward_f32 / ggnn_sparse_rnn_train_backward_f32), the same readout, loss, clip and Adam; the cell's
    kernel and bias gradients arrive in the optimizer's gradient views like every other graph variable's."""
    return _native_sparse_step(model, batch_data, False, rnn=True)


def _native_sparse_step(model, batch_data: Dict[str, Any], attention: bool, panel: bool = False, rnn: bool = False) -> torch.Tensor:
    lib = _lib.load()
    # the entry points of the route: whole-block sizes (32 / 64 / 100) or column panels (128 / 192 / 256), one argument list
    if panel:
        prepare, workspace_bytes = lib.ggnn_sparse_train_panel_prepare_f32, lib.ggnn_sparse_train_panel_workspace_bytes
        train_forward, train_backward = lib.ggnn_sparse_train_panel_forward_f32, lib.ggnn_sparse_train_panel_backward_f32
    else:
        prepare, workspace_bytes = lib.ggnn_sparse_train_prepare_f32, lib.ggnn_sparse_train_workspace_bytes
        train_forward, train_backward = lib.ggnn_sparse_train_forward_f32, lib.ggnn_sparse_train_backward_f32
    p = model.params
    opt = model.optimizer
    model.feed(batch_data)
    ph = model.placeholders
    h0 = ph['initial_node_representation'].contiguous()
    V, D = h0.shape
    T = model.num_edge_types
    L = len(p['layer_timesteps'])
    steps = int(sum(p['layer_timesteps']))
    index = ph['message_index']
    comp = getattr(index, "_compact", None)
    if comp is None or getattr(comp, "_bwd", None) is None:
        ops.prepare_message_index(index, D, True, training=True)
        comp = index._compact
    bwd = ops.compact_backward(index, comp)
    R = comp.num_rows
    use_avg = bool(p['use_edge_msg_avg_aggregation'])
    nin = ph['num_incoming_edges_per_type']
    act = ops.ACT_IDS[p['graph_rnn_activation'].lower()]
    residuals = [[int(i) for i in (p['residual_connections'].get(str(l)) or [])] for l in range(L)]
    res_ptr, res_idx = [0], []
    for r in residuals:
        res_idx.extend(r)
        res_ptr.append(len(res_idx))
    st = torch.cuda.current_stream()
    if getattr(model, "_native_ws", None) is None:
        model._native_ws = _Workspace()
    side = backward.side_stream(h0.device)
    dev = h0.device

    with torch.no_grad():
        # ---- this step's weights: masked edge weights (:91, one mask per layer and step) and the kernels' stage images ----
        ew_keep = float(ph.get('edge_weight_dropout_keep_prob', 1.0))
        cells = model.gnn_weights.rnn_cells
        masks = [(ew_keep, model.dropout_seed('edge_weights', l)) for l in range(L)] if ew_keep < 1.0 else []
        nxs = [len(residuals[l]) + 1 for l in range(L)]
        # operand format of each layer's GRU forward: two-piece f16 only where this step's operands are provably in its range
        # (formats.py: max|h0|, the weights' maxima tracked across optimizer steps, tanh cell, mean aggregation), else exact bf16x3
        gru_fmts = [ops.GRU_FMT_EXACT] * L if rnn else model.gru_formats(h0, ew_keep, 1.0, training=True)
        if attention:                      # (the range proof does not cover attention-weighted sums: every product exact)
            gru_fmts = [ops.GRU_FMT_EXACT] * L
        fm = _i32(gru_fmts)
        if rnn:
            # layer by layer through the version-keyed cache: the images of the key-True route's launches, bit for bit (every
            # product exact: ReLU states have no bound)
            edge_packed, edge_packed_t, rnn_packed, rnn_bwd_packed = [], [], [], []
            for l in range(L):
                W = model._edge_weight_vars[l].view(T, D, D)
                if masks:
                    W = backward.masked(W, masks[l][0], masks[l][1])
                edge_packed.append(ops.PACKED.edge(W))
                edge_packed_t.append(ops.PACKED.edge_t(W))
                rnn_packed.append(ops.PACKED.rnn(cells[l].kernel, nxs[l], D))
                rnn_bwd_packed.append(ops.PACKED.rnn_bwd(cells[l].kernel, nxs[l], D))
        elif L <= 16 and USE_FUSED_PREPARE:
            # all ~120 images of the step in ONE launch, the weight-dropout mask applied on the fly (ggnn_sparse_train_prepare_f32)
            imgs = getattr(model, "_native_images", None)
            if imgs is None:
                f32 = lambda nbytes: torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
                eb = lib.ggnn_msg_transform_compact_workspace_bytes(D, T)
                imgs = model._native_images = (
                    [f32(eb) for _ in range(L)], [f32(eb) for _ in range(L)],
                    [f32(lib.ggnn_gru_packed_bytes(D, nxs[l])) for l in range(L)],
                    [f32(lib.ggnn_gru_bwd_packed_bytes(D, nxs[l])) for l in range(L)])
            edge_packed, edge_packed_t, gru_packed, gru_bwd_packed = imgs
            seeds = (ctypes.c_uint64 * L)(*[m[1] for m in masks]) if masks else None
            check(prepare(
                L, T, D, _i32(nxs), _ptrs(model._edge_weight_vars), ew_keep if masks else 1.0, seeds,
                _ptrs([c.gates_kernel for c in cells]), _ptrs([c.candidate_kernel for c in cells]), fm, _ptrs(edge_packed),
                _ptrs(edge_packed_t), _ptrs(gru_packed), _ptrs(gru_bwd_packed), st.cuda_stream))
        else:
            edge_packed, edge_packed_t, gru_packed, gru_bwd_packed = [], [], [], []
            for l in range(L):
                W = model._edge_weight_vars[l].view(T, D, D)
                if masks:
                    W = backward.masked(W, masks[l][0], masks[l][1])
                edge_packed.append(ops.PACKED.edge(W))
                edge_packed_t.append(ops.PACKED.edge_t(W))
                gru_packed.append(ops.PACKED.gru(cells[l].gates_kernel, cells[l].candidate_kernel, nxs[l], D, gru_fmts[l]))
                gru_bwd_packed.append(ops.PACKED.gru_bwd(cells[l].gates_kernel, cells[l].candidate_kernel, nxs[l], D))

        # ---- forward ------------------------------------------------------------------------------------------------------
        M = index.num_messages
        if attention:
            ws_bytes = lib.ggnn_sparse_attn_train_workspace_bytes(V, D, T, R, steps, M)
            factors = _ptrs(model.gnn_weights.edge_type_attention_weights)
        elif rnn:
            ws_bytes = lib.ggnn_sparse_rnn_train_workspace_bytes(V, D, T, R, steps)
            if not ws_bytes:
                raise ValueError("native training step, RNN cell: no workspace for V=%d D=%d T=%d rows=%d steps=%d" % (V, D, T, R, steps))
        else:
            ws_bytes = workspace_bytes(V, D, T, R, steps)
            if not ws_bytes:
                raise ValueError("native training step: no workspace for V=%d D=%d T=%d rows=%d steps=%d" % (V, D, T, R, steps))
        ws, dstate = model._native_ws.get(ws_bytes, L, V, D, dev)
        tro = (ctypes.c_int64 * (T + 1))(*comp.type_row_off)
        lt, rp, ri = _i32(p['layer_timesteps']), _i32(res_ptr), _i32(res_idx)
        if not rnn:
            bg = _ptrs([c.gates_bias for c in cells]); bc = _ptrs([c.candidate_bias for c in cells])
        final_off = ctypes.c_int64(0)
        if rnn:
            ops._launch("sparse_rnn_train_forward[steps=%d]" % steps, lambda: lib.ggnn_sparse_rnn_train_forward_f32(
                h0.data_ptr(), V, D, T, M, index.row_ptr.data_ptr(), comp.gather_row.data_ptr(), comp.pair_node.data_ptr(), tro,
                nin.data_ptr(), 1 if use_avg else 0, L, lt, rp, ri, _ptrs(edge_packed), _ptrs([c.bias for c in cells]),
                _ptrs(rnn_packed), act, ws.data_ptr(), ws.numel(), ctypes.byref(final_off), st.cuda_stream))
        elif attention:
            ops._launch("sparse_attn_train_forward[steps=%d]" % steps, lambda: lib.ggnn_sparse_attn_train_forward_f32(
                h0.data_ptr(), V, D, T, M, index.row_ptr.data_ptr(), index.gather_row.data_ptr(), comp.gather_row.data_ptr(),
                comp.pair_node.data_ptr(), tro, nin.data_ptr(), 1 if use_avg else 0, L, lt, rp, ri, _ptrs(edge_packed), factors, bg, bc,
                _ptrs(gru_packed), act, ws.data_ptr(), ws.numel(), ctypes.byref(final_off), st.cuda_stream))
        else:
            check(train_forward(
                h0.data_ptr(), V, D, T, index.row_ptr.data_ptr(), comp.gather_row.data_ptr(), comp.pair_node.data_ptr(), tro,
                nin.data_ptr(), 1 if use_avg else 0, L, lt, rp, ri, _ptrs(edge_packed), bg, bc, _ptrs(gru_packed), fm, act,
                ws.data_ptr(), ws.numel(), ctypes.byref(final_off), st.cuda_stream))
        off = int(final_off.value)
        final = ws[off:off + V * D * 4].view(torch.float32).view(V, D)
        model.ops['final_node_representations'] = final

        # ---- gated regression + masked loss per task (:220-231, chem_tensorflow.py:158-170) ---------------------------------
        G = int(ph['num_graphs'])
        gnl, gptr = ph['graph_nodes_list'], ph.get('graph_ptr')
        multi = _multitask_readout(model, D)
        saved, loss, dens = (_readout_multi_forward if multi else _readout_per_task_forward)(model, final, h0, gnl, gptr, None, G)

        # data parallelism: the loss is normalised by the mask count of the WHOLE step (parallel.DataParallelContext.global_loss)
        dist = getattr(model, "dist", None)
        sharded = dist is not None and dist.active
        if sharded:
            dist.all_reduce_sum_(dens)
            if multi:
                loss = (saved[-1][:, 0] / (dens + SMALL_NUMBER) * model.task_ratio_factors(dev)).sum()
            else:
                loss = torch.stack([model.ops['loss_numerator_task%i' % t] / (dens[i] + SMALL_NUMBER) *
                                    model.task_ratio(t) for i, t in enumerate(p['task_ids'])]).sum()

        # ---- backward -----------------------------------------------------------------------------------------------------
        opt._flat["g"].zero_()
        gviews = opt.sink_targets()
        d_final = (_readout_multi_backward if multi else _readout_per_task_backward)(model, saved, dens, gviews)
        gv = lambda t: gviews[t.data_ptr()]
        node_heads = ops._ptr(ops.slot_heads(bwd.node_index, bwd.node_index.row_ptr, bwd.node_index.gather_row, V))
        g_edge = _ptrs([gv(model._edge_weight_vars[l]) for l in range(L)])
        if not rnn:
            g_cells = [_ptrs([gv(getattr(c, name)) for c in cells]) for name in ('gates_kernel', 'gates_bias', 'candidate_kernel', 'candidate_bias')]
        if rnn:
            ops._launch("sparse_rnn_train_backward[steps=%d]" % steps, lambda: lib.ggnn_sparse_rnn_train_backward_f32(
                h0.data_ptr(), V, D, T, comp.pair_node.data_ptr(), tro, nin.data_ptr(), 1 if use_avg else 0, L, lt, rp, ri,
                bwd.rows_index.row_ptr.data_ptr(), bwd.rows_index.gather_row.data_ptr(),
                ops._ptr(ops.slot_heads(bwd.rows_index, bwd.rows_index.row_ptr, bwd.rows_index.gather_row, R)),
                bwd.node_index.row_ptr.data_ptr(), bwd.node_index.gather_row.data_ptr(), node_heads,
                bwd.identity.pair_node.data_ptr(), _ptrs(edge_packed_t), _ptrs(rnn_bwd_packed), act, g_edge,
                _ptrs([gv(c.kernel) for c in cells]), _ptrs([gv(c.bias) for c in cells]), d_final.data_ptr(), _ptrs(dstate),
                ws.data_ptr(), ws.numel(), st.cuda_stream, side.cuda_stream))
        elif attention:
            sni = bwd.source_node_index
            mto = (ctypes.c_int64 * (T + 1))(*index.type_off)
            ops._launch("sparse_attn_train_backward[steps=%d]" % steps, lambda: lib.ggnn_sparse_attn_train_backward_f32(
                h0.data_ptr(), V, D, T, M, index.row_ptr.data_ptr(), index.gather_row.data_ptr(), comp.gather_row.data_ptr(),
                index.msg_perm.data_ptr(), mto, comp.pair_node.data_ptr(), tro, nin.data_ptr(), 1 if use_avg else 0, L, lt, rp, ri,
                sni.row_ptr.data_ptr(), sni.gather_row.data_ptr(), sni.msg.data_ptr(), ops.source_slot_rows(index, comp).data_ptr(),
                bwd.node_index.row_ptr.data_ptr(), bwd.node_index.gather_row.data_ptr(), node_heads, bwd.identity.pair_node.data_ptr(),
                _ptrs(edge_packed), _ptrs(edge_packed_t), _ptrs(gru_bwd_packed), factors, act, g_edge,
                _ptrs([gv(a) for a in model.gnn_weights.edge_type_attention_weights]), *g_cells, d_final.data_ptr(), _ptrs(dstate),
                ws.data_ptr(), ws.numel(), st.cuda_stream, side.cuda_stream))
        else:
            check(train_backward(
                h0.data_ptr(), V, D, T, comp.pair_node.data_ptr(), tro, nin.data_ptr(), 1 if use_avg else 0, L, lt, rp, ri,
                bwd.rows_index.row_ptr.data_ptr(), bwd.rows_index.gather_row.data_ptr(),
                ops._ptr(ops.slot_heads(bwd.rows_index, bwd.rows_index.row_ptr, bwd.rows_index.gather_row, R)),
                bwd.node_index.row_ptr.data_ptr(), bwd.node_index.gather_row.data_ptr(), node_heads,
                bwd.identity.pair_node.data_ptr(), _ptrs(edge_packed_t), _ptrs(gru_bwd_packed), act, g_edge, *g_cells,
                d_final.data_ptr(), _ptrs(dstate), ws.data_ptr(), ws.numel(), st.cuda_stream, side.cuda_stream))
        for l, (keep, seed) in enumerate(masks):             # :91 d variable = mask / keep * d masked weights, once per layer
            g = gv(model._edge_weight_vars[l])
            ops.dropout(g, keep, seed, out=g)

        # ---- (all-reduce) -> per-variable clip -> Adam ---------------------------------------------------------------------
        if sharded:
            dist.all_reduce_sum_(opt._flat["g"])
        opt.mark_all_active()
        opt.clip_and_apply(p['clamp_gradient_norm'])
    return loss.detach()


# ---- the dense model (chem_tensorflow_dense.py:93-117) on ggnn_dense_train_forward_f32 / ggnn_dense_train_backward_f32 ---------------
def dense_model_eligible(model) -> bool:
    """The part of `dense_eligible` that depends on the model only: a dense model that asks for the native step
    (params['graph_resident_training'] == 'native'; True keeps the autograd graph-resident route) on a GPU, the fused optimizer over
    exactly the trainable variables, nothing frozen, one-layer readout MLPs, no active data-parallel context."""
    p = getattr(model, "params", None)
    if p is None or p.get('graph_resident_training') != 'native' or not hasattr(model, "_graph_resident_step"):
        return False
    if not torch.cuda.is_available() or torch.device(model.device).type != 'cuda' or not backward.USE_NATIVE_STEP or not p['use_graph']:
        return False
    if not ops.dense_edge_grad_supported(model.num_edge_types, p['hidden_size']) or int(p['num_timesteps']) < 1:
        return False
    dist = getattr(model, "dist", None)
    if dist is not None and dist.active:
        return False
    opt = model.optimizer
    variables = list(model.trainable_variables.values())
    if not (opt.fused and len(opt.vars) == len(variables) and all(a is b for a, b in zip(opt.vars, variables))):
        return False
    have = {v.data_ptr() for v in variables}
    if any(v.data_ptr() not in have for v in model.named_variables().values()):        # (--freeze-graph-model)
        return False
    for task_id in p['task_ids']:
        for kind in ('regression_gate_task%i', 'regression_transform_task%i'):
            if len(model.weights[kind % task_id].params["weights"]) != 1:
                return False
    return True


def dense_eligible(model, batch_data: Dict[str, Any]) -> bool:
    """True when this step of a dense model can run on the native sequences: dense_model_eligible, no per-launch timing, and a batch
    the graph-resident route takes (DenseGGNNChemModel._graph_resident_step: kernels for the shape, no dropout on the propagation)."""
    if ops._timing is not None or not dense_model_eligible(model):
        return False
    h0, A, v = batch_data.get('initial_node_representation'), batch_data.get('adjacency_matrix'), batch_data.get('num_vertices')
    if h0 is None or A is None or v is None or h0.dim() != 3 or A.dim() != 4 or h0.shape[0] == 0:
        return False
    D, E = model.params['hidden_size'], model.num_edge_types
    if h0.dtype != torch.float32 or A.dtype != torch.float32 or tuple(h0.shape[1:]) != (int(v), D) \
            or tuple(A.shape) != (h0.shape[0], E, int(v), int(v)):
        return False
    return model._graph_resident_step(int(v), h0, A, feed=batch_data)


class _DenseWorkspace:
    """One growing device buffer per model: the saved tensors and temporaries of a step (ggnn_dense_train_workspace_bytes)."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None

    def get(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(int(nbytes * 1.05) + 256, dtype=torch.uint8, device=device)
        return self.buf


def native_dense_train_step(model, batch_data: Dict[str, Any]) -> torch.Tensor:
    """native_train_step for the dense model: two C calls for the propagation and every graph-model gradient, the readout + loss
    per task between them, clip + Adam.  No torch.autograd, and in a steady state no read-back."""
    lib = _lib.load()
    p = model.params
    opt = model.optimizer
    model.feed(batch_data)
    ph = model.placeholders
    v = int(ph['num_vertices'])
    D, E, steps = p['hidden_size'], model.num_edge_types, int(p['num_timesteps'])
    h0 = ph['initial_node_representation']
    b = h0.shape[0]
    A_fed = ph['adjacency_matrix']
    st = torch.cuda.current_stream()
    side = backward.side_stream(h0.device)
    dev = h0.device

    with torch.no_grad():
        # ---- operand format of the forward (proven bounds, formats.py; the weights' maxima tracked across optimizer steps) ----
        fmt = model.propagate_format(v, tracked_weights=True)
        # ---- this step's weight images, once per weight version ----
        W = model.weights['edge_weights']
        cell = model.weights['node_gru']
        has_bias = bool(p['use_edge_bias'])
        bias = model.weights['edge_biases'].reshape(E, D) if has_bias else None
        edge_packed = ops.PACKED.dense_edge(W)
        gru_packed = ops.PACKED.dense_gru(cell.gates_kernel, cell.candidate_kernel, D)
        bwd_packed = ops.PACKED.dense_bwd(W, cell.gates_kernel, cell.candidate_kernel)
        nin = model._in_degrees(A_fed, b, v) if has_bias else None
        h0 = h0.reshape(b, v, D).contiguous()
        A = A_fed.contiguous()

        # ---- forward ------------------------------------------------------------------------------------------------------
        if getattr(model, "_native_ws", None) is None:
            model._native_ws = _DenseWorkspace()
        ws = model._native_ws.get(lib.ggnn_dense_train_workspace_bytes(b, v, E, D, steps), dev)
        final_off = ctypes.c_int64(0)
        ops._launch("dense_train_forward[steps=%d]" % steps, lambda: lib.ggnn_dense_train_forward_f32(
            h0.data_ptr(), A.data_ptr(), edge_packed.data_ptr(), gru_packed.data_ptr(), ops._ptr(bias), cell.gates_bias.data_ptr(),
            cell.candidate_bias.data_ptr(), b, v, E, D, steps, int(fmt), ws.data_ptr(), ws.numel(), ctypes.byref(final_off),
            st.cuda_stream))
        off = int(final_off.value)
        final = ws[off:off + b * v * D * 4].view(torch.float32).view(b * v, D)
        model.ops['final_node_representations'] = final.view(b, v, D)

        # ---- gated regression on the real vertices + masked loss per task (chem_tensorflow_dense.py:119-129, chem_tensorflow.py:158-170)
        h0_rows = h0.view(b * v, D)
        gnl, gptr = model._readout_rows(b, v, dev)
        node_mask = ph['node_mask'].reshape(-1).contiguous()
        multi = _multitask_readout(model, D)
        saved, loss, dens = (_readout_multi_forward if multi else _readout_per_task_forward)(model, final, h0_rows, gnl, gptr, node_mask, b)

        # ---- backward -----------------------------------------------------------------------------------------------------
        opt._flat["g"].zero_()
        gviews = opt.sink_targets()
        d_final = (_readout_multi_backward if multi else _readout_per_task_backward)(model, saved, dens, gviews)
        gv = lambda t: gviews[t.data_ptr()].data_ptr()
        ops._launch("dense_train_backward[steps=%d]" % steps, lambda: lib.ggnn_dense_train_backward_f32(
            d_final.data_ptr(), A.data_ptr(), ops._ptr(nin), bwd_packed.data_ptr(), b, v, E, D, steps, gv(W),
            gv(model.weights['edge_biases']) if has_bias else None, gv(cell.gates_kernel), gv(cell.gates_bias),
            gv(cell.candidate_kernel), gv(cell.candidate_bias), ws.data_ptr(), ws.numel(), st.cuda_stream, side.cuda_stream))

        # ---- per-variable clip -> Adam --------------------------------------------------------------------------------------
        opt.mark_all_active()
        opt.clip_and_apply(p['clamp_gradient_norm'])
    return loss.detach()


# ---- the sparse GCN (chem_tensorflow_gcn.py:62-82) on ggnn_gcn_train_forward_f32 / ggnn_gcn_train_backward_f32 ------------------------
def _gcn_native_entries(model):
    """The entry points of the model's native step, chosen once: (launch-name stem, workspace query, forward call, backward call), or
    None when its hidden size has none.  A model on the panel route (params['gcn_panel_layers'] at 128 / 192 / 256 on a GPU,
    gcn_model.gcn_panel_route) takes the ggnn_gcn_panel_train_* family; every other model the ggnn_gcn_train_* family (32 / 64 / 100)."""
    lib = _lib.load()
    D = int(model.params['hidden_size'])
    if model.gcn_panel_route():
        if not lib.ggnn_gcn_panel_train_supported(D):
            return None
        return ("gcn_panel_train", lib.ggnn_gcn_panel_train_workspace_bytes, lib.ggnn_gcn_panel_train_forward_f32,
                lib.ggnn_gcn_panel_train_backward_f32)
    if not lib.ggnn_gcn_train_supported(D):
        return None
    return "gcn_train", lib.ggnn_gcn_train_workspace_bytes, lib.ggnn_gcn_train_forward_f32, lib.ggnn_gcn_train_backward_f32


def gcn_model_eligible(model) -> bool:
    """The part of `gcn_eligible` that depends on the model only: a GCN model that asks for the native step
    (params['native_training'], read with .get: not a key of default_params, whose keys a reference checkpoint must match) on a GPU,
    a hidden size with the fused layer kernels (or, with params['gcn_panel_layers'] too, with the panel kernels: _gcn_native_entries),
    the fused optimizer over exactly the trainable variables, nothing frozen, one-layer readout MLPs, no active data-parallel context."""
    p = getattr(model, "params", None)
    if p is None or not p.get('native_training') or not hasattr(model, "_graph") or 'gcn_use_bias' not in p:
        return False
    if not torch.cuda.is_available() or torch.device(model.device).type != 'cuda' or not backward.USE_NATIVE_STEP or not p['use_graph']:
        return False
    L = int(p['num_timesteps'])
    if L < 1 or L > 64 or _gcn_native_entries(model) is None:
        return False
    dist = getattr(model, "dist", None)
    if dist is not None and dist.active:
        return False
    opt = model.optimizer
    variables = list(model.trainable_variables.values())
    if not (opt.fused and len(opt.vars) == len(variables) and all(a is b for a, b in zip(opt.vars, variables))):
        return False
    have = {v.data_ptr() for v in variables}
    if any(v.data_ptr() not in have for v in model.named_variables().values()):        # (--freeze-graph-model)
        return False
    for task_id in p['task_ids']:
        for kind in ('regression_gate_task%i', 'regression_transform_task%i'):
            if len(model.weights[kind % task_id].params["weights"]) != 1:
                return False
    return True


def gcn_eligible(model, batch_data: Dict[str, Any]) -> bool:
    """True when this step of a GCN model can run on the native sequences: gcn_model_eligible, no per-launch timing, a batch with
    nodes and graphs whose nodes are sorted by graph (the fused readout's condition), and A_hat as a GCNGraph or as the adjacency
    feeds one is built from."""
    if ops._timing is not None or not gcn_model_eligible(model):
        return False
    h0 = batch_data.get('initial_node_representation')
    if h0 is None or not h0.is_cuda or h0.dtype != torch.float32 or h0.dim() != 2 or h0.shape[0] == 0 \
            or h0.shape[1] != model.params['hidden_size']:
        return False
    if batch_data.get('graph_nodes_sorted') is not True or int(batch_data.get('num_graphs') or 0) == 0:
        return False
    keep = float(batch_data.get('graph_state_keep_prob', 1.0))
    if not 0.0 < keep <= 1.0:
        return False
    if batch_data.get('gcn_graph') is None and (batch_data.get('adjacency_list') is None or batch_data.get('adjacency_weights') is None):
        return False
    return True


def native_gcn_train_step(model, batch_data: Dict[str, Any]) -> torch.Tensor:
    """native_train_step for the sparse GCN: two C calls for the layers and every graph-model gradient (the ggnn_gcn_train_* pair, or
    on the panel route the ggnn_gcn_panel_train_* pair: _gcn_native_entries), the readout + loss per task between them, clip + Adam.  No torch.autograd; the dropout masks are the autograd route's (the same seeds and row keys)."""
    p = model.params
    opt = model.optimizer
    stem, workspace_bytes, train_forward, train_backward = _gcn_native_entries(model)
    model.feed(batch_data)
    ph = model.placeholders
    h0 = ph['initial_node_representation'].contiguous()
    V, D = h0.shape
    graph = model._graph()
    if graph.num_nodes != V:
        raise ValueError("initial_node_representation has %d rows, the graph %d nodes" % (V, graph.num_nodes))
    Ws = model.weights['edge_weights']
    bs = model.weights['edge_biases'] if p['gcn_use_bias'] else None
    L = len(Ws)
    keep = float(ph.get('graph_state_keep_prob', 1.0))
    uid = model._node_uid() if keep < 1.0 else None
    seeds = (ctypes.c_uint64 * L)(*[(model.dropout_seed('gcn_state', l) & 0xFFFFFFFFFFFFFFFF) if keep < 1.0 and l < L - 1 else 0
                                    for l in range(L)])
    st = torch.cuda.current_stream()
    side = backward.side_stream(h0.device)
    dev = h0.device

    with torch.no_grad():
        # ---- forward: every weight image in one launch, then the L saving layer launches ---------------------------------------
        if getattr(model, "_native_ws", None) is None:
            model._native_ws = _DenseWorkspace()
        ws = model._native_ws.get(workspace_bytes(V, D, L), dev)
        final_off = ctypes.c_int64(0)
        w_arr, b_arr = _ptrs(Ws), (None if bs is None else _ptrs(bs))
        ops._launch("%s_forward[L=%d]" % (stem, L), lambda: train_forward(
            h0.data_ptr(), V, D, L, graph.row_ptr.data_ptr(), ops._ptr(graph.col), ops._ptr(graph.val), graph.nnz, w_arr, b_arr,
            ops._ptr(uid), seeds, keep, ws.data_ptr(), ws.numel(), ctypes.byref(final_off), st.cuda_stream))
        off = int(final_off.value)
        final = ws[off:off + V * D * 4].view(torch.float32).view(V, D)
        model.ops['final_node_representations'] = final

        # ---- gated regression + masked loss per task (chem_tensorflow_gcn.py:84-93, chem_tensorflow.py:158-170) -----------------
        G = int(ph['num_graphs'])
        gnl, gptr = ph['graph_nodes_list'], ph.get('graph_ptr')
        multi = _multitask_readout(model, D)
        saved, loss, dens = (_readout_multi_forward if multi else _readout_per_task_forward)(model, final, h0, gnl, gptr, None, G)

        # ---- backward -----------------------------------------------------------------------------------------------------
        opt._flat["g"].zero_()
        gviews = opt.sink_targets()
        d_final = (_readout_multi_backward if multi else _readout_per_task_backward)(model, saved, dens, gviews)
        gW_arr = _ptrs([gviews[w.data_ptr()] for w in Ws])
        gb_arr = None if bs is None else _ptrs([gviews[b.data_ptr()] for b in bs])
        ops._launch("%s_backward[L=%d]" % (stem, L), lambda: train_backward(
            d_final.data_ptr(), V, D, L, graph.row_ptr_t.data_ptr(), ops._ptr(graph.col_t), ops._ptr(graph.val_t), graph.nnz,
            ops._ptr(uid), seeds, keep, gW_arr, gb_arr, ws.data_ptr(), ws.numel(), st.cuda_stream, side.cuda_stream))

        # ---- per-variable clip -> Adam --------------------------------------------------------------------------------------
        opt.mark_all_active()
        opt.clip_and_apply(p['clamp_gradient_norm'])
    return loss.detach()
