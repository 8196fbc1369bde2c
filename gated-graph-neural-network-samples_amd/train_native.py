"""The optimisation step on native launch sequences: what chem_tensorflow.py:183-191 runs through sess.run -- forward, gated
regression + masked loss (chem_tensorflow.py:158-170), compute_gradients, per-variable clip_by_norm, Adam -- without torch.autograd
in between.

native_step holds the sequence once: feed -> the route's propagation forward (one C call that saves what the backward needs in
the model's workspace) -> readout + loss, one ops call per task or with params['multitask_readout'] one for all -> the optimizer's
flat gradient zeroed -> readout backward -> the route's propagation backward (one C call; every graph variable's gradient lands in
the optimizer's gradient views) -> (data-parallel all-reduce) -> per-variable clip + Adam.  Per step the host makes those two C
calls, the readout's, a handful of launches for the weight images and masks, and the optimizer's two launches: ~1 ms of host time
instead of the autograd path's ~4.4 ms.  train.train_step takes the first entry of ROUTES whose predicate holds; everything else
keeps the autograd path (backward.PropagationStepFn, variants.py), which is also what every route is tested against.

ROUTES, in dispatch order (config keys are read with .get: none is a key of default_params, whose keys a reference checkpoint must
match):

default    no key.  The sparse GGNN (chem_tensorflow_sparse.py:117-218) with the GRU cell, no attention, no edge bias, state
           keep-prob 1, hidden size 32 / 64 / 100 unpadded, at most two residual inputs per layer.  csrc/ggnn_train.hip:
           ggnn_sparse_train_{prepare,forward,backward}_f32.  The GRU forward's operand format per layer is the range proof's
           (model.gru_formats).  The only route that runs under an active data-parallel context.
attention  compact_attention = 'native' (True keeps variants.CompactAttentionStepFn).  The same model with propagation attention
           on the compacted route (:147-149, 170-196; SparseGGNNChemModel.attention_route).
           ggnn_sparse_attn_train_{forward,backward}_f32: the default's arguments plus the by-target message index and the
           attention factors, whose gradients arrive like every other graph variable's.  Every product exact: the range proof does
           not cover attention-weighted sums.
panel      native_panel_training = True.  The default model at hidden 128 / 192 / 256 unpadded (116, which pads to 128, keeps
           autograd, as do these sizes without the key: backward.PropagationStepFn on the panel kernels).
           ggnn_sparse_train_panel_{prepare,forward,backward}_f32: the same driver on its column-panel route, the default's
           argument lists.
rnn        compact_rnn = 'native' (True keeps variants.CompactRnnStepFn).  The BasicRNNCell on the compacted route
           (graph_rnn_cell = RNN, the R-GCN configuration; SparseGGNNChemModel.rnn_route), every layer's (hidden size, inputs) in
           ops.rnn_fused_supported.  ggnn_sparse_rnn_train_{forward,backward}_f32: the cell's kernel and bias in place of the GRU's
           four arguments.  Every product exact: ReLU states have no bound.  Its weight images come layer by layer from ops.PACKED
           (one entry per weight version): there is no one-launch prepare for this cell.
dense      graph_resident_training = 'native' (True keeps the autograd graph-resident route).  The dense GGNN
           (chem_tensorflow_dense.py:93-117).  csrc/ggnn_dense_train.hip: ggnn_dense_train_{forward,backward}_f32 on cached weight
           images; the readout runs on the real vertices (node_mask).
gcn        native_training = True.  The sparse GCN (chem_tensorflow_gcn.py:62-82).  csrc/ggnn_gcn_train.hip:
           ggnn_gcn_train_{forward,backward}_f32, or with gcn_panel_layers = True at hidden 128 / 192 / 256 their panel twins
           ggnn_gcn_panel_train_{forward,backward}_f32 (_gcn_native_entries); the dropout masks are the autograd route's (the same
           seeds and row keys).
"""
from __future__ import annotations

import ctypes
import functools
import os
from typing import Any, Callable, Dict, NamedTuple, Optional

import torch

from . import _lib, backward, ops
from .utils import SMALL_NUMBER

# the hidden sizes of the column-panel kernels (the panel route: params['native_panel_training'])
PANEL_SIZES = (128, 192, 256)

# all of a step's weight images in one launch (GGNN_FUSED_PREPARE=0: mask / transpose / pack layer by layer through the caches of ops.py)
USE_FUSED_PREPARE = os.environ.get("GGNN_FUSED_PREPARE", "1") != "0"


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


# ---- eligibility: each route's model predicate is its model-kind guard, its own conditions, then _step_eligible -----------------------
def _step_eligible(model) -> bool:
    """What every route asks of a model: the native step switched on, a GPU model that runs its graph layers, the fused optimizer
    over exactly the trainable variables, nothing frozen, one-layer readout MLPs (gate and transform)."""
    p = getattr(model, "params", None)
    if p is None or not backward.USE_NATIVE_STEP or not torch.cuda.is_available() or torch.device(model.device).type != 'cuda' \
            or not p['use_graph']:
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


def _data_parallel(model) -> bool:
    """An active data-parallel context: only the default route reduces across ranks."""
    dist = getattr(model, "dist", None)
    return dist is not None and dist.active


def _sparse_params(model):
    """The params of a sparse GGNN model the compacted native sequences can take whatever its cell -- no edge bias, hidden size
    unpadded, no graph-state dropout, at most 60 layers of at least one timestep each -- or None."""
    p = getattr(model, "params", None)
    if p is None or not hasattr(model, "_edge_weight_vars") or not backward.USE_COMPACT_TRANSFORM:
        return None
    if p['use_edge_bias'] or model._kw != p['hidden_size'] or float(p.get('graph_state_dropout_keep_prob', 1.0)) < 1.0:
        return None
    if len(p['layer_timesteps']) > 60 or any(int(s) < 1 for s in p['layer_timesteps']):
        return None
    return p


def _fan_ins(p):
    """Inputs of each layer's cell: its residual inputs + the aggregated messages."""
    return [len(p['residual_connections'].get(str(l)) or []) + 1 for l in range(len(p['layer_timesteps']))]


def _gru_cell(model) -> bool:
    return getattr(model, "cell_type", None) == 'gru'


def _whole_block_eligible(p) -> bool:
    """The GRU that gathers the segment sum in the kernel, switched on, at a hidden size that has it (32 / 64 / 100) with the
    compacted transform and the single-launch backward, and every layer's fan-in within that kernel's."""
    D = p['hidden_size']
    return bool(backward.TRAIN_GATHER_IN_GRU) and ops.gru_gather_fused(D) and ops.compact_supported(D) and D <= 104 \
        and ops.gru_bwd_is_fused(D) and all(nx <= ops.GRU_FUSED_MAX_INPUTS for nx in _fan_ins(p))


def model_eligible(model) -> bool:
    """The part of `eligible` that depends on the model only (run_epoch uses it to choose how batches are prefetched): the default
    route's model of the module docstring.  An active data-parallel context is fine."""
    p = _sparse_params(model)
    if p is None or not _gru_cell(model) or p['use_propagation_attention'] or not _whole_block_eligible(p):
        return False
    return _step_eligible(model)


def attn_model_eligible(model) -> bool:
    """The part of `attn_eligible` that depends on the model only: a sparse model whose config asks for the native step with
    params['compact_attention'] == 'native' (True keeps the autograd step) and whose attention runs on the compacted route
    (attention_route()), under the default model's conditions otherwise, and no active data-parallel context."""
    p = _sparse_params(model)
    if p is None or not _gru_cell(model) or not p['use_propagation_attention']:
        return False
    if p.get('compact_attention') != 'native' or not model.attention_route() or _data_parallel(model) or not _whole_block_eligible(p):
        return False
    return _step_eligible(model)


def panel_model_eligible(model) -> bool:
    """The part of `panel_eligible` that depends on the model only: a sparse model whose config asks for the native step at the
    column-panel sizes with params['native_panel_training'] and whose hidden size is 128 / 192 / 256 unpadded, under the default
    model's conditions otherwise (the GRU's place of the segment sum aside: the panel kernels have one, whatever
    TRAIN_GATHER_IN_GRU says), and no active data-parallel context."""
    p = _sparse_params(model)
    if p is None or not _gru_cell(model) or p['use_propagation_attention'] or not p.get('native_panel_training') or _data_parallel(model):
        return False
    D = p['hidden_size']
    if D not in PANEL_SIZES or not _lib.load().ggnn_sparse_train_panel_supported(D) or not ops.compact_supported(D) \
            or not ops.gru_bwd_is_fused(D) or any(nx > ops.GRU_FUSED_MAX_INPUTS for nx in _fan_ins(p)):
        return False
    return _step_eligible(model)


def rnn_model_eligible(model) -> bool:
    """The part of `rnn_eligible` that depends on the model only: a sparse model whose config asks for the native step with
    params['compact_rnn'] == 'native' (True keeps the autograd step) and whose BasicRNNCell runs on the compacted route
    (rnn_route()), every layer's (hidden size, inputs) in ops.rnn_fused_supported -- 32 / 64 with at most two residual inputs, 100
    with none -- and no active data-parallel context."""
    p = _sparse_params(model)
    if p is None or not hasattr(model, "rnn_route"):
        return False
    if p.get('compact_rnn') != 'native' or not model.rnn_route() or _data_parallel(model):
        return False
    if any(not ops.rnn_fused_supported(p['hidden_size'], nx) for nx in _fan_ins(p)):
        return False
    return _step_eligible(model)


def dense_model_eligible(model) -> bool:
    """The part of `dense_eligible` that depends on the model only: a dense model that asks for the native step
    (params['graph_resident_training'] == 'native'; True keeps the autograd graph-resident route), kernels for its edge types and
    hidden size, at least one timestep, no active data-parallel context."""
    p = getattr(model, "params", None)
    if p is None or not hasattr(model, "_graph_resident_step") or p.get('graph_resident_training') != 'native':
        return False
    if not ops.dense_edge_grad_supported(model.num_edge_types, p['hidden_size']) or int(p['num_timesteps']) < 1 or _data_parallel(model):
        return False
    return _step_eligible(model)


def _gcn_native_entries(model):
    """The entry points of the model's native step: (launch-name stem, workspace query, forward call, backward call), or None when
    its hidden size has none.  A model on the panel route (params['gcn_panel_layers'] at 128 / 192 / 256 on a GPU,
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
    (params['native_training']), 1 .. 64 layers, a hidden size with the fused layer kernels (or, with params['gcn_panel_layers'] too,
    with the panel kernels: _gcn_native_entries), no active data-parallel context."""
    p = getattr(model, "params", None)
    if p is None or not hasattr(model, "_graph") or 'gcn_use_bias' not in p or not p.get('native_training'):
        return False
    if not 1 <= int(p['num_timesteps']) <= 64 or _gcn_native_entries(model) is None or _data_parallel(model):
        return False
    return _step_eligible(model)


def _sparse_batch_eligible(model, batch_data: Dict[str, Any]) -> bool:
    """A batch the sparse native sequences take: on the GPU, sorted by graph, at least one message, no graph-state dropout."""
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


def eligible(model, batch_data: Dict[str, Any]) -> bool:
    """True when this step can run on the default route: model_eligible, no per-launch timing, and a batch on the GPU, sorted by
    graph, with at least one message."""
    return ops._timing is None and model_eligible(model) and _sparse_batch_eligible(model, batch_data)


def attn_eligible(model, batch_data: Dict[str, Any]) -> bool:
    """True when this step of a model with propagation attention can run on the attention route: attn_model_eligible, no
    per-launch timing, and a batch as for `eligible`."""
    return ops._timing is None and attn_model_eligible(model) and _sparse_batch_eligible(model, batch_data)


def panel_eligible(model, batch_data: Dict[str, Any]) -> bool:
    """True when this step of the default model at hidden size 128 / 192 / 256 can run on the panel route: panel_model_eligible,
    no per-launch timing, and a batch as for `eligible`."""
    return ops._timing is None and panel_model_eligible(model) and _sparse_batch_eligible(model, batch_data)


def rnn_eligible(model, batch_data: Dict[str, Any]) -> bool:
    """True when this step of a model with the BasicRNNCell can run on the rnn route: rnn_model_eligible, no per-launch timing,
    and a batch as for `eligible`."""
    return ops._timing is None and rnn_model_eligible(model) and _sparse_batch_eligible(model, batch_data)


def dense_eligible(model, batch_data: Dict[str, Any]) -> bool:
    """True when this step of a dense model can run on the dense route: dense_model_eligible, no per-launch timing, and a batch
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


def gcn_eligible(model, batch_data: Dict[str, Any]) -> bool:
    """True when this step of a GCN model can run on the gcn route: gcn_model_eligible, no per-launch timing, a batch with nodes and
    graphs whose nodes are sorted by graph (the fused readout's condition), and A_hat as a GCNGraph or as the adjacency feeds one is
    built from."""
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


# ---- what the propagation pairs share ----------------------------------------------------------------------------------------------------
class _Workspace:
    """One growing device buffer per model: the saved tensors and temporaries of a step (the route's *_workspace_bytes) and, for the
    sparse routes, the layer-input gradient accumulators.  Allocated on the training stream, reused by every step."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None
        self.dstate: Optional[torch.Tensor] = None

    def get(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(int(nbytes * 1.05) + 256, dtype=torch.uint8, device=device)
        return self.buf

    def layer_gradients(self, L: int, V: int, D: int, device):
        if self.dstate is None or self.dstate.numel() < L * V * D or self.dstate.device != device:
            self.dstate = torch.empty(int(L * V * D * 1.05) + 64, dtype=torch.float32, device=device)
        return [self.dstate[l * V * D:(l + 1) * V * D].view(V, D) for l in range(L)]


def _workspace(model) -> _Workspace:
    if getattr(model, "_native_ws", None) is None:
        model._native_ws = _Workspace()
    return model._native_ws


def _final(ws: torch.Tensor, final_off, rows: int, D: int) -> torch.Tensor:
    """The final node representations the forward call left in the workspace, as a [rows, D] view."""
    off = int(final_off.value)
    return ws[off:off + rows * D * 4].view(torch.float32).view(rows, D)


class _SparseStep:
    """What the four sparse routes' calls share, built once per step from the fed batch: the message index with its compacted
    sources and backward indices, the argument runs every C call of theirs has in common, the streams, this step's weight-dropout
    masks, and (workspace) the step's buffers."""

    def __init__(self, model):
        p, ph = model.params, model.placeholders
        self.h0 = h0 = ph['initial_node_representation'].contiguous()
        self.V, self.D = V, D = h0.shape
        self.T = T = model.num_edge_types
        self.L = L = len(p['layer_timesteps'])
        self.steps = int(sum(p['layer_timesteps']))
        self.index = index = ph['message_index']
        comp = getattr(index, "_compact", None)
        if comp is None or getattr(comp, "_bwd", None) is None:
            ops.prepare_message_index(index, D, True, training=True)
            comp = index._compact
        self.comp = comp
        self.bwd = ops.compact_backward(index, comp)
        self.R, self.M = comp.num_rows, index.num_messages
        self.act = ops.ACT_IDS[p['graph_rnn_activation'].lower()]
        residuals = [[int(i) for i in (p['residual_connections'].get(str(l)) or [])] for l in range(L)]
        res_ptr, res_idx = [0], []
        for r in residuals:
            res_idx.extend(r)
            res_ptr.append(len(res_idx))
        self.nxs = [len(r) + 1 for r in residuals]
        # the argument runs: (h0, V, D, T) and (pair_node, type_row_off, nin, use_avg, L, layer_timesteps, res_ptr, res_idx)
        self.shape = (h0.data_ptr(), V, D, T)
        self.layers = (comp.pair_node.data_ptr(), (ctypes.c_int64 * (T + 1))(*comp.type_row_off),
                       ph['num_incoming_edges_per_type'].data_ptr(), 1 if p['use_edge_msg_avg_aggregation'] else 0, L,
                       _i32(p['layer_timesteps']), _i32(res_ptr), _i32(res_idx))
        self.stream = torch.cuda.current_stream().cuda_stream
        self.side = backward.side_stream(h0.device).cuda_stream
        # this step's masked edge weights (:91): one mask per layer and step
        self.ew_keep = ew_keep = float(ph.get('edge_weight_dropout_keep_prob', 1.0))
        self.masks = [(ew_keep, model.dropout_seed('edge_weights', l)) for l in range(L)] if ew_keep < 1.0 else []
        self.cells = model.gnn_weights.rnn_cells
        self.final_off = ctypes.c_int64(0)

    def workspace(self, model, nbytes: int, what: str = ""):
        if not nbytes:
            raise ValueError("native training step%s: no workspace for V=%d D=%d T=%d rows=%d steps=%d" % (
                what, self.V, self.D, self.T, self.R, self.steps))
        ws = _workspace(model)
        self.ws = ws.get(nbytes, self.h0.device)
        self.dstate = ws.layer_gradients(self.L, self.V, self.D, self.h0.device)

    def saving(self):
        """The tail of a forward call: activation, workspace, where it left `final`, stream."""
        return self.act, self.ws.data_ptr(), self.ws.numel(), ctypes.byref(self.final_off), self.stream

    def outputs(self, model):
        """What a route's forward returns to native_step."""
        ph = model.placeholders
        return (self, _final(self.ws, self.final_off, self.V, self.D), self.h0, ph['graph_nodes_list'], ph.get('graph_ptr'), None,
                int(ph['num_graphs']))

    def sums(self, index, segments: int):
        """(row_ptr, gather_row, slot heads) of a backward segment sum."""
        return index.row_ptr.data_ptr(), index.gather_row.data_ptr(), ops._ptr(ops.slot_heads(index, index.row_ptr, index.gather_row, segments))

    def gradients(self, d_final):
        """The tail of a backward call: d_final, the layer-input gradient accumulators, workspace, streams."""
        return d_final.data_ptr(), ops._ptr_array(self.dstate), self.ws.data_ptr(), self.ws.numel(), self.stream, self.side

    def unmask_edge_gradients(self, model, gv):
        for l, (keep, seed) in enumerate(self.masks):        # :91 d variable = mask / keep * d masked weights, once per layer
            g = gv(model._edge_weight_vars[l])
            ops.dropout(g, keep, seed, out=g)


def _layer_images(model, s: _SparseStep, pack_cell: Callable, pack_cell_bwd: Callable):
    """(edge, transposed edge, cell forward, cell backward) images per layer, mask / transpose / pack layer by layer through the
    version-keyed cache (ops.PACKED): the images of the autograd route's launches, bit for bit.  pack_cell(l, cell, nx) /
    pack_cell_bwd(l, cell, nx) are the cell's two packers."""
    edge, edge_t, cell, cell_bwd = [], [], [], []
    for l in range(s.L):
        W = model._edge_weight_vars[l].view(s.T, s.D, s.D)
        if s.masks:
            W = backward.masked(W, s.masks[l][0], s.masks[l][1])
        edge.append(ops.PACKED.edge(W))
        edge_t.append(ops.PACKED.edge_t(W))
        cell.append(pack_cell(l, s.cells[l], s.nxs[l]))
        cell_bwd.append(pack_cell_bwd(l, s.cells[l], s.nxs[l]))
    return edge, edge_t, cell, cell_bwd


def _gru_images(model, s: _SparseStep, fmts, prepare):
    """The step's images for the GRU cell in the layers' operand formats `fmts`: all ~120 of them in ONE launch of `prepare`
    (ggnn_sparse_train_prepare_f32 or its panel twin), the weight-dropout mask applied on the fly; beyond its 16 layers, or with
    USE_FUSED_PREPARE off, layer by layer."""
    D, L = s.D, s.L
    if L > 16 or not USE_FUSED_PREPARE:
        return _layer_images(model, s, lambda l, c, nx: ops.PACKED.gru(c.gates_kernel, c.candidate_kernel, nx, D, fmts[l]),
                             lambda l, c, nx: ops.PACKED.gru_bwd(c.gates_kernel, c.candidate_kernel, nx, D))
    imgs = getattr(model, "_native_images", None)
    if imgs is None:
        lib = _lib.load()
        f32 = lambda nbytes: torch.empty(nbytes // 4, dtype=torch.float32, device=s.h0.device)
        eb = lib.ggnn_msg_transform_compact_workspace_bytes(D, s.T)
        imgs = model._native_images = (
            [f32(eb) for _ in range(L)], [f32(eb) for _ in range(L)],
            [f32(lib.ggnn_gru_packed_bytes(D, s.nxs[l])) for l in range(L)],
            [f32(lib.ggnn_gru_bwd_packed_bytes(D, s.nxs[l])) for l in range(L)])
    seeds = (ctypes.c_uint64 * L)(*[m[1] for m in s.masks]) if s.masks else None
    P = ops._ptr_array
    ops._launch("sparse_train_prepare[L=%d]" % L, lambda: prepare(
        L, s.T, D, _i32(s.nxs), P(model._edge_weight_vars), s.ew_keep if s.masks else 1.0, seeds,
        P([c.gates_kernel for c in s.cells]), P([c.candidate_kernel for c in s.cells]), _i32(fmts), *[P(i) for i in imgs], s.stream))
    return imgs


def _gru_biases(s: _SparseStep):
    return ops._ptr_array([c.gates_bias for c in s.cells]), ops._ptr_array([c.candidate_bias for c in s.cells])


def _graph_gradients(model, s: _SparseStep, gv, cell_variables):
    """The optimizer's gradient views of the edge weights and of each named variable of the cells, as pointer arrays per layer."""
    return [ops._ptr_array([gv(W) for W in model._edge_weight_vars])] + \
        [ops._ptr_array([gv(getattr(c, name)) for c in s.cells]) for name in cell_variables]


GRU_VARIABLES = ('gates_kernel', 'gates_bias', 'candidate_kernel', 'candidate_bias')


# ---- default and panel: one pair, parameterised by the entry-point family of csrc/ggnn_train.hip ------------------------------------------
class _GruEntries(NamedTuple):
    stem: str                   # of the launch names
    prepare: str                # the library's symbols
    workspace_bytes: str
    forward: str
    backward: str


WHOLE_BLOCK = _GruEntries("sparse_train", "ggnn_sparse_train_prepare_f32", "ggnn_sparse_train_workspace_bytes",
                          "ggnn_sparse_train_forward_f32", "ggnn_sparse_train_backward_f32")             # hidden 32 / 64 / 100
COLUMN_PANEL = _GruEntries("sparse_train_panel", "ggnn_sparse_train_panel_prepare_f32", "ggnn_sparse_train_panel_workspace_bytes",
                           "ggnn_sparse_train_panel_forward_f32", "ggnn_sparse_train_panel_backward_f32")  # hidden 128 / 192 / 256


def _gru_forward(entries: _GruEntries, model):
    lib = _lib.load()
    s = _SparseStep(model)
    # operand format of each layer's GRU forward: two-piece f16 only where this step's operands are provably in its range
    # (formats.py: max|h0|, the weights' maxima tracked across optimizer steps, tanh cell, mean aggregation), else exact bf16x3
    fmts = model.gru_formats(s.h0, s.ew_keep, 1.0, training=True)
    edge, s.edge_t, gru, s.cell_bwd = _gru_images(model, s, fmts, getattr(lib, entries.prepare))
    s.workspace(model, getattr(lib, entries.workspace_bytes)(s.V, s.D, s.T, s.R, s.steps))
    forward, P = getattr(lib, entries.forward), ops._ptr_array
    ops._launch("%s_forward[steps=%d]" % (entries.stem, s.steps), lambda: forward(
        *s.shape, s.index.row_ptr.data_ptr(), s.comp.gather_row.data_ptr(), *s.layers, P(edge), *_gru_biases(s), P(gru), _i32(fmts),
        *s.saving()))
    return s.outputs(model)


def _gru_backward(entries: _GruEntries, model, s: _SparseStep, d_final, gv):
    train_backward, P = getattr(_lib.load(), entries.backward), ops._ptr_array
    g = _graph_gradients(model, s, gv, GRU_VARIABLES)
    ops._launch("%s_backward[steps=%d]" % (entries.stem, s.steps), lambda: train_backward(
        *s.shape, *s.layers, *s.sums(s.bwd.rows_index, s.R), *s.sums(s.bwd.node_index, s.V), s.bwd.identity.pair_node.data_ptr(), P(s.edge_t),
        P(s.cell_bwd), s.act, *g, *s.gradients(d_final)))
    s.unmask_edge_gradients(model, gv)


# ---- attention: the GRU pair's arguments plus the by-target message index and the attention factors ----------------------------------------
def _attn_forward(model):
    lib = _lib.load()
    s = _SparseStep(model)
    # (the range proof does not cover attention-weighted sums: every product exact; gru_formats records that on the model)
    model.gru_formats(s.h0, s.ew_keep, 1.0, training=True)
    s.edge, s.edge_t, gru, s.cell_bwd = _gru_images(model, s, [ops.GRU_FMT_EXACT] * s.L, lib.ggnn_sparse_train_prepare_f32)
    s.workspace(model, lib.ggnn_sparse_attn_train_workspace_bytes(s.V, s.D, s.T, s.R, s.steps, s.M), ", attention")
    P = ops._ptr_array
    s.factors = P(model.gnn_weights.edge_type_attention_weights)
    ops._launch("sparse_attn_train_forward[steps=%d]" % s.steps, lambda: lib.ggnn_sparse_attn_train_forward_f32(
        *s.shape, s.M, s.index.row_ptr.data_ptr(), s.index.gather_row.data_ptr(), s.comp.gather_row.data_ptr(), *s.layers, P(s.edge),
        s.factors, *_gru_biases(s), P(gru), *s.saving()))
    return s.outputs(model)


def _attn_backward(model, s: _SparseStep, d_final, gv):
    lib, index, sni, P = _lib.load(), s.index, s.bwd.source_node_index, ops._ptr_array
    g = _graph_gradients(model, s, gv, GRU_VARIABLES)
    mto = (ctypes.c_int64 * (s.T + 1))(*index.type_off)
    ops._launch("sparse_attn_train_backward[steps=%d]" % s.steps, lambda: lib.ggnn_sparse_attn_train_backward_f32(
        *s.shape, s.M, index.row_ptr.data_ptr(), index.gather_row.data_ptr(), s.comp.gather_row.data_ptr(), index.msg_perm.data_ptr(), mto,
        *s.layers, sni.row_ptr.data_ptr(), sni.gather_row.data_ptr(), sni.msg.data_ptr(), ops.source_slot_rows(index, s.comp).data_ptr(),
        *s.sums(s.bwd.node_index, s.V), s.bwd.identity.pair_node.data_ptr(), P(s.edge), P(s.edge_t), P(s.cell_bwd), s.factors, s.act, g[0],
        P([gv(a) for a in model.gnn_weights.edge_type_attention_weights]), *g[1:], *s.gradients(d_final)))
    s.unmask_edge_gradients(model, gv)


# ---- rnn: the BasicRNNCell's kernel and bias in place of the GRU's four arguments ---------------------------------------------------------
def _rnn_forward(model):
    lib = _lib.load()
    s = _SparseStep(model)
    D, P = s.D, ops._ptr_array
    # (every product exact: ReLU states have no bound)
    edge, s.edge_t, rnn, s.cell_bwd = _layer_images(model, s, lambda l, c, nx: ops.PACKED.rnn(c.kernel, nx, D),
                                                    lambda l, c, nx: ops.PACKED.rnn_bwd(c.kernel, nx, D))
    s.workspace(model, lib.ggnn_sparse_rnn_train_workspace_bytes(s.V, D, s.T, s.R, s.steps), ", RNN cell")
    ops._launch("sparse_rnn_train_forward[steps=%d]" % s.steps, lambda: lib.ggnn_sparse_rnn_train_forward_f32(
        *s.shape, s.M, s.index.row_ptr.data_ptr(), s.comp.gather_row.data_ptr(), *s.layers, P(edge), P([c.bias for c in s.cells]), P(rnn),
        *s.saving()))
    return s.outputs(model)


def _rnn_backward(model, s: _SparseStep, d_final, gv):
    lib, P = _lib.load(), ops._ptr_array
    g = _graph_gradients(model, s, gv, ('kernel', 'bias'))
    ops._launch("sparse_rnn_train_backward[steps=%d]" % s.steps, lambda: lib.ggnn_sparse_rnn_train_backward_f32(
        *s.shape, *s.layers, *s.sums(s.bwd.rows_index, s.R), *s.sums(s.bwd.node_index, s.V), s.bwd.identity.pair_node.data_ptr(), P(s.edge_t),
        P(s.cell_bwd), s.act, *g, *s.gradients(d_final)))
    s.unmask_edge_gradients(model, gv)


# ---- dense: csrc/ggnn_dense_train.hip on cached weight images ------------------------------------------------------------------------------
def _dense_forward(model):
    lib = _lib.load()
    p, ph = model.params, model.placeholders
    v = int(ph['num_vertices'])
    D, E, steps = p['hidden_size'], model.num_edge_types, int(p['num_timesteps'])
    h0 = ph['initial_node_representation']
    b = h0.shape[0]
    A_fed = ph['adjacency_matrix']
    stream = torch.cuda.current_stream().cuda_stream
    side = backward.side_stream(h0.device).cuda_stream
    # operand format of the forward (proven bounds, formats.py; the weights' maxima tracked across optimizer steps)
    fmt = model.propagate_format(v, tracked_weights=True)
    # this step's weight images, once per weight version
    W = model.weights['edge_weights']
    cell = model.weights['node_gru']
    bias = model.weights['edge_biases'] if p['use_edge_bias'] else None
    edge_packed = ops.PACKED.dense_edge(W)
    gru_packed = ops.PACKED.dense_gru(cell.gates_kernel, cell.candidate_kernel, D)
    bwd_packed = ops.PACKED.dense_bwd(W, cell.gates_kernel, cell.candidate_kernel)
    nin = model._in_degrees(A_fed, b, v) if bias is not None else None
    h0 = h0.reshape(b, v, D).contiguous()
    A = A_fed.contiguous()
    ws = _workspace(model).get(lib.ggnn_dense_train_workspace_bytes(b, v, E, D, steps), h0.device)
    final_off = ctypes.c_int64(0)
    ops._launch("dense_train_forward[steps=%d]" % steps, lambda: lib.ggnn_dense_train_forward_f32(
        h0.data_ptr(), A.data_ptr(), edge_packed.data_ptr(), gru_packed.data_ptr(), ops._ptr(None if bias is None else bias.reshape(E, D)),
        cell.gates_bias.data_ptr(), cell.candidate_bias.data_ptr(), b, v, E, D, steps, int(fmt), ws.data_ptr(), ws.numel(),
        ctypes.byref(final_off), stream))
    # the readout runs on the real vertices (chem_tensorflow_dense.py:119-129)
    gnl, gptr = model._readout_rows(b, v, h0.device)
    state = (A, nin, bwd_packed, (b, v, E, D, steps), W, bias, cell, ws, stream, side)
    return state, _final(ws, final_off, b * v, D), h0.view(b * v, D), gnl, gptr, ph['node_mask'].reshape(-1).contiguous(), b


def _dense_backward(model, state, d_final, gv):
    A, nin, bwd_packed, shape, W, bias, cell, ws, stream, side = state
    g = lambda t: gv(t).data_ptr()
    ops._launch("dense_train_backward[steps=%d]" % shape[-1], lambda: _lib.load().ggnn_dense_train_backward_f32(
        d_final.data_ptr(), A.data_ptr(), ops._ptr(nin), bwd_packed.data_ptr(), *shape, g(W), None if bias is None else g(bias),
        g(cell.gates_kernel), g(cell.gates_bias), g(cell.candidate_kernel), g(cell.candidate_bias), ws.data_ptr(), ws.numel(),
        stream, side))


# ---- gcn: csrc/ggnn_gcn_train.hip, every weight image in the forward's first launch, then the L saving layer launches ---------------------
def _gcn_forward(model):
    p, ph = model.params, model.placeholders
    stem, workspace_bytes, train_forward, train_backward = _gcn_native_entries(model)
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
    stream = torch.cuda.current_stream().cuda_stream
    side = backward.side_stream(h0.device).cuda_stream
    ws = _workspace(model).get(workspace_bytes(V, D, L), h0.device)
    final_off = ctypes.c_int64(0)
    w_arr, b_arr = ops._ptr_array(Ws), ops._ptr_array(bs)
    ops._launch("%s_forward[L=%d]" % (stem, L), lambda: train_forward(
        h0.data_ptr(), V, D, L, graph.row_ptr.data_ptr(), ops._ptr(graph.col), ops._ptr(graph.val), graph.nnz, w_arr, b_arr,
        ops._ptr(uid), seeds, keep, ws.data_ptr(), ws.numel(), ctypes.byref(final_off), stream))
    state = ("%s_backward[L=%d]" % (stem, L), train_backward, (V, D, L), graph, uid, seeds, keep, Ws, bs, ws, stream, side)
    return state, _final(ws, final_off, V, D), h0, ph['graph_nodes_list'], ph.get('graph_ptr'), None, int(ph['num_graphs'])


def _gcn_backward(model, state, d_final, gv):
    name, train_backward, shape, graph, uid, seeds, keep, Ws, bs, ws, stream, side = state
    gW_arr = ops._ptr_array([gv(w) for w in Ws])
    gb_arr = None if bs is None else ops._ptr_array([gv(b) for b in bs])
    ops._launch(name, lambda: train_backward(
        d_final.data_ptr(), *shape, graph.row_ptr_t.data_ptr(), ops._ptr(graph.col_t), ops._ptr(graph.val_t), graph.nnz,
        ops._ptr(uid), seeds, keep, gW_arr, gb_arr, ws.data_ptr(), ws.numel(), stream, side))


# ---- the table and the step -----------------------------------------------------------------------------------------------------------------
class Route(NamedTuple):
    name: str
    model_eligible: Callable[[Any], bool]                       # the model alone (how run_epoch prefetches batches)
    eligible: Callable[[Any, Dict[str, Any]], bool]             # model + batch: what train.train_step asks, per step
    # forward(model) -> (state, final [rows, D] in the workspace, h0 [rows, D], graph_nodes_list, graph_ptr, node_mask, G)
    forward: Callable
    # backward(model, state, d_final, gv): every graph variable's gradient into gv(variable), the optimizer's view of it
    backward: Callable


ROUTES = (
    Route("default", model_eligible, eligible, functools.partial(_gru_forward, WHOLE_BLOCK), functools.partial(_gru_backward, WHOLE_BLOCK)),
    Route("attention", attn_model_eligible, attn_eligible, _attn_forward, _attn_backward),
    Route("panel", panel_model_eligible, panel_eligible, functools.partial(_gru_forward, COLUMN_PANEL),
          functools.partial(_gru_backward, COLUMN_PANEL)),
    Route("rnn", rnn_model_eligible, rnn_eligible, _rnn_forward, _rnn_backward),
    Route("dense", dense_model_eligible, dense_eligible, _dense_forward, _dense_backward),
    Route("gcn", gcn_model_eligible, gcn_eligible, _gcn_forward, _gcn_backward),
)


def native_step(route: Route, model, batch_data: Dict[str, Any]) -> torch.Tensor:
    """One optimisation step of `model` on `route` (whose predicate the caller has asked): see the module docstring.  No
    torch.autograd, and in a steady state no read-back."""
    p = model.params
    opt = model.optimizer
    model.feed(batch_data)
    with torch.no_grad():
        state, final, h0, gnl, gptr, node_mask, G = route.forward(model)
        D = final.shape[1]
        model.ops['final_node_representations'] = final.view(model.placeholders['initial_node_representation'].shape)  # (dense: [b, v, D])

        # ---- gated regression + masked loss (chem_tensorflow.py:158-170), per task or all tasks at once ----------------------------
        multi = _multitask_readout(model, D)
        saved, loss, dens = (_readout_multi_forward if multi else _readout_per_task_forward)(model, final, h0, gnl, gptr, node_mask, G)

        # data parallelism: the loss is normalised by the mask count of the WHOLE step (parallel.DataParallelContext.global_loss)
        sharded = _data_parallel(model)
        if sharded:
            model.dist.all_reduce_sum_(dens)
            if multi:
                loss = (saved[-1][:, 0] / (dens + SMALL_NUMBER) * model.task_ratio_factors(final.device)).sum()
            else:
                loss = torch.stack([model.ops['loss_numerator_task%i' % t] / (dens[i] + SMALL_NUMBER) *
                                    model.task_ratio(t) for i, t in enumerate(p['task_ids'])]).sum()

        # ---- backward: the readout's, then the propagation's, into the optimizer's flat gradient -------------------------------------
        opt._flat["g"].zero_()
        gviews = opt.sink_targets()
        d_final = (_readout_multi_backward if multi else _readout_per_task_backward)(model, saved, dens, gviews)
        route.backward(model, state, d_final, lambda t: gviews[t.data_ptr()])

        # ---- (all-reduce) -> per-variable clip -> Adam -------------------------------------------------------------------------------
        if sharded:
            model.dist.all_reduce_sum_(opt._flat["g"])
        opt.mark_all_active()
        opt.clip_and_apply(p['clamp_gradient_norm'])
    return loss.detach()
