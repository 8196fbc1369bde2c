"""DenseGGNNChemModel -- host-side mirror of chem_tensorflow_dense.py:51-265 on PyTorch-ROCm tensors.

Per timestep (chem_tensorflow_dense.py:100-115):
    m_e  = h W_e (+ b_e)          for all e: ONE FP32-MFMA GEMM [b*v,D]x[D,e*D]  (ggnn_msg_transform_f32)
    acts = sum_e A_e m_e          batched [v,v]x[v,D] from LDS                   (ggnn_dense_aggregate_f32)
    h    = GRU(acts, h)           one GRU shared by all timesteps (:101-102)     (ggnn_gru_f32)
Inference / validation runs all timesteps in one graph-resident launch (ggnn_dense_propagate_f32).  Training runs the dense step as
the sparse step it is on the b*v padded nodes (_compute_for_training: the hand-written backward of backward.PropagationStepFn), or,
with params['graph_resident_training'], on the graph-resident forward and backward launches (backward.DensePropagateFn); with the
value 'native' of that key the whole optimisation step is two native calls without torch.autograd (train_native.ROUTES, entry `dense`).
With params['pack_on_device'] the batches are assembled on the GPU from the resident dataset (ggnn_dense_assemble_batch), training
batches together with that sparse form.
"""
from __future__ import annotations

from collections import defaultdict
from typing import Any, Dict, Sequence

import numpy as np
import torch

from . import formats, ops
from .chem_model import ChemModel
from .data import DENSE_BUCKET_SIZES, MoleculeSet, pack_dense_batch
from .sparse_model import GRUCellWeights
from .utils import glorot_init, tf_dropout, tf_glorot_uniform

import os

# Inference with all timesteps in one graph-resident launch (GGNN_DENSE_GRAPH_KERNEL=0: three launches per timestep)
USE_GRAPH_RESIDENT_KERNEL = os.environ.get("GGNN_DENSE_GRAPH_KERNEL", "1") != "0"


class DenseGGNNChemModel(ChemModel):
    def __init__(self, args):
        super().__init__(args)

    @classmethod
    def default_params(cls):
        # chem_tensorflow_dense.py:57-66
        params = dict(super().default_params())
        params.update({
            'batch_size': 256,
            'graph_state_dropout_keep_prob': 1.,
            'task_sample_ratios': {},
            'use_edge_bias': True,
            'edge_weight_dropout_keep_prob': 1
        })
        # (params['pack_on_device'] and params['graph_resident_training'], default False, are read with .get: a key in this dict would
        # break restoring the reference's checkpoints, whose params must match key for key, chem_tensorflow.py:336-340)
        return params

    def prepare_specific_graph_model(self) -> None:
        """chem_tensorflow_dense.py:68-91.
        params['pack_on_device'] (default False): batches are assembled on the GPU from the resident dataset
        (DeviceMoleculeSet.dense_tables, ggnn_dense_assemble_batch) instead of packed in NumPy and uploaded -- the same feeds bit for
        bit; a training feed also carries the sparse form its step needs ('_sparse_form').  Needs a CUDA/HIP device."""
        if self.params.get('pack_on_device') and torch.device(self.device).type != 'cuda':
            raise ValueError("pack_on_device=True assembles batches on the GPU; device %r is not a CUDA/HIP device" % (str(self.device),))
        h_dim = self.params['hidden_size']
        for name in ('initial_node_representation', 'node_mask', 'num_vertices', 'adjacency_matrix'):
            self.placeholders[name] = None
        self.placeholders['graph_state_keep_prob'] = 1.0
        self.placeholders['edge_weight_dropout_keep_prob'] = 1.0
        dev = self.device
        # :84 glorot over the last two dims of [e,h,h]
        self.weights['edge_weights'] = torch.from_numpy(glorot_init([self.num_edge_types, h_dim, h_dim])).to(dev)
        if self.params['use_edge_bias']:
            self.weights['edge_biases'] = torch.zeros([self.num_edge_types, 1, h_dim], dtype=torch.float32, device=dev)
        # :87-90 tf.contrib.rnn.GRUCell(h_dim) (tanh), gate bias 1, candidate bias 0
        self.weights['node_gru'] = GRUCellWeights(tf_glorot_uniform([2 * h_dim, 2 * h_dim], self.tf_generator).to(dev),
                                                  torch.ones(2 * h_dim, dtype=torch.float32, device=dev),
                                                  tf_glorot_uniform([2 * h_dim, h_dim], self.tf_generator).to(dev),
                                                  torch.zeros(h_dim, dtype=torch.float32, device=dev))

    def graph_model_variables(self) -> Dict[str, torch.Tensor]:
        out = {"graph_model/Variable:0": self.weights['edge_weights']}
        if self.params['use_edge_bias']:
            out["graph_model/Variable_1:0"] = self.weights['edge_biases']
        cell = self.weights['node_gru']
        base = "graph_model/gru_scope/gru_cell"
        out[base + "/gates/kernel:0"] = cell.gates_kernel; out[base + "/gates/bias:0"] = cell.gates_bias
        out[base + "/candidate/kernel:0"] = cell.candidate_kernel; out[base + "/candidate/bias:0"] = cell.candidate_bias
        return out

    def set_graph_weights(self, edge_weights, edge_biases, gru: dict) -> None:
        with torch.no_grad():
            as_t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(self.device)
            self.weights['edge_weights'].copy_(as_t(edge_weights))
            if self.params['use_edge_bias']:
                self.weights['edge_biases'].copy_(as_t(edge_biases).reshape(self.weights['edge_biases'].shape))
            c = self.weights['node_gru']
            c.gates_kernel.copy_(as_t(gru['Wg'])); c.gates_bias.copy_(as_t(gru['bg']))
            c.candidate_kernel.copy_(as_t(gru['Wc'])); c.candidate_bias.copy_(as_t(gru['bc']))

    def propagate_format(self, v: int, tracked_weights: bool = False) -> int:
        """Operand format of the graph-resident dense forward for the fed batch (formats.py: the two-piece f16 format only where its
        range is PROVEN, the exact bf16x3 split otherwise).  The dense cell is the tanh GRU (chem_tensorflow_dense.py:88), so every
        state stays <= S = max(1, max|h0|); a vertex sums over at most v * E (source, type) pairs: |acts| <= v E (D max|W_e| S +
        max|b_e|) (:103-112); the weights must lie within the x 2^8 packing's range.  Kept in self.last_format / last_format_bounds.
        tracked_weights (the native training step): the weights' maxima come from formats.TrainingWeightBounds -- measured every
        REMEASURE_STEPS optimizer steps and bounded by Adam's step bound in between -- instead of one measurement per weight version,
        so a steady-state step reads nothing back; the bounds and the decision are computed from them in the same way."""
        from . import formats
        pol = formats.policy()
        if not formats.split_path() or pol == "exact":
            fmt = formats.BF16X3
        elif pol == "force2":
            fmt = formats.F16X2
        else:
            cell = self.weights['node_gru']
            ts = [self.weights['edge_weights'], cell.gates_kernel, cell.candidate_kernel]
            if self.params['use_edge_bias']:
                ts.append(self.weights['edge_biases'])
            if tracked_weights:
                if getattr(self, "_train_weight_bounds", None) is None:
                    self._train_weight_bounds = formats.TrainingWeightBounds()
                mx = self._train_weight_bounds.get(ts, self.optimizer)
            else:
                mx = formats.weight_absmax(ts)
            S = formats.state_bound(formats.h0_absmax(self.placeholders), 'tanh')
            # (|A| <= 1 for the reference's 0 / 1 adjacency; a weighted or multi-edge feed scales the sum: measured, cached per tensor,
            # unless the device packer declared it for this very tensor)
            a_max = formats.adjacency_absmax(self.placeholders['adjacency_matrix'], self.placeholders)
            acts = max(1.0, a_max) * v * self.num_edge_types * (self.params['hidden_size'] * mx[0] * S + (mx[3] if len(mx) > 3 else 0.0))
            if a_max != a_max:
                acts = float("nan")
            fmt = formats.layer_format(S, acts, formats.nanmax(mx[0], mx[1], mx[2]))
            self.last_format_bounds = {"proven": fmt == formats.F16X2, "state_bound": S, "acts_bound": acts, "adjacency_absmax": a_max,
                                       "weight_absmax": formats.nanmax(mx[0], mx[1], mx[2])}
        self.last_format = fmt
        return fmt

    def compute_final_node_representations(self) -> torch.Tensor:
        """chem_tensorflow_dense.py:93-117."""
        if self.training and torch.is_grad_enabled():
            return self._compute_for_training()
        ph = self.placeholders
        v = ph['num_vertices']
        h_dim = self.params['hidden_size']
        h = ph['initial_node_representation']                          # [b, v, h]
        b = h.shape[0]
        h = h.reshape(-1, h_dim).contiguous()                          # :97
        A = ph['adjacency_matrix']                                     # [b, e, v, v]; the :80 transpose is an indexing choice
        keep_w = float(ph.get('edge_weight_dropout_keep_prob', 1.0))
        keep_s = float(ph.get('graph_state_keep_prob', 1.0))
        bias = self.weights['edge_biases'].reshape(self.num_edge_types, h_dim) if self.params['use_edge_bias'] else None
        cell = self.weights['node_gru']
        # the GRU's LDS weight images are packed once per weight version (the one cell is shared by all timesteps, :101-102)
        if USE_GRAPH_RESIDENT_KERNEL and keep_w >= 1.0 and keep_s >= 1.0 and h.is_cuda \
                and ops.dense_propagate_supported(int(v), self.num_edge_types, h_dim):
            # all timesteps in ONE launch: a graph's states stay on its CU (ggnn_dense_propagate_f32)
            W = self.weights['edge_weights'].contiguous()
            return ops.dense_propagate(h.reshape(b, int(v), h_dim), A.contiguous(), ops.PACKED.dense_edge(W),
                                       ops.PACKED.dense_gru(cell.gates_kernel, cell.candidate_kernel, h_dim), bias,
                                       cell.gates_bias, cell.candidate_bias, self.params['num_timesteps'],
                                       fmt=self.propagate_format(int(v)))
        packed = ops.PACKED.gru(cell.gates_kernel, cell.candidate_kernel, 1, h_dim) if ops.gru_is_fused(h_dim) else None
        for i in range(self.params['num_timesteps']):                  # :100
            # :104 a fresh weight-dropout mask per (timestep, edge type)
            W = tf_dropout(self.weights['edge_weights'], keep_w, self.dropout_seed('edge_weights', i)).contiguous()
            Hm = ops.msg_transform(h, W)                               # :104-106 for all edge types
            acts = ops.dense_aggregate(A, Hm, bias)                    # :107-112
            if packed is not None:
                h = ops.gru_packed([acts], h, packed, cell.gates_bias, cell.candidate_bias, "tanh")      # :115
            else:
                h = ops.gru([acts], h, cell.gates_kernel, cell.gates_bias, cell.candidate_kernel, cell.candidate_bias,
                            "tanh")                                    # :115
            h = tf_dropout(h, keep_s, self.dropout_seed('state', i))
        return h.reshape(b, v, h_dim)                                  # :116

    def _compute_for_training(self) -> torch.Tensor:
        """Training form of chem_tensorflow_dense.py:93-117.  A dense step IS a sparse step on the b*v padded nodes:
        acts[d] = sum_e sum_s A_e[d,s] (h_s W_e + b_e) = segment_sum of the transformed source rows + nin @ b_e, with
        sum aggregation and the single shared GRU (the identity tests/test_oracle.py pins).  So the 0/1 adjacency
        tensor is turned into per-type (src, dst) lists once per batch and every timestep runs through the same
        differentiable step as the sparse model (backward.PropagationStepFn: hand-written backward kernels).  Padded
        vertices are isolated nodes there -- their state still evolves through the GRU biases, as in the reference,
        and is masked only at the readout (:126).
        params['graph_resident_training'] (default False): where the graph-resident kernels exist for the batch (_graph_resident_step)
        all timesteps run as ONE differentiable op instead -- one saving forward launch, one backward launch, the weight gradients
        once per variable (backward.DensePropagateFn); every other batch takes the route above.  The value 'native' of the key asks
        for the dense route of train_native.ROUTES, which train.train_step dispatches to before this function is reached; being truthy, it
        sends a batch the native step cannot take through the graph-resident route here, and from there to the route above."""
        from .autograd import propagation_step
        ph = self.placeholders
        v = int(ph['num_vertices'])
        h_dim, T = self.params['hidden_size'], self.num_edge_types
        h0 = ph['initial_node_representation']
        b = h0.shape[0]
        A = ph['adjacency_matrix']                                      # [b, e, dst, src]
        if self._graph_resident_step(v, h0, A):
            return self._compute_graph_resident(v, h0, A)
        sparse_form = ph.get('_sparse_form')
        if sparse_form is None or sparse_form[0] is not A:
            nz = A.nonzero()                                            # rows (b, e, dst, src), lexicographic
            base = nz[:, 0] * v
            pairs = torch.stack([base + nz[:, 3], base + nz[:, 2]], dim=1).to(torch.int32)
            etype = nz[:, 1]
            adjacency_lists = [pairs[etype == t].contiguous() for t in range(T)]
            nin = A.sum(dim=3).permute(0, 2, 1).reshape(b * v, T).to(torch.float32).contiguous()
            sparse_form = ph['_sparse_form'] = (A, ops.build_message_index(adjacency_lists, b * v), nin)
        _, index, nin = sparse_form
        keep_w = float(ph.get('edge_weight_dropout_keep_prob', 1.0))
        keep_s = float(ph.get('graph_state_keep_prob', 1.0))
        bias = self.weights['edge_biases'].reshape(T, h_dim) if self.params['use_edge_bias'] else None
        cell = self.weights['node_gru']
        h = h0.reshape(-1, h_dim).contiguous()
        for i in range(self.params['num_timesteps']):
            # :104 a fresh mask per (timestep, edge type): the [e, h, h] tensor's rows are keyed (e, row), one seed per timestep
            ew_mask = (keep_w, self.dropout_seed('edge_weights', i)) if keep_w < 1.0 else None
            h = propagation_step(h, index, nin, self.weights['edge_weights'], bias, False, [], cell, "tanh", need_grad=True,
                                 ew_mask=ew_mask)
            h = tf_dropout(h, keep_s, self.dropout_seed('state', i))
        return h.reshape(b, v, h_dim)

    def _graph_resident_step(self, v: int, h0: torch.Tensor, A: torch.Tensor, feed: Dict[str, Any] = None) -> bool:
        """Whether this training batch takes the graph-resident route: asked for, on the GPU, kernels for the shape on the split matrix
        path, no weight or state dropout (the dense defaults), and no per-launch timing (which wants the per-timestep launches).
        feed: a batch that is about to be fed (train_native.dense_eligible asks before model.feed): its keep-probs count, the
        placeholders' where it brings none -- what the placeholders hold once it is fed."""
        ph = self.placeholders
        keep = lambda k: float(feed[k] if feed is not None and k in feed else ph.get(k, 1.0))
        return bool(self.params.get('graph_resident_training', False)) and h0.is_cuda and A.is_cuda and ops._timing is None \
            and keep('edge_weight_dropout_keep_prob') >= 1.0 and keep('graph_state_keep_prob') >= 1.0 \
            and formats.split_path() and ops.dense_train_supported(v, self.num_edge_types, self.params['hidden_size'])

    def _in_degrees(self, A: torch.Tensor, b: int, v: int) -> torch.Tensor:
        """In-degrees per (vertex, type) [b*v, E] of the fed adjacency tensor: the operand of the edge biases' gradient.  The device
        packer's ('_sparse_form'), else counted once per fed tensor ('_dense_nin')."""
        ph = self.placeholders
        sparse_form, cached = ph.get('_sparse_form'), ph.get('_dense_nin')
        if sparse_form is not None and sparse_form[0] is A:
            return sparse_form[2]
        if cached is not None and cached[0] is A:
            return cached[1]
        nin = A.sum(dim=3).permute(0, 2, 1).reshape(b * v, self.num_edge_types).to(torch.float32).contiguous()
        ph['_dense_nin'] = (A, nin)
        return nin

    def _compute_graph_resident(self, v: int, h0: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
        from .backward import DensePropagateFn
        h_dim, T = self.params['hidden_size'], self.num_edge_types
        b = h0.shape[0]
        nin = self._in_degrees(A, b, v) if self.params['use_edge_bias'] else None
        bias = self.weights['edge_biases'].reshape(T, h_dim) if self.params['use_edge_bias'] else None
        cell = self.weights['node_gru']
        return DensePropagateFn.apply(h0.reshape(b, v, h_dim).contiguous(), A.contiguous(), nin, self.weights['edge_weights'], bias,
                                      cell.gates_kernel, cell.gates_bias, cell.candidate_kernel, cell.candidate_bias,
                                      self.params['num_timesteps'], self.propagate_format(v))

    def _readout_rows(self, b: int, v: int, device):
        """(graph of every row, first row of every graph) of the flattened [b*v, h] states, cached per (b, v, device)."""
        key = (b, v, str(device))
        cached = getattr(self, '_readout_index', None)
        if cached is None or cached[0] != key:
            gnl = torch.arange(b, dtype=torch.int32, device=device).repeat_interleave(v).contiguous()
            gptr = (torch.arange(b + 1, dtype=torch.int32, device=device) * v).contiguous()
            self._readout_index = cached = (key, gnl, gptr)
        return cached[1], cached[2]

    def gated_regression_with_loss(self, last_h, regression_gate, regression_transform, target_values, target_mask):
        """chem_tensorflow_dense.py:119-129 + chem_tensorflow.py:161-166 on the fused readout kernels: graph g owns the
        consecutive rows g*v .. g*v+v-1 of the flattened [b*v, h] states, padding vertices are switched off by node_mask."""
        from .autograd import readout_loss
        ph = self.placeholders
        h_dim = self.params['hidden_size']
        g, t = regression_gate.params, regression_transform.params
        if not last_h.is_cuda or h_dim > 256 or len(g["weights"]) != 1 or len(t["weights"]) != 1:
            return None
        b, v = last_h.shape[0], int(ph['num_vertices'])
        gnl, gptr = self._readout_rows(b, v, last_h.device)
        out, num, ab, ms = readout_loss(last_h.reshape(-1, h_dim), ph['initial_node_representation'].reshape(-1, h_dim).contiguous(),
                                        gnl, gptr, ph['node_mask'].reshape(-1).contiguous(), b,
                                        regression_gate.dropped_weight(0), g["biases"][0], regression_transform.dropped_weight(0),
                                        t["biases"][0], target_values.contiguous(), target_mask.contiguous())
        self.output = out
        return out, num, ab, ms

    def gated_regression_with_loss_multi(self, last_h):
        """gated_regression_with_loss for every entry of task_ids in one pass over the [b*v, h] states (autograd.readout_loss_multi;
        params['multitask_readout']): -> (out [K,b], num [K], ab [K], ms [K]), or None when the multi-task kernels do not apply."""
        from .autograd import readout_loss_multi
        ph = self.placeholders
        task_ids = self.params['task_ids']
        K, h_dim = len(task_ids), self.params['hidden_size']
        gates = [self.weights['regression_gate_task%i' % t] for t in task_ids]
        transforms = [self.weights['regression_transform_task%i' % t] for t in task_ids]
        if not last_h.is_cuda or K < 2 or not ops.readout_multi_supported(h_dim, K) \
                or any(len(m.params["weights"]) != 1 for m in gates + transforms):
            return None
        b, v = last_h.shape[0], int(ph['num_vertices'])
        gnl, gptr = self._readout_rows(b, v, last_h.device)
        return readout_loss_multi(last_h.reshape(-1, h_dim), ph['initial_node_representation'].reshape(-1, h_dim).contiguous(),
                                  gnl, gptr, ph['node_mask'].reshape(-1).contiguous(), b,
                                  [m.dropped_weight(0) for m in gates], [m.params["biases"][0] for m in gates],
                                  [m.dropped_weight(0) for m in transforms], [m.params["biases"][0] for m in transforms],
                                  ph['target_values'], ph['target_mask'])

    def gated_regression(self, last_h, regression_gate, regression_transform):
        """chem_tensorflow_dense.py:119-129."""
        ph = self.placeholders
        h_dim = self.params['hidden_size']
        gate_input = torch.cat([last_h, ph['initial_node_representation']], dim=2).reshape(-1, 2 * h_dim)
        last = last_h.reshape(-1, h_dim)
        gated_outputs = torch.sigmoid(regression_gate(gate_input)) * regression_transform(last)     # [b*v, 1]
        gated_outputs = gated_outputs.reshape(-1, ph['num_vertices'])                                # [b, v]
        masked_gated_outputs = gated_outputs * ph['node_mask']
        output = masked_gated_outputs.sum(dim=1)                                                     # [b]
        self.output = output
        return output

    # ----- Data preprocessing and chunking into minibatches:
    def process_raw_graphs(self, raw_data, is_training_data: bool, bucket_sizes=None) -> Any:
        """chem_tensorflow_dense.py:132-164: bucket graphs by padded size; a bucket holds graph ids."""
        ms = raw_data if isinstance(raw_data, MoleculeSet) else MoleculeSet.from_json(raw_data)
        if bucket_sizes is None:
            bucket_sizes = DENSE_BUCKET_SIZES
        n = ms.nodes_per_graph()
        # :138 argmax(bucket_sizes > max vertex index mentioned by an edge); graphs without bonds (the
        # reference would fail on max([])) fall back to their node count
        max_idx = n - 1
        nb = np.diff(ms.bond_ptr)
        has = nb > 0
        if has.any():
            ends = np.maximum(ms.bonds[:, 0], ms.bonds[:, 2]).astype(np.int64)
            max_idx = max_idx.copy()
            max_idx[has] = np.maximum.reduceat(ends, ms.bond_ptr[:-1][has])
        if (max_idx >= n).any():
            raise IndexError("a bond mentions a vertex outside its graph")
        chosen = np.searchsorted(bucket_sizes, np.maximum(max_idx, n - 1), side='right')
        if (chosen >= len(bucket_sizes)).any():
            raise ValueError("graph larger than the largest bucket size")
        bucketed = defaultdict(list)
        for g, bi in enumerate(chosen):
            bucketed[int(bi)].append(g)
        # :153-158 per bucket: shuffle, then labels of the examples beyond task_sample_ratios are masked.  The mask
        # belongs to the graph (it follows it through the later per-epoch shuffles).  The reference's `labels[task_id] = None`
        # indexes the per-task label list (len(task_ids) entries) by TASK ID: the right label only for task_ids == [0..k), an
        # IndexError or a neighbour's label otherwise.  Like the sparse model here, the label of THAT task is masked.
        label_mask = np.ones((ms.num_graphs, len(self.params['task_ids'])), dtype=np.float32)
        if is_training_data:
            for bucket_list in bucketed.values():
                np.random.shuffle(bucket_list)
                for internal_id, task_id in enumerate(self.params['task_ids']):
                    task_sample_ratio = self.params['task_sample_ratios'].get(str(task_id))
                    if task_sample_ratio is not None:
                        ex_to_sample = int(len(bucket_list) * task_sample_ratio)
                        if bucket_list[ex_to_sample:]:
                            label_mask[np.asarray(bucket_list[ex_to_sample:]), internal_id] = 0.0
        # :160-162 one entry per full batch of a bucket (remainder graphs are dropped)
        bucket_at_step = [b for b, graphs in bucketed.items() for _ in range(len(graphs) // self.params['batch_size'])]
        return {"molecules": ms, "bucketed": dict(bucketed), "bucket_sizes": np.asarray(bucket_sizes),
                "bucket_at_step": bucket_at_step, "device_batches": {}, "label_mask": label_mask}

    def _epoch_order(self, bucketed, bucket_at_step):
        """The graphs of make_minibatch_iterator's steps, concatenated (int64), and each step's first position in it."""
        bs = self.params['batch_size']
        counters = defaultdict(int)
        parts = []
        for bucket in bucket_at_step:
            c = counters[bucket]
            parts.append(np.asarray(bucketed[bucket][c * bs:(c + 1) * bs], dtype=np.int64))
            counters[bucket] += 1
        starts = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        return (np.concatenate(parts) if parts else np.zeros(0, np.int64)), [int(x) for x in starts]

    def to_device_batch(self, db) -> Dict[str, Any]:
        dev = self.device
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return {'initial_node_representation': t(db.initial_node_representation), 'adjacency_matrix': t(db.adjacency_matrix),
                'node_mask': t(db.node_mask), 'num_vertices': db.num_vertices, 'target_values': t(db.target_values),
                'target_mask': t(db.target_mask), 'num_graphs': db.num_graphs}

    def prepare_resident_data(self, data: Any, is_training: bool) -> None:
        """pack_on_device: upload the dataset and build the dataset-level tables on the CURRENT stream (run_epoch calls this before it
        hands the epoch to the producer thread, whose stream is ordered behind it)."""
        if not self.params.get('pack_on_device') or data is None:
            return
        if data.get("molecules_dev") is None:
            from .data_device import DeviceMoleculeSet
            data["molecules_dev"] = DeviceMoleculeSet(data["molecules"], self.device, data["label_mask"])
        dms = data["molecules_dev"]
        dms.dense_tables(self.num_edge_types, self.params['tie_fwd_bkwd'])
        K = dms.targets.shape[1] if dms.targets.dim() == 2 else 0
        if any(not 0 <= int(t) < K for t in self.params['task_ids']):
            raise IndexError("task_ids %s outside the dataset's %d targets" % (self.params['task_ids'], K))
        dms.task_ids_dev(self.params['task_ids'])

    # run_epoch's producer thread with pack_on_device (threaded_batches 'auto'): the dense training step is the autograd path, whose
    # Python the launching thread is busy with; packing on the producer thread's stream measured 2.30 against 2.91 ms per step inline
    # (tools/dense_bench.py, profiles/dense_epoch.json)
    DEVICE_PACK_THREADED = True

    def threaded_batches_default(self) -> bool:
        if self.params.get('pack_on_device'):
            return self.DEVICE_PACK_THREADED
        return super().threaded_batches_default()

    def _device_compact(self) -> bool:
        """Whether the training step transforms on the compacted (source, type) rows (backward.PropagationStepFn's own test)."""
        from . import backward
        D = self.params['hidden_size']
        return backward.compact_training(D)

    def _device_epoch(self, data: Any, order: np.ndarray) -> torch.Tensor:
        """The epoch's order on the device (one upload) and its per-(graph, type) prefix sums (one launch)."""
        self.prepare_resident_data(data, False)
        dms = data["molecules_dev"]
        tab = dms.dense_tables(self.num_edge_types, self.params['tie_fwd_bkwd'])
        order_dev = dms.upload_order(np.asarray(order, dtype=np.int64))
        if order_dev.is_cuda:
            order_dev.record_stream(torch.cuda.current_stream(order_dev.device))    # (allocated on the upload stream, read on this one)
        return ops.dense_epoch_table(tab["counts_t"], order_dev)

    def device_batch(self, data: Any, epoch_tab: torch.Tensor, start: int, ids: np.ndarray, v: int, is_training: bool) -> Dict[str, Any]:
        """The batch of graphs `ids` = epoch positions [start, start + len(ids)), assembled on the GPU in one launch
        (ops.dense_assemble_batch).  The host computes only the per-type sizes, from its own count tables; nothing is read back.
        Feeds are to_device_batch(pack_dense_batch(...))'s; a training feed also carries '_sparse_form' = (A, index, nin), the form
        _compute_for_training would derive from A, and both feeds declare max|h0| and max|A| (formats.py)."""
        dms = data["molecules_dev"]
        T = self.num_edge_types
        tab = dms.dense_tables(T, self.params['tie_fwd_bkwd'])
        ids = np.asarray(ids, dtype=np.int64)
        mc = tab["mc"][ids].sum(axis=0)
        compact = bool(is_training) and self._device_compact()
        type_off = [0] + [int(x) for x in np.cumsum(mc)]
        type_row_off = [0] + [int(x) for x in np.cumsum(tab["pc"][ids].sum(axis=0))] if compact else None
        out = ops.dense_assemble_batch(tab, dms.node_feat, dms.targets, dms.label_mask, dms.task_ids_dev(self.params['task_ids']),
                                       epoch_tab, start, len(ids), v, self.params['hidden_size'], type_off, type_row_off,
                                       sparse=bool(is_training), compact=compact, arange=dms.arange_i32)
        A = out['adjacency_matrix']
        feed = {'initial_node_representation': out['initial_node_representation'], 'adjacency_matrix': A,
                'node_mask': out['node_mask'], 'num_vertices': int(v), 'target_values': out['target_values'],
                'target_mask': out['target_mask'], 'num_graphs': len(ids)}
        if is_training:
            feed['_sparse_form'] = (A, out['index'], out['nin'])
        formats.declare_h0_absmax(feed, dms.node_feat_absmax)
        # (every entry the packer wrote is 0 or 1: max|A| is 1 as soon as the batch has a message -- what a measurement would find)
        return formats.declare_adjacency_absmax(feed, 1.0 if type_off[-1] else 0.0)

    def make_minibatch_iterator(self, data, is_training: bool):
        """chem_tensorflow_dense.py:195-228.  With pack_on_device the batches are assembled on the GPU (device_batch) from the same
        shuffles, in the same order: the same feeds bit for bit."""
        ms: MoleculeSet = data["molecules"]
        bucketed, bucket_sizes, bucket_at_step = data["bucketed"], data["bucket_sizes"], data["bucket_at_step"]
        if is_training:                                   # :197-200 the step list, then every bucket; in place (orders compose over epochs)
            for shuffled in (bucket_at_step, *bucketed.values()):
                np.random.shuffle(shuffled)
        batches_taken = defaultdict(int)                  # per bucket, so far in this epoch
        keep_prob = self.params['graph_state_dropout_keep_prob'] if is_training else 1.0
        bs = self.params['batch_size']
        on_device = bool(self.params.get('pack_on_device'))
        epoch_tab, starts = None, None                    # pack_on_device: the epoch's order on the device, formed at the first batch
        for step, bucket in enumerate(bucket_at_step):
            start_idx = batches_taken[bucket] * bs
            ids = np.asarray(bucketed[bucket][start_idx:start_idx + bs])
            key = (bucket, batches_taken[bucket])
            if is_training or key not in data["device_batches"]:
                if on_device:
                    if epoch_tab is None:
                        order, starts = self._epoch_order(bucketed, bucket_at_step)
                        epoch_tab = self._device_epoch(data, order)
                    feed = self.device_batch(data, epoch_tab, starts[step], ids, int(bucket_sizes[bucket]), is_training)
                else:
                    db = pack_dense_batch(ms, ids, int(bucket_sizes[bucket]), self.num_edge_types,
                                          self.params['hidden_size'], self.params['tie_fwd_bkwd'], self.params['task_ids'],
                                          label_mask=data.get("label_mask"))
                    feed = self.to_device_batch(db)
                if not is_training:
                    data["device_batches"][key] = feed
            else:
                feed = data["device_batches"][key]
            feed = dict(feed)
            # :222-223 the dense model feeds graph_state_dropout_keep_prob into BOTH keep-prob placeholders
            feed['graph_state_keep_prob'] = keep_prob
            feed['edge_weight_dropout_keep_prob'] = keep_prob
            batches_taken[bucket] += 1
            yield feed
