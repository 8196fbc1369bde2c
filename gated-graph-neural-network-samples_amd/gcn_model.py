"""SparseGCNChemModel -- host-side mirror of chem_tensorflow_gcn.py (Kipf-style GCN) on PyTorch-ROCm tensors, with every layer

    out = dropout(relu(A_hat h W_l + b_l))          (ReLU and dropout on all but the last layer; chem_tensorflow_gcn.py:68-80)

running as one fused aggregate-transform HIP launch (csrc/ggnn_gcn.hip) at hidden sizes 32 / 64 / 100, and as the composition
weighted segment sum -> GEMM -> epilogue at the others -- or, with params['gcn_panel_layers'] = True, as one launch of the
column-panel kernel (csrc/ggnn_gcn_panel.hip) at hidden sizes 128 / 192 / 256.  Inference runs all layers behind one native call
(ggnn_gcn_propagate_f32); training runs GCNLayerFn per layer (hand-written backward, no autograd on the kernels), or with
params['native_training'] = True the whole step as two native calls (train_native.ROUTES, entry `gcn`, csrc/ggnn_gcn_train.hip:
hidden sizes 32 / 64 / 100, and 128 / 192 / 256 when params['gcn_panel_layers'] is set as well).
The readout and loss are the fused kernels of the sparse GGNN (chem_tensorflow_gcn.py:84-93 is the same formula).
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Sequence

import numpy as np
import torch

from . import ops
from .backward import _SINK, _on_side_stream, _tn
from .chem_model import ChemModel
from .data import MoleculeSet, _ranges, batch_boundaries
from .sparse_model import SparseGGNNChemModel
from .utils import glorot_init


def gcn_adjacency(ms: MoleculeSet):
    """The reference's __graph_to_adjacency_list (chem_tensorflow_gcn.py:117-142) for every graph of `ms` at once:
    undirected 0/1 adjacency (bond types ignored, duplicate bonds collapse), + I (a self-bond gives a diagonal of 2),
    D^-1/2 A D^-1/2 in f64 with 1e-7 added after the power, entries row-major sorted.
    -> (entry_ptr int64 [G+1], adjacency_list int64 [nnz, 2] (graph-local), adjacency_weights float64 [nnz]).
    Cast the weights to float32 at feed time (the placeholder is float32)."""
    G = ms.num_graphs
    N = int(ms.node_ptr[-1])
    nb = np.diff(ms.bond_ptr)
    off = np.repeat(ms.node_ptr[:-1], nb).astype(np.int64)
    s = ms.bonds[:, 0].astype(np.int64) + off
    d = ms.bonds[:, 2].astype(np.int64) + off
    bond_keys = np.unique(np.concatenate([s * N + d, d * N + s]))               # adj[src, dest] = adj[dest, src] = 1
    diag = np.arange(N, dtype=np.int64) * (N + 1)                              # + np.eye
    keys, inv = np.unique(np.concatenate([bond_keys, diag]), return_inverse=True)
    A = np.bincount(inv.reshape(-1), minlength=len(keys)).astype(np.float64)
    i, j = keys // N, keys % N
    row_sum = np.bincount(i, weights=A, minlength=N)
    d_inv_sqrt = np.power(row_sum, -0.5) + 1e-7
    w = (d_inv_sqrt[i] * A) * d_inv_sqrt[j]                                    # (D A) D, one nonzero term per product
    g = np.repeat(np.arange(G, dtype=np.int64), np.diff(ms.node_ptr))[i] if N else np.zeros(0, np.int64)
    entry_ptr = np.zeros(G + 1, np.int64)
    np.cumsum(np.bincount(g, minlength=G), out=entry_ptr[1:])
    base = ms.node_ptr[g]
    adj = np.stack([i - base, j - base], axis=1)
    return entry_ptr, adj, w


class GCNLayerFn(torch.autograd.Function):
    """One GCN layer with its hand-written backward.  With P = S W + b, S = A_hat x, out = drop(relu(P)):
        dP = act_bwd(dropout(dOut), out)   (identity on the linear layer)
        dW = S^T dP (ggnn_gemm_tn_f32), db = colsum(dP), dx = A_hat^T (dP W^T) (the same layer launch on the transposed CSR).
    Inside backward.weight_gradient_sink the dW / db products go to the optimiser's flat gradient buffer on the side stream.
    panel: the layer launch and the dx launch take ops.gcn_layer's panel route (hidden sizes 128 / 192 / 256)."""

    @staticmethod
    def forward(ctx, x, W, b, graph, relu, keep_prob, seed, row_key, panel=False):
        out, S = ops.gcn_layer(x.contiguous(), graph, W, b, relu, keep_prob, seed, row_key, save_s=True, panel=bool(panel))
        ctx.panel = bool(panel)
        ctx.save_for_backward(S, out, W)
        ctx.graph, ctx.relu, ctx.keep, ctx.seed, ctx.row_key = graph, bool(relu), float(keep_prob), int(seed), row_key
        ctx.w_ptr = W.data_ptr()
        ctx.b_ptr = None if b is None else b.data_ptr()
        return out

    @staticmethod
    def backward(ctx, g):
        S, out, W = ctx.saved_tensors
        g = g.contiguous()
        if ctx.keep < 1.0:
            g = ops.dropout(g, ctx.keep, ctx.seed, ctx.row_key)
        dP = ops.act_bwd(g, out, "relu") if ctx.relu else g
        dW = db = None
        has_b = ctx.b_ptr is not None
        tW = _SINK.target(ctx.w_ptr, W.shape) if ctx.needs_input_grad[1] else None
        tb = _SINK.target(ctx.b_ptr, (W.shape[1],)) if has_b and ctx.needs_input_grad[2] else None
        if tW is not None and (tb is not None or not (has_b and ctx.needs_input_grad[2])):
            def weight_products():
                _SINK.add(ctx.w_ptr, tW, _tn(S, dP))
                if tb is not None:
                    _SINK.add(ctx.b_ptr, tb, ops.colsum(dP))
            _on_side_stream([S, dP], weight_products)
        else:
            if ctx.needs_input_grad[1]:
                dW = _tn(S, dP)
            if has_b and ctx.needs_input_grad[2]:
                db = ops.colsum(dP)
        dx = ops.gcn_layer(dP, ctx.graph, W, transpose=True, panel=ctx.panel)[0] if ctx.needs_input_grad[0] else None
        return dx, dW, db, None, None, None, None, None, None


class SparseGCNChemModel(ChemModel):
    def __init__(self, args):
        super().__init__(args)

    @classmethod
    def default_params(cls):
        # chem_tensorflow_gcn.py:33-40
        params = dict(super().default_params())
        params.update({'batch_size': 100000,
                       'task_sample_ratios': {},
                       'gcn_use_bias': False,
                       'graph_state_dropout_keep_prob': 1.0,
                       })
        # (params['pack_on_device'], default False, is read with .get like the sparse model's: a key in this dict would break
        # restoring the reference's checkpoints, whose params must match key for key, chem_tensorflow.py:336-340.  So is
        # params['native_training'], default False: the optimisation step on the gcn route of train_native.ROUTES, and
        # params['gcn_panel_layers'], default False: hidden sizes 128 / 192 / 256 on the column-panel kernel, gcn_panel_route)
        return params

    DERIVED_PLACEHOLDERS = dict(ChemModel.DERIVED_PLACEHOLDERS, adjacency_list=('gcn_graph',), adjacency_weights=('gcn_graph',))

    # ---- weights ------------------------------------------------------------------------------------
    def prepare_specific_graph_model(self) -> None:
        """chem_tensorflow_gcn.py:42-59: glorot weights [D, D] per layer from the NumPy stream in creation order, zero biases.
        params['pack_on_device'] (default False): batches are assembled on the GPU from the resident dataset
        (DeviceMoleculeSet.gcn_tables, ggnn_gcn_assemble_batch) instead of packed in NumPy and uploaded -- the same feeds bit for bit,
        without 'adjacency_list' / 'adjacency_weights'.  Needs a CUDA/HIP device."""
        h_dim = self.params['hidden_size']
        if h_dim <= 0 or h_dim % 4:
            raise ValueError("hidden_size %r: the GCN kernels take positive multiples of 4" % (h_dim,))
        if self.annotation_size > h_dim:
            raise ValueError("annotation_size %d exceeds hidden_size %d" % (self.annotation_size, h_dim))
        if self.params.get('pack_on_device') and torch.device(self.device).type != 'cuda':
            raise ValueError("pack_on_device=True assembles batches on the GPU; device %r is not a CUDA/HIP device" % (str(self.device),))
        self._kw = h_dim                               # (the borrowed readout methods read the kernel width)
        for name in ('initial_node_representation', 'adjacency_list', 'adjacency_weights', 'graph_nodes_list', 'gcn_graph'):
            self.placeholders[name] = None
        self.placeholders['graph_state_keep_prob'] = 1.0
        dev = self.device
        L = self.params['num_timesteps']
        self.weights['edge_weights'] = [torch.from_numpy(glorot_init((h_dim, h_dim))).to(dev) for _ in range(L)]
        self.weights['edge_biases'] = [torch.zeros(h_dim, dtype=torch.float32, device=dev) for _ in range(L)] \
            if self.params['gcn_use_bias'] else []

    def graph_model_variables(self) -> Dict[str, torch.Tensor]:
        out = {}
        for i, W in enumerate(self.weights['edge_weights']):
            out["graph_model/gcn_scope/gcn_weights_%i:0" % i] = W
        for i, b in enumerate(self.weights['edge_biases']):
            out["graph_model/gcn_scope/gcn_bias_%i:0" % i] = b
        return out

    def set_graph_weights(self, weights: Sequence[np.ndarray], biases: Optional[Sequence[np.ndarray]] = None) -> None:
        """Inject explicit layer weights [D, D] (and biases [D] with gcn_use_bias)."""
        with torch.no_grad():
            for t, w in zip(self.weights['edge_weights'], weights):
                t.copy_(torch.as_tensor(np.asarray(w, dtype=np.float32)).to(t.device))
            for t, b in zip(self.weights['edge_biases'], biases or []):
                t.copy_(torch.as_tensor(np.asarray(b, dtype=np.float32)).to(t.device))

    # ---- forward --------------------------------------------------------------------------------------
    def _graph(self) -> "ops.GCNGraph":
        ph = self.placeholders
        graph = ph.get('gcn_graph')
        if graph is None:
            V = ph['initial_node_representation'].shape[0]
            graph = ph['gcn_graph'] = ops.gcn_graph(ph['adjacency_list'], ph['adjacency_weights'], V, self.device)
        return graph

    def gcn_panel_route(self) -> bool:
        """params['gcn_panel_layers'] (default False) asks for the column-panel layer kernel (csrc/ggnn_gcn_panel.hip); it is
        available on a CUDA/HIP device at hidden sizes 128 / 192 / 256.  Anywhere else the key changes nothing."""
        return bool(self.params.get('gcn_panel_layers')) and torch.device(self.device).type == 'cuda' \
            and ops.gcn_panel_supported(self.params['hidden_size'])

    def compute_final_node_representations(self) -> torch.Tensor:
        """chem_tensorflow_gcn.py:62-82."""
        ph = self.placeholders
        h = ph['initial_node_representation']
        graph = self._graph()
        Ws = self.weights['edge_weights']
        bs = self.weights['edge_biases'] if self.params['gcn_use_bias'] else None
        keep = float(ph.get('graph_state_keep_prob', 1.0))
        need_grad = self.training and torch.is_grad_enabled()
        L = len(Ws)
        D = self.params['hidden_size']
        panel = self.gcn_panel_route()
        if not need_grad and keep >= 1.0 and ops._timing is None:            # every layer in one native call
            if panel:
                return ops.gcn_panel_propagate(h, graph, Ws, bs)
            if ops.gcn_fused_supported(D):
                return ops.gcn_propagate(h, graph, Ws, bs)
        uid = self._node_uid() if keep < 1.0 else None
        for l in range(L):
            last = l == L - 1
            kp = 1.0 if last else keep
            seed = self.dropout_seed('gcn_state', l) if kp < 1.0 else 0
            b = bs[l] if bs is not None else None
            if need_grad:
                h = GCNLayerFn.apply(h, Ws[l], b, graph, not last, kp, seed, uid, panel)
            else:
                h = ops.gcn_layer(h, graph, Ws[l], b, relu=not last, keep_prob=kp, seed=seed, row_key=uid, panel=panel)[0]
        return h

    def _node_uid(self) -> Optional[torch.Tensor]:
        return self.placeholders.get('node_uid')

    # chem_tensorflow_gcn.py:84-93 is the sparse GGNN's readout formula: the same fused readout / loss kernels
    gated_regression_with_loss = SparseGGNNChemModel.gated_regression_with_loss
    gated_regression_with_loss_multi = SparseGGNNChemModel.gated_regression_with_loss_multi
    gated_regression = SparseGGNNChemModel.gated_regression
    _graph_nodes_sorted = SparseGGNNChemModel._graph_nodes_sorted
    _pad_blocks = staticmethod(SparseGGNNChemModel._pad_blocks)

    # ---- data preprocessing and chunking into minibatches ------------------------------------------------
    def process_raw_graphs(self, raw_data, is_training_data: bool) -> Any:
        """chem_tensorflow_gcn.py:96-115, vectorised over the whole set (gcn_adjacency).  Training data are shuffled once
        (np.random.permutation draws the swaps of np.random.shuffle) and labels beyond task_sample_ratios are masked
        (the reference indexes its per-graph label list by task id, :113)."""
        ms = raw_data if isinstance(raw_data, MoleculeSet) else MoleculeSet.from_json(raw_data)
        K = len(self.params['task_ids'])
        label_mask = np.ones((ms.num_graphs, K), dtype=np.float32)
        if is_training_data:
            ms = ms.subset(np.random.permutation(ms.num_graphs))
            for task_id in self.params['task_ids']:
                ratio = self.params['task_sample_ratios'].get(str(task_id))
                if ratio is not None:
                    label_mask[int(ms.num_graphs * ratio):, task_id] = 0.0
        entry_ptr, adj, w = gcn_adjacency(ms)
        return {"molecules": ms, "label_mask": label_mask, "entry_ptr": entry_ptr, "adjacency_list": adj,
                "adjacency_weights": w, "valid_batches": None}

    def pack_batch(self, data: Any, ids: np.ndarray, keep_prob: float) -> Dict[str, Any]:
        """One minibatch of the graphs `ids` (chem_tensorflow_gcn.py:154-196) as a feed dict on the device."""
        ms: MoleculeSet = data["molecules"]
        dev = self.device
        D = self.params['hidden_size']
        npg = np.diff(ms.node_ptr)[ids]
        V = int(npg.sum())
        feat = ms.node_feat[_ranges(ms.node_ptr[ids], npg)]
        h0 = np.zeros((V, D), np.float32)
        h0[:, :feat.shape[1]] = feat
        node_off = np.concatenate([[0], np.cumsum(npg)[:-1]]).astype(np.int64)
        ne = np.diff(data["entry_ptr"])[ids]
        esel = _ranges(data["entry_ptr"][ids], ne)
        adj = data["adjacency_list"][esel] + np.repeat(node_off, ne)[:, None]
        w = data["adjacency_weights"][esel].astype(np.float32)
        gnl = np.repeat(np.arange(len(ids), dtype=np.int32), npg)
        local = np.arange(V, dtype=np.int64) - np.repeat(node_off, npg)
        uid = (np.repeat(np.asarray(ids, np.int64), npg) << 20) + local     # state-dropout row keys: (graph id, node), as the GGNN's
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        task_cols = np.asarray(self.params['task_ids'], dtype=np.int64)
        mask = data["label_mask"][ids]
        return {
            'initial_node_representation': t(h0),
            'adjacency_list': adj,
            'adjacency_weights': w,
            'gcn_graph': ops.gcn_graph(adj, w, V, dev),
            'graph_nodes_list': t(gnl),
            'graph_ptr': t(np.concatenate([[0], np.cumsum(npg)]).astype(np.int32)),
            'graph_nodes_sorted': True,
            'node_uid': t(uid),
            # (an unsampled label is fed as 0 with mask 0, chem_tensorflow_gcn.py:175-177)
            'target_values': t(np.where(mask > 0, ms.targets[ids][:, task_cols], 0.0).T.astype(np.float32)),
            'target_mask': t(mask.T),
            'num_graphs': int(len(ids)),
            'graph_state_keep_prob': keep_prob,
        }

    def prepare_resident_data(self, data: Any, is_training: bool) -> None:
        """pack_on_device: upload the dataset and build the dataset-level A_hat tables on the CURRENT stream (run_epoch calls this
        before it hands the epoch to the producer thread, whose stream is ordered behind it)."""
        if not self.params.get('pack_on_device') or data is None:
            return
        if data.get("molecules_dev") is None:
            from .data_device import DeviceMoleculeSet
            data["molecules_dev"] = DeviceMoleculeSet(data["molecules"], self.device, data["label_mask"])
        dms = data["molecules_dev"]
        dms.gcn_tables(data["entry_ptr"], data["adjacency_list"], data["adjacency_weights"])
        K = dms.targets.shape[1] if dms.targets.dim() == 2 else 0
        if any(not 0 <= int(t) < K for t in self.params['task_ids']):
            raise IndexError("task_ids %s outside the dataset's %d targets" % (self.params['task_ids'], K))
        dms.task_ids_dev(self.params['task_ids'])

    # run_epoch's producer thread with pack_on_device (threaded_batches 'auto'): a batch is one launch and ~0.13 ms of host work, so
    # a second thread mostly takes the interpreter lock from the step's launches: 1.55 against 1.44 ms per step inline
    # (tools/gcn_bench.py --leg epoch, profiles/gcn_epoch.json)
    DEVICE_PACK_THREADED = False

    def threaded_batches_default(self) -> bool:
        if self.params.get('pack_on_device'):
            return self.DEVICE_PACK_THREADED
        from . import train_native
        if train_native.gcn_model_eligible(self):
            return False                          # the native step leaves the host slack: inline packing, as for the native GGNN step
        return super().threaded_batches_default()

    def device_batches(self, data: Any, order: np.ndarray, keep_prob: float):
        """One epoch's batches of graph order `order`, assembled on the GPU (pack_on_device): the order goes up once
        (DeviceMoleculeSet.upload_order), its node / entry prefix sums are formed there once (ops.gcn_epoch_table), and every batch
        is one ggnn_gcn_assemble_batch launch.  The host computes only the batch boundaries and totals, from its own count copies;
        nothing is read back.  Feeds are pack_batch's without 'adjacency_list' / 'adjacency_weights'."""
        self.prepare_resident_data(data, False)
        dms = data["molecules_dev"]
        tab = dms.gcn_tables(data["entry_ptr"], data["adjacency_list"], data["adjacency_weights"])
        order = np.asarray(order, dtype=np.int64)
        npg = dms.nodes_per_graph[order]
        bounds = batch_boundaries(npg, self.params['batch_size'])
        node_cum = np.concatenate([[0], np.cumsum(npg)])
        entry_cum = np.concatenate([[0], np.cumsum(tab["entries_per_graph"][order])])
        order_dev = dms.upload_order(order)
        if order_dev.is_cuda:
            order_dev.record_stream(torch.cuda.current_stream(order_dev.device))    # (allocated on the upload stream, read on this one)
        epoch_tab = ops.gcn_epoch_table(tab["counts_t"], order_dev)
        tids = dms.task_ids_dev(self.params['task_ids'])
        D = self.params['hidden_size']
        for s, e in zip(bounds[:-1], bounds[1:]):
            graph, h0, gnl, graph_ptr, uid, tv, tm = ops.gcn_assemble_batch(
                tab["node_ptr"], dms.node_feat, tab["csr"], tab["csr_t"], dms.targets, dms.label_mask, tids, epoch_tab, s, e - s,
                int(node_cum[e] - node_cum[s]), int(entry_cum[e] - entry_cum[s]), D)
            yield {
                'initial_node_representation': h0,
                'gcn_graph': graph,
                'graph_nodes_list': gnl,
                'graph_ptr': graph_ptr,
                'graph_nodes_sorted': True,
                'node_uid': uid,
                'target_values': tv,
                'target_mask': tm,
                'num_graphs': int(e - s),
                'graph_state_keep_prob': keep_prob,
            }

    def make_minibatch_iterator(self, data: Any, is_training: bool):
        """chem_tensorflow_gcn.py:144-196: graphs packed while node_offset + n < batch_size (strict); training data reshuffled
        every epoch (in place, so the orders compose), validation batches packed once and kept on the device.  With
        pack_on_device the batches are assembled on the GPU (device_batches), the same feeds bit for bit."""
        ms: MoleculeSet = data["molecules"]
        if not is_training and data["valid_batches"] is not None:
            yield from (dict(b) for b in data["valid_batches"])
            return
        if is_training:
            perm = np.random.permutation(ms.num_graphs)
            prev = data.get("epoch_order")
            order = perm if prev is None else prev[perm]
            data["epoch_order"] = order
        else:
            order = np.arange(ms.num_graphs)
        keep = self.params['graph_state_dropout_keep_prob'] if is_training else 1.0
        if self.params.get('pack_on_device'):
            batches = self.device_batches(data, order, keep)
        else:
            bounds = batch_boundaries(np.diff(ms.node_ptr)[order], self.params['batch_size'])
            batches = (self.pack_batch(data, order[s:e], keep) for s, e in zip(bounds[:-1], bounds[1:]))
        if is_training:
            yield from batches
        else:
            data["valid_batches"] = list(batches)
            yield from (dict(b) for b in data["valid_batches"])
