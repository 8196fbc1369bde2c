"""ChemModel -- what the chemistry models (sparse_model, dense_model, gcn_model) share: the configuration, the datasets, the per-task
gated read-out with its masked loss, the optimizer, the training harness and the checkpoints; host code around libggnn_hip.so:
  * construction runs in steps: the run's files, the parameters (resolve_params), the seeds, the data, the model, then a
    restored checkpoint or step zero;
  * `self.placeholders` is a dict name -> tensor that `feed()` fills from a minibatch, `self.ops` holds the last batch's values;
  * run_epoch hands every step to an EpochStats, train() keeps the best validation score in a BestEpoch;
  * a checkpoint is a pickle {params, weights, train_step, valid_step} with the weights under TF-1.x variable names.
The parameter keys and defaults, the checkpoints, the log entries, the file names and the printed text are an interchange format
with the TensorFlow implementation of these models (chem_tensorflow.py) and stay as they are.  `args` is a dict with its
command-line keys ('--config', '--config-file', '--data_dir', '--log_dir', '--restore', '--freeze-graph-model',
'--restrict_data') and keys of our own: 'train_data' / 'valid_data' (an in-memory MoleculeSet or raw JSON list instead of a file),
'--device' (default 'cuda:0'), '--quiet' (nothing is written or announced), 'dist' (a parallel.DataParallelContext).
"""
from __future__ import annotations

import gc
import json
import os
import pickle
import random
import time
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from .data import MoleculeSet
from .utils import MLP, SMALL_NUMBER, ThreadedIterator

# mean absolute error at which each of the 13 QM9 targets counts as chemically accurate; error ratios are MAEs in these units
CHEMICAL_ACCURACIES = np.array([0.066513725, 0.012235489, 0.071939046, 0.033730778, 0.033486113, 0.004278493, 0.001330901,
                                0.004165489, 0.004128926, 0.00409976, 0.004527465, 0.012292586, 0.037467458])


def start_readback(stats: torch.Tensor):
    """Start the device->host copy of a step's statistics on a SIDE stream, behind an event recorded where they were computed.
    `tensor.cpu()` would put the copy on the training stream, i.e. behind everything queued there: with the next step
    already enqueued the host then waits for that whole step, the launch queue runs dry once per step and the GPU idles
    while the following step is being enqueued (1.1 ms of a 7.2 ms fresh-batch step).  Returns (host tensor, event)."""
    if not stats.is_cuda:
        return (stats, None)
    from .backward import side_stream
    rb = side_stream(stats.device)          # (shared with the weight-gradient products: they are done before the step's end)
    ready = torch.cuda.Event()
    ready.record()
    host = torch.empty(stats.shape, dtype=stats.dtype, device='cpu', pin_memory=True)
    with torch.cuda.stream(rb):
        rb.wait_event(ready)
        host.copy_(stats, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
    stats.record_stream(rb)
    return (host, done)


class EpochStats:
    """What one epoch accumulates: run_epoch feeds it one step at a time, result() gives the epoch's figures.

    A step's loss and per-task MAE stay on the device until the NEXT step has been queued: reading them at once would stall the
    launching thread until the GPU has finished the step, and the GPU would idle while the next step's launches are issued.  The
    progress line therefore trails by one batch; the epoch's result does not.  Under data parallelism a rank sees one shard of
    each step's global batch: the loss / MAE numerators and mask counts stay on the device and are summed over the ranks once per
    epoch, so that EVERY rank derives the same figures and hence the same best-epoch / patience decisions (ranks that disagreed
    would leave the others hanging in the next gradient all-reduce)."""
    def __init__(self, model, epoch_name: str):
        self.model, self.epoch_name, self.task_ids = model, epoch_name, model.params['task_ids']
        self.sharded = model.dist is not None and model.dist.active
        self.started, self.steps, self.graphs = time.time(), 0, 0
        self.loss_sum, self.accuracy_sums = 0, []            # unsharded: sums of (value * the step's graph count)
        self.pending = None                                  # unsharded: the last step's read-back, not yet in the sums
        self.shard_stats, self.shard_graphs = [], []         # sharded: per step, what reduce_over_ranks takes

    def add(self, batch_loss: torch.Tensor, ops: Dict[str, Any], num_graphs: int) -> None:
        self.graphs += num_graphs
        if self.sharded:
            self.shard_stats.append(torch.stack([ops[k % t].detach().to(torch.float64).reshape(()) for k in (
                'loss_numerator_task%i', 'loss_denominator_task%i', 'abs_error_sum_task%i') for t in self.task_ids]))
            self.shard_graphs.append(float(num_graphs))
        else:
            stats = torch.stack([batch_loss.detach().reshape(()).to(torch.float64)] +
                                [ops['accuracy_task%i' % t].detach().reshape(()).to(torch.float64) for t in self.task_ids])
            readback = start_readback(stats)
            self.absorb_pending()
            self.pending = (readback, self.steps, num_graphs, self.graphs)
        self.steps += 1

    def absorb_pending(self) -> None:
        """Wait for the pending read-back, add it to the sums and print the progress line of its step."""
        if self.pending is None:
            return
        (host, done), step, num_graphs, graphs_so_far = self.pending
        self.pending = None
        if done is not None:
            done.synchronize()
        vals = host.numpy()
        self.loss_sum += float(vals[0]) * num_graphs
        self.accuracy_sums.append(vals[1:] * num_graphs)
        if not self.model.quiet:
            print("Running %s, batch %i (has %i graphs). Loss so far: %.4f" % (
                self.epoch_name, step, num_graphs, self.loss_sum / graphs_so_far), end='\r')

    @staticmethod
    def reduce_over_ranks(model, shard_stats, shard_graphs):
        """(loss, per-task MAE, graphs) of an epoch under data parallelism, by ONE all-reduce: per step the global batch's loss
        is sum_tasks (sum_ranks numerator) / (sum_ranks mask count + 1e-7) * ratio -- the masked loss on the union of the
        shards --, and the steps are weighted by their global graph counts.  `model` needs only params and dist."""
        K = len(model.params['task_ids'])
        if not shard_stats:
            return 0.0, np.zeros(K), 0
        packed = torch.cat([torch.stack(shard_stats),
                            torch.tensor(shard_graphs, dtype=torch.float64, device=shard_stats[0].device)[:, None]], dim=1)
        model.dist.all_reduce_sum_(packed)
        packed = packed.cpu().numpy()
        num, den, abs_sum, graphs = packed[:, :K], packed[:, K:2 * K], packed[:, 2 * K:3 * K], packed[:, 3 * K]
        ratios = np.array([ChemModel.task_ratio(model, t) for t in model.params['task_ids']])
        step_loss = (num / (den + SMALL_NUMBER) * ratios).sum(axis=1)
        step_acc = abs_sum / (den + SMALL_NUMBER)
        total = graphs.sum()
        return float((step_loss * graphs).sum() / total), (step_acc * graphs[:, None]).sum(axis=0) / total, int(total)

    def result(self):
        """(loss, per-task MAE, per-task error ratio, graphs per second, steps): loss and MAE are means over the epoch's graphs."""
        self.absorb_pending()
        if self.sharded:
            loss, maes, graphs = self.reduce_over_ranks(self.model, self.shard_stats, self.shard_graphs)
        else:
            graphs = self.graphs
            maes = np.sum(self.accuracy_sums, axis=0) / graphs
            loss = self.loss_sum / graphs
        return loss, maes, maes / CHEMICAL_ACCURACIES[self.task_ids], graphs / (time.time() - self.started), self.steps


class BestEpoch:
    """The best (lowest) validation score so far, the epoch that reached it, and the early-stopping rule."""
    def __init__(self, patience: int):
        self.patience, self.score, self.epoch = patience, float("+inf"), 0

    def update(self, epoch: int, score) -> str:
        """'improved' when `score` becomes the new best, 'stop' when `patience` epochs have passed since the best one, else ''."""
        if score < self.score:
            self.score, self.epoch = score, epoch
            return 'improved'
        return 'stop' if epoch - self.epoch >= self.patience else ''


class ChemModel(object):
    @classmethod
    def default_params(cls):
        # the configuration schema (chem_tensorflow.py:18-37): a checkpoint's params are compared against it key for key
        return {
            'num_epochs': 3000,
            'patience': 25,
            'learning_rate': 0.001,
            'clamp_gradient_norm': 1.0,
            'out_layer_dropout_keep_prob': 1.0,
            'hidden_size': 100,
            'num_timesteps': 4,
            'use_graph': True,
            'tie_fwd_bkwd': True,
            'task_ids': [0],
            'random_seed': 0,
            'train_file': 'molecules_train.json',
            'valid_file': 'molecules_valid.json'
        }

    def __init__(self, args):
        self.args, self.quiet, self.dist = args, bool(args.get('--quiet')), args.get('dist')
        self.device = torch.device(args.get('--device') or 'cuda:0')
        self._name_run_files()
        self.params = self.resolve_params(args)
        self._announce_run()
        self._seed(self.params['random_seed'])
        self.max_num_vertices = self.num_edge_types = self.annotation_size = 0        # (load_data raises them to the data's)
        self.train_data = self.load_data(args.get('train_data', self.params['train_file']), is_training_data=True)
        self.valid_data = self.load_data(args.get('valid_data', self.params['valid_file']), is_training_data=False)
        self._build()
        checkpoint = args.get('--restore')
        self.train_step_id, self.valid_step_id = (0, 0) if checkpoint is None else self.restore_progress(checkpoint)

    # ---- construction steps -----------------------------------------------------------------------
    def _name_run_files(self) -> None:
        self.data_dir, self._log_dir = self.args.get('--data_dir') or '', self.args.get('--log_dir') or '.'
        self.run_id = "%s_%i" % (time.strftime("%Y-%m-%d-%H-%M-%S"), os.getpid())
        self.log_file, self.best_model_file = self._run_file("log.json"), self._run_file("model_best.pickle")

    def _run_file(self, suffix: str) -> str:
        return os.path.join(self._log_dir, "%s_%s" % (self.run_id, suffix))

    @classmethod
    def resolve_params(cls, args) -> Dict[str, Any]:
        """The run's parameters from their three sources, later ones winning: default_params(), the JSON file that --config-file
        names, and --config (a JSON string, or the dict itself)."""
        sources = [cls.default_params()]
        if args.get('--config-file') is not None:
            with open(args['--config-file']) as f:
                sources.append(json.load(f))
        inline = args.get('--config')
        if inline is not None:
            sources.append(json.loads(inline) if isinstance(inline, str) else inline)
        return {key: value for source in sources for key, value in source.items()}

    def _announce_run(self) -> None:
        if self.quiet:
            return
        os.makedirs(self._log_dir, exist_ok=True)
        with open(self._run_file("params.json"), "w") as f:
            json.dump(self.params, f)
        print("Run %s starting with following parameters:\n%s" % (self.run_id, json.dumps(self.params)))

    def _seed(self, seed: int) -> None:
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        self.tf_generator = torch.Generator().manual_seed(seed)      # stands in for TensorFlow's graph-level seed (utils.tf_glorot_uniform)

    def _build(self) -> None:
        self.placeholders, self.weights, self.ops = {}, {}, {}          # name -> fed tensor / variables / the last batch's values
        self.training, self.dropout_step = False, 0      # dropout_step: optimisation steps taken, part of every dropout mask's key
        self.make_model()
        self.make_train_step()

    # ---- data ---------------------------------------------------------------------------------
    def load_data(self, source, is_training_data: bool):
        """`source` is a file name under data_dir, a raw JSON list or a MoleculeSet.  Raises num_edge_types (the highest bond id,
        doubled when forward and backward edges are not tied), annotation_size and max_num_vertices to what the data need."""
        if source is None:
            return None
        if isinstance(source, MoleculeSet):
            ms = source
        elif isinstance(source, (list, tuple)):
            ms = MoleculeSet.from_json(source)
        else:
            full_path = os.path.join(self.data_dir, source)
            if not self.quiet:
                print("Loading data from %s" % full_path)
            ms = MoleculeSet.load(full_path)
        limit = self.args.get("--restrict_data")
        if limit is not None and limit > 0:
            ms = ms.subset(np.arange(min(limit, ms.num_graphs)))
        if ms.num_graphs:
            self.max_num_vertices = max(self.max_num_vertices, int(ms.nodes_per_graph().max()) - 1)
            self.num_edge_types = max(self.num_edge_types, ms.num_fwd_edge_types * (1 if self.params['tie_fwd_bkwd'] else 2))
            self.annotation_size = max(self.annotation_size, ms.annotation_size)
        return self.process_raw_graphs(ms, is_training_data)

    def process_raw_graphs(self, raw_data, is_training_data: bool) -> Any:
        raise Exception("Models have to implement process_raw_graphs!")

    # ---- model ----------------------------------------------------------------------------------
    def make_model(self):
        """The placeholders and the weights: the graph model's and each task's read-out MLPs (the per-batch arithmetic is in forward_batch)."""
        self.placeholders['target_values'] = None
        self.placeholders['target_mask'] = None
        self.placeholders['num_graphs'] = None
        self.placeholders['out_layer_dropout_keep_prob'] = 1.0
        self.prepare_specific_graph_model()
        for task_id in self.params['task_ids']:
            keep = lambda: self.placeholders['out_layer_dropout_keep_prob']
            self.weights['regression_gate_task%i' % task_id] = MLP(2 * self.params['hidden_size'], 1, [], keep, device=self.device)
            self.weights['regression_transform_task%i' % task_id] = MLP(self.params['hidden_size'], 1, [], keep, device=self.device)
            for kind in ('regression_gate', 'regression_transform'):
                self.weights['%s_task%i' % (kind, task_id)].dropout_seed = \
                    lambda layer, kind=kind, task_id=task_id: self.dropout_seed(kind, task_id, layer)

    def dropout_seed(self, *site) -> int:
        """Key of the dropout mask drawn at `site` in the current optimisation step: a hash of (random_seed, step, site), hence
        identical on every rank of a data-parallel job whatever else a rank draws (the reference's masks come from TF's
        graph-seeded stream, chem_tensorflow.py:85; under DP every rank must hold the same weight mask)."""
        from .utils import dropout_seed
        return dropout_seed(self.params['random_seed'], self.dropout_step, *site)

    def named_variables(self) -> Dict[str, torch.Tensor]:
        """All trainable tensors under TF-style variable names (chem_tensorflow.py:311-313 naming)."""
        out = dict(self.graph_model_variables())
        for task_id in self.params['task_ids']:
            for scope, key in (("regression_gate", 'regression_gate_task%i'), ("regression", 'regression_transform_task%i')):
                mlp = self.weights[key % task_id]
                for i, (W, b) in enumerate(zip(mlp.params["weights"], mlp.params["biases"])):
                    out["out_layer_task%i/%s/MLP_W_layer%i:0" % (task_id, scope, i)] = W
                    out["out_layer_task%i/%s/MLP_b_layer%i:0" % (task_id, scope, i)] = b
        return out

    def graph_model_variables(self) -> Dict[str, torch.Tensor]:
        return {}

    def forward_batch(self, batch_data: Dict[str, Any]):
        """One batch (chem_tensorflow.py:141-170): final node representations, per-task gated regression, masked loss and MAE."""
        self.feed(batch_data)
        if self.params['use_graph']:
            final = self.compute_final_node_representations()
        else:
            final = torch.zeros_like(self.placeholders['initial_node_representation'])   # :147
        self.ops['final_node_representations'] = final
        task_losses = self.ops['losses'] = []
        fused_readout = getattr(self, 'gated_regression_with_loss', None)
        if self._forward_tasks_multi(final):
            return self.ops['loss']
        for internal_id, task_id in enumerate(self.params['task_ids']):
            gate_mlp = self.weights['regression_gate_task%i' % task_id]
            transform_mlp = self.weights['regression_transform_task%i' % task_id]
            task_targets = self.placeholders['target_values'][internal_id, :]
            task_mask = self.placeholders['target_mask'][internal_id, :]
            # models with a fused readout + loss kernel (one forward and one backward launch group on the GPU) return the
            # prediction together with the three masked sums of :161-166; None -> the op-by-op form below
            fused = fused_readout(final, gate_mlp, transform_mlp, task_targets, task_mask) if fused_readout else None
            if fused is not None:
                computed_values, loss_num, abs_sum, mask_sum = fused
            else:
                computed_values = self.gated_regression(final, gate_mlp, transform_mlp)
                diff = computed_values - task_targets                                         # :161
                diff = diff * task_mask                                                       # :164
                loss_num, abs_sum, mask_sum = (0.5 * diff * diff).sum(), diff.abs().sum(), task_mask.sum()
            task_target_num = mask_sum + SMALL_NUMBER                                         # :163
            self.ops['accuracy_task%i' % task_id] = abs_sum / task_target_num                 # :165
            task_loss = loss_num / task_target_num                                            # :166
            task_loss = task_loss * self.task_ratio(task_id)
            task_losses.append(task_loss)
            self.ops['loss_numerator_task%i' % task_id] = loss_num
            self.ops['abs_error_sum_task%i' % task_id] = abs_sum
            self.ops['loss_denominator_task%i' % task_id] = mask_sum
        self.ops['loss'] = torch.stack(task_losses).sum()                                     # :170
        return self.ops['loss']

    def task_ratio(self, task_id) -> float:
        """The factor on a task's loss: 1 / task_sample_ratios[task_id], 1 where the task has none.  The id is looked up as
        task_ids holds it (chem_tensorflow.py:168); a configuration that keys its ratios by str therefore gets 1."""
        return 1.0 / (self.params['task_sample_ratios'].get(task_id) or 1.0)

    def task_ratio_factors(self, device) -> torch.Tensor:
        """[K] float32: task_ratio per entry of task_ids, cached on the device."""
        vals = tuple(self.task_ratio(t) for t in self.params['task_ids'])
        cached = getattr(self, '_task_ratio_factors', None)
        if cached is None or cached[0] != (vals, str(device)):
            self._task_ratio_factors = cached = ((vals, str(device)), torch.tensor(vals, dtype=torch.float32, device=device))
        return cached[1]

    def publish_task_stats(self, out: torch.Tensor, num: torch.Tensor, ab: torch.Tensor, ms: torch.Tensor) -> torch.Tensor:
        """The per-task entries of self.ops (:161-170) from the multi-task readout's out [K,G] and masked sums [K] each, by a
        constant number of torch ops: the entries are views of the K-vectors.  Returns the loss."""
        task_ids = self.params['task_ids']
        den = ms + SMALL_NUMBER                                                               # :163
        accuracy = ab / den                                                                   # :165
        task_losses = num / den * self.task_ratio_factors(num.device)                         # :166, :168
        for name, vec in (('accuracy_task%i', accuracy), ('loss_numerator_task%i', num), ('abs_error_sum_task%i', ab),
                          ('loss_denominator_task%i', ms)):
            for entry, task_id in zip(vec.unbind(0), task_ids):
                self.ops[name % task_id] = entry
        self.ops['losses'] = list(task_losses.unbind(0))
        self.ops['loss'] = task_losses.sum()                                                  # :170
        self.output = out[len(task_ids) - 1]                                                  # (the per-task loop leaves the last task's)
        return self.ops['loss']

    def _forward_tasks_multi(self, final) -> bool:
        """params['multitask_readout'] (default False; read with .get: not a key of default_params, whose keys a reference checkpoint
        must match): the gated regression and masked loss of EVERY task in one fused pass (autograd.readout_loss_multi) instead of
        one per entry of task_ids.  False -- and the per-task loop runs -- for one task, and wherever the model's
        gated_regression_with_loss_multi says the multi-task kernels do not apply (it returns None)."""
        multi = getattr(self, 'gated_regression_with_loss_multi', None)
        if not self.params.get('multitask_readout') or multi is None or len(self.params['task_ids']) < 2:
            return False
        fused = multi(final)
        if fused is None:
            return False
        self.publish_task_stats(*fused)
        return True

    def feed(self, batch_data: Dict[str, Any]) -> None:
        """The reference's feed_dict: every placeholder the batch carries is replaced.  Values DERIVED from a fed
        placeholder and cached next to it (the message index built from 'adjacency_lists', the dense model's sparse
        form of 'adjacency_matrix') are dropped unless the batch brings its own, so a reference-style feed dict can
        never run on the previous batch's index."""
        for src, derived in self.DERIVED_PLACEHOLDERS.items():
            if src in batch_data and batch_data[src] is not self.placeholders.get(src):   # (same object: cache stays valid)
                for d in derived:
                    if d not in batch_data:
                        self.placeholders[d] = None
        self.placeholders.update(batch_data)

    DERIVED_PLACEHOLDERS = {'adjacency_lists': ('message_index',),
                            'adjacency_matrix': ('_sparse_form', 'adjacency_absmax', '_adjacency_absmax_of'),
                            'initial_node_representation': ('h0_absmax', '_h0_absmax_of'),      # (formats.h0_absmax: measured once per fed h0)
                            'graph_nodes_list': ('graph_ptr', 'graph_nodes_sorted', 'graph_ids', 'node_uid')}

    def make_train_step(self):
        """Adam(lr) on all trainable variables (minus graph_model/* when --freeze-graph-model), per-variable clip_by_norm."""
        from .train import TFAdam
        variables = self.named_variables()
        if self.args.get('--freeze-graph-model'):
            graph_vars = set(self.graph_model_variables().keys())
            for name in graph_vars:
                if not self.quiet:
                    print("Freezing weights of variable %s." % name)
            variables = {k: v for k, v in variables.items() if k not in graph_vars}
        self.trainable_variables = variables
        self.optimizer = TFAdam(list(variables.values()), lr=self.params['learning_rate'])

    def gated_regression(self, last_h, regression_gate, regression_transform):
        raise Exception("Models have to implement gated_regression!")

    def prepare_specific_graph_model(self) -> None:
        raise Exception("Models have to implement prepare_specific_graph_model!")

    def compute_final_node_representations(self) -> torch.Tensor:
        raise Exception("Models have to implement compute_final_node_representations!")

    def make_minibatch_iterator(self, data: Any, is_training: bool):
        raise Exception("Models have to implement make_minibatch_iterator!")

    # ---- training loop ----------------------------------------------------------------------------
    def train_batch(self, batch_data: Dict[str, Any]):
        """One optimisation step: forward, backward, per-variable clipping, Adam."""
        from .train import train_step
        try:
            return train_step(self, batch_data)
        finally:
            self.dropout_step += 1

    def threaded_batches_default(self) -> bool:
        """Whether run_epoch packs training batches on a producer thread when params['threaded_batches'] is 'auto'.
        The producer thread pays when the launching thread is the bottleneck (the autograd path: ~4 ms of Python per step);
        with the native step the host has slack, packing a batch inline costs 0.3 ms of it, and a second thread only takes
        the interpreter lock away from the launches (5.8 vs 6.05 ms per step, tools/bench_extra.py epoch)."""
        from . import train_native
        return not (train_native.model_eligible(self) or train_native.attn_model_eligible(self) or train_native.panel_model_eligible(self)
                    or train_native.rnn_model_eligible(self))

    def _epoch_batches(self, data, is_training: bool):
        """The epoch's batches.  In a training epoch with params['threaded_batches'] ('auto': threaded_batches_default) a producer thread
        packs the next two on the model's packer stream while this one trains; validation batches are packed once and stay resident."""
        batches = self.make_minibatch_iterator(data, is_training)
        threaded = self.params.get('threaded_batches', 'auto')
        if threaded == 'auto':
            threaded = self.threaded_batches_default()
        if not (is_training and threaded):
            return batches
        prepare = getattr(self, 'prepare_resident_data', None)
        if prepare is not None:
            prepare(data, is_training)               # resident dataset + tables on THIS stream, before the producer starts
        if self.device.type == "cuda" and torch.cuda.is_available() and getattr(self, '_packer_stream', None) is None:
            self._packer_stream = torch.cuda.Stream(self.device)   # one packer stream for all epochs of this model
        return ThreadedIterator(batches, max_queue_size=2, device=self.device, stream=getattr(self, '_packer_stream', None))

    def run_epoch(self, epoch_name: str, data, is_training: bool, start_step: int = 0):
        """One pass over `data`, training or evaluating; returns (loss, accuracies, error_ratios, instances_per_sec, steps) -- see
        EpochStats.result.  `start_step` numbered the summaries of the TensorFlow implementation; nothing here needs it."""
        stats = EpochStats(self, epoch_name)
        run_batch = self.train_batch if is_training else torch.no_grad()(self.forward_batch)
        keep_prob = self.params['out_layer_dropout_keep_prob'] if is_training else 1.0
        for batch_data in self._epoch_batches(data, is_training):
            num_graphs = batch_data['num_graphs']
            batch_data['out_layer_dropout_keep_prob'] = keep_prob
            stats.add(run_batch(batch_data), self.ops, num_graphs)
        return stats.result()

    def _result_line(self, kind: str, result) -> str:
        """The line train() prints after a training ('Train') or validation ('Valid') epoch."""
        loss, accs, errs, speed = result[:4]
        per_task = lambda values: " ".join("%i:%.5f" % pair for pair in zip(self.params['task_ids'], values))
        return "\r\x1b[K %s: loss: %.5f | acc: %s | error_ratio: %s | instances/sec: %.2f" % (kind, loss, per_task(accs), per_task(errs), speed)

    def _log_epoch(self, log: List[dict], epoch: int, elapsed: float, train_result, valid_result) -> None:
        """Append the epoch's entry to `log` and, unless --quiet, rewrite the log file."""
        logged = lambda r: (r[0], r[1].tolist(), r[2].tolist(), r[3])
        log.append({'epoch': epoch, 'time': elapsed, 'train_results': logged(train_result), 'valid_results': logged(valid_result)})
        if not self.quiet:
            with open(self.log_file, 'w') as out:
                json.dump(log, out, indent=4)

    def _save_best(self, score, previous) -> None:
        if not self.quiet and (self.dist is None or self.dist.rank == 0):      # one writer under data parallelism
            self.save_progress(self.best_model_file, self.train_step_id, self.valid_step_id)
            print("  (Best epoch so far, cum. val. acc decreased to %.5f from %.5f. Saving to '%s')" % (score, previous, self.best_model_file))

    def train(self):
        """Train for num_epochs, or until the summed validation MAE has not improved for `patience` epochs; returns the log entries.
        A restored model first scores one validation epoch, which then counts as the best so far."""
        log, started = [], time.time()
        # Move everything alive so far (torch, the datasets, the model) out of the cyclic collector's reach: a full
        # collection over them stalls the launching thread for tens of ms, during which the GPU queue runs dry.
        gc.collect()
        gc.freeze()
        best = BestEpoch(self.params['patience'])
        restored_from, last_epoch = self.args.get('--restore'), self.params['num_epochs']
        if restored_from is not None:
            resumed = self.run_epoch("Resumed (validation)", self.valid_data, False)
            best.score = np.sum(resumed[1])
            self.valid_step_id += resumed[4]
            print("\r\x1b[KResumed operation, initial cum. val. acc: %.5f" % best.score)
        for epoch in range(1, last_epoch + 1):
            print("== Epoch %i" % epoch)
            train_result = self.run_epoch("epoch %i (training)" % epoch, self.train_data, True, self.train_step_id)
            self.train_step_id += train_result[4]
            print(self._result_line("Train", train_result))
            valid_result = self.run_epoch("epoch %i (validation)" % epoch, self.valid_data, False, self.valid_step_id)
            self.valid_step_id += valid_result[4]
            print(self._result_line("Valid", valid_result))
            self._log_epoch(log, epoch, time.time() - started, train_result, valid_result)
            score, previous = np.sum(valid_result[1]), best.score
            verdict = best.update(epoch, score)
            if verdict == 'improved':
                self._save_best(score, previous)
            elif verdict == 'stop':
                print("Stopping training after %i epochs without improvement on validation accuracy." % self.params['patience'])
                break
        return log

    # ---- checkpoints: a pickle {params, weights, train_step, valid_step}, weights under TF variable names -----------
    def save_progress(self, model_path: str, train_step: int, valid_step: int) -> None:
        """named_variables() and the optimizer's state variables (Adam slots, beta powers, step) as arrays by name, params, the step counters."""
        weights = {name: t.detach().cpu().numpy() for name, t in self.named_variables().items()}
        weights.update(self.optimizer.state_variables(self.trainable_variables))
        checkpoint = {"params": self.params, "weights": weights, "train_step": train_step, "valid_step": valid_step}
        with open(model_path, 'wb') as f:
            pickle.dump(checkpoint, f, pickle.HIGHEST_PROTOCOL)

    def check_checkpoint_params(self, saved: Dict[str, Any]) -> None:
        """A checkpoint restores only into the configuration it was written with, key for key; task_ids and num_epochs may differ."""
        if len(self.params) != len(saved):
            raise AssertionError("the model and the checkpoint differ in the parameter keys %s" % sorted(set(saved) ^ set(self.params)))
        for key, value in self.params.items():
            if key not in ('task_ids', 'num_epochs') and (key not in saved or saved[key] != value):
                raise AssertionError("parameter %r is %r in the model but %r in the checkpoint" % (key, value, saved.get(key, '<absent>')))

    def restore_progress(self, model_path: str) -> (int, int):
        """Load save_progress's file into the model and the optimizer, by name; returns (train_step, valid_step)."""
        if not self.quiet:
            print("Restoring weights from file %s." % model_path)
        with open(model_path, 'rb') as f:
            checkpoint = pickle.load(f)
        self.check_checkpoint_params(checkpoint['params'])
        saved = checkpoint['weights']
        variables = self.named_variables()
        for name, t in variables.items():
            if name in saved:
                with torch.no_grad():
                    t.copy_(torch.from_numpy(np.asarray(saved[name])).to(t.device).reshape(t.shape))
            else:
                print('Freshly initializing %s since no saved value was found.' % name)
        known = set(variables) | self.optimizer.load_state_variables(self.trainable_variables, saved)
        for name in saved:
            if name not in known:
                print('Saved weights for %s not used by model.' % name)
        return checkpoint['train_step'], checkpoint['valid_step']
