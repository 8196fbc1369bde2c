"""CPU tests of the optimiser-side arithmetic and of the data-parallel reduction (gloo, world_size 2):
TF-1.3 Adam, per-variable clip_by_norm, and 'shard -> sum all-reduce == one big batch' for the
reference's masked-loss normalisation with UNEQUAL shard sizes."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def test_tf_adam_matches_formula(pkg):
    torch.manual_seed(0)
    v = torch.randn(7, 3); v0 = v.clone()
    opt = pkg.train.TFAdam([v], lr=0.01)
    m = torch.zeros_like(v); s = torch.zeros_like(v); ref = v0.clone()
    for t in range(1, 5):
        g = torch.randn(7, 3)
        opt.apply_gradients([g.clone()])
        m = 0.9 * m + 0.1 * g; s = 0.999 * s + 0.001 * g * g
        lr_t = 0.01 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        ref = ref - lr_t * m / (s.sqrt() + 1e-8)
        assert torch.allclose(v, ref, atol=1e-7)
    named = {"a/b:0": v}
    state = opt.state_variables(named)
    assert set(state) == {"beta1_power:0", "beta2_power:0", "ggnn_amd/adam_step:0", "a/b/Adam:0", "a/b/Adam_1:0"}
    opt2 = pkg.train.TFAdam([v.clone()], lr=0.01)
    used = opt2.load_state_variables(named, state)
    assert opt2.t == 4 and torch.allclose(opt2.m[0], opt.m[0]) and "a/b/Adam_1:0" in used


def test_clip_by_norm_is_per_variable(pkg):
    a = torch.full((4,), 3.0)      # norm 6 -> scaled to norm 1
    b = torch.full((4,), 0.1)      # norm 0.2 -> untouched
    grads = [a.clone(), None, b.clone()]
    pkg.train.clip_by_norm_(grads, 1.0)
    assert abs(float(grads[0].norm()) - 1.0) < 1e-6
    assert torch.equal(grads[2], b)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


class _ToyModel:
    """Stand-in with the two hooks DataParallelContext uses: params + ops[loss numerator/denominator]."""
    def __init__(self, w):
        self.params = {"task_ids": [0], "task_sample_ratios": {}}
        self.ops = {}
        self.w = w

    def forward(self, x, y, mask):
        diff = (x.matmul(self.w).squeeze(-1) - y) * mask
        self.ops["loss_numerator_task0"] = (0.5 * diff * diff).sum()
        self.ops["loss_denominator_task0"] = mask.sum()


def _host_rank():
    """The gloo workers below rehearse the host side of data parallelism on CPU tensors: they must not claim cuda:<rank>,
    which a box with fewer GPUs than ranks does not have.  (Spawned process: the patch dies with it.)"""
    torch.cuda.is_available = lambda: False


def _dp_worker(rank, world, port, ret):
    import importlib
    pkg = importlib.import_module("gated-graph-neural-network-samples_amd")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    _host_rank()
    ctx = pkg.parallel.DataParallelContext.from_env(backend="gloo")
    g = torch.Generator().manual_seed(0)
    X = torch.randn(10, 4, generator=g, dtype=torch.float64); Y = torch.randn(10, generator=g, dtype=torch.float64)
    mask = torch.tensor([1, 1, 0, 1, 1, 1, 1, 0, 1, 1], dtype=torch.float64)
    w0 = torch.randn(4, 1, generator=g, dtype=torch.float64)
    cut = 3                                    # UNEQUAL shards: 3 graphs on rank 0, 7 on rank 1
    sl = slice(0, cut) if rank == 0 else slice(cut, 10)
    w = w0.clone().float().requires_grad_(True)
    model = _ToyModel(w)
    model.forward(X[sl].float(), Y[sl].float(), mask[sl].float())
    loss = ctx.global_loss(model)
    loss.backward()
    grads = [w.grad]
    ctx.reduce_gradients([w], grads)
    # weights broadcast
    wb = torch.full((4, 1), float(rank))
    ctx.broadcast_([wb])
    total = loss.detach().clone(); ctx.all_reduce_sum_(total)
    if rank == 0:
        wf = w0.clone().requires_grad_(True)
        diff = (X.matmul(wf).squeeze(-1) - Y) * mask
        full = (0.5 * diff * diff).sum() / (mask.sum() + 1e-7)
        full.backward()
        ret["grad_err"] = float((grads[0].double() - wf.grad).abs().max())
        ret["loss_err"] = abs(float(total) - float(full))
        ret["bcast_ok"] = bool((wb == 0).all())
    dist.destroy_process_group()


def test_data_parallel_reduction_equals_single_batch_gloo(pkg):
    port = _free_port()
    mgr = mp.Manager(); ret = mgr.dict()
    mp.spawn(_dp_worker, args=(2, port, ret), nprocs=2, join=True)
    assert ret["grad_err"] < 1e-6 and ret["loss_err"] < 1e-6 and ret["bcast_ok"]


def _dp8_worker(rank, world, port, ret):
    """world_size 8 over gloo: every rank packs ITS shard of one epoch (data.pack_batches -> epoch_boundaries), the ranks
    all-reduce what they hold, a gradient-sized flat buffer, and a toy model's sharded loss gradient."""
    import importlib
    pkg = importlib.import_module("gated-graph-neural-network-samples_amd")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    _host_rank()
    ctx = pkg.parallel.DataParallelContext.from_env(backend="gloo")
    ms = pkg.synthetic_qm9(900, mean_nodes=12, seed=5)
    params = {"batch_size": 1000, "hidden_size": 100}
    order = np.random.default_rng(3).permutation(ms.num_graphs)            # the epoch's shuffle: the same on every rank
    batches = pkg.data.pack_batches(ms, params, 4, order, None, rank, world)
    held = np.zeros(ms.num_graphs)
    steps = torch.tensor([float(len(batches))], dtype=torch.float64)
    nodes = torch.zeros(world, 16, dtype=torch.float64)                    # [rank, step] node counts
    bounds = pkg.data.epoch_boundaries(np.diff(ms.node_ptr)[order], params["batch_size"], world, True)
    for s_, b in enumerate(batches):
        nodes[rank, s_] = b.num_nodes
        i = s_ * world + rank
        held[order[bounds[i]:bounds[i + 1]]] += 1
        assert b.num_graphs == bounds[i + 1] - bounds[i] and 0 < b.num_nodes < params["batch_size"]
    held_t = torch.from_numpy(held); ctx.all_reduce_sum_(held_t); ctx.all_reduce_sum_(nodes)
    smax = steps.clone(); ctx.all_reduce_max_(smax); smin = -steps.clone(); ctx.all_reduce_max_(smin)
    # the flat gradient all-reduce at the default model's size (591,802 floats)
    variables = [torch.zeros(400, 100), torch.zeros(591802 - 40000)]
    grads = [torch.full_like(v, float(rank + 1)) for v in variables]
    ctx.reduce_gradients(variables, grads)
    # sharded masked loss == the one-batch loss, 8 UNEQUAL shards (one of them without a single labelled graph)
    g = torch.Generator().manual_seed(0)
    n = 40
    X = torch.randn(n, 4, generator=g, dtype=torch.float64); Y = torch.randn(n, generator=g, dtype=torch.float64)
    mask = (torch.rand(n, generator=g) > 0.2).double()
    cuts = [0, 1, 3, 4, 10, 17, 18, 30, 40]
    mask[cuts[2]:cuts[3]] = 0
    w0 = torch.randn(4, 1, generator=g, dtype=torch.float64)
    sl = slice(cuts[rank], cuts[rank + 1])
    w = w0.clone().float().requires_grad_(True)
    model = _ToyModel(w)
    model.forward(X[sl].float(), Y[sl].float(), mask[sl].float())
    loss = ctx.global_loss(model)
    loss.backward()
    tg = [w.grad]
    ctx.reduce_gradients([w], tg)
    if rank == 0:
        wf = w0.clone().requires_grad_(True)
        diff = (X.matmul(wf).squeeze(-1) - Y) * mask
        full = (0.5 * diff * diff).sum() / (mask.sum() + 1e-7)
        full.backward()
        per_rank = nodes.sum(1).numpy()
        ret.update(covered=bool((held_t == 1).all()), steps_equal=float(smax) == -float(smin), steps=float(smax),
                   rank_nodes=per_rank.tolist(), step_nodes=nodes[:, :int(smax)].numpy().tolist(),
                   flat_ok=all(bool((x == 36.0).all()) for x in grads), grad_err=float((tg[0].double() - wf.grad).abs().max()))
    dist.barrier()
    dist.destroy_process_group()


def test_world_size_8_sharding_and_flat_allreduce_gloo(pkg):
    """Round-3 review: the 8-rank path had only ever run with 2 ranks.  Eight gloo ranks: the epoch sharder partitions the
    dataset, every rank takes the same number of steps, every step is node-balanced across the ranks, the flat 2.4 MB
    all-reduce returns the sum, and the sharded masked loss is the one-batch loss."""
    port = _free_port()
    mgr = mp.Manager(); ret = mgr.dict()
    mp.spawn(_dp8_worker, args=(8, port, ret), nprocs=8, join=True)
    assert ret["covered"] and ret["steps_equal"] and ret["flat_ok"] and ret["grad_err"] < 1e-6
    rn = np.asarray(ret["rank_nodes"])
    assert rn.max() / rn.min() < 1.02, rn                                   # per-rank node counts within 2 %
    sn = np.asarray(ret["step_nodes"])
    assert (sn > 0).all() and (sn.max(0) / sn.min(0)).max() < 1.05, sn      # and no step waits on a padding batch


def test_epoch_boundaries_balance_full_qm9_sized_epoch(pkg):
    """data.epoch_boundaries on a full-QM9-sized epoch (133,885 molecules, ~25 greedy batches of < 100,000 nodes) for 8 ranks:
    32 batches, each below batch_size, node counts within 2 % of each other (dealing the 25 greedy batches to 8 ranks leaves
    7 of 32 slots empty: 0.78 epoch efficiency); one rank or balance off: the reference's greedy batches."""
    rng = np.random.default_rng(0)
    n = np.clip(np.rint(rng.normal(18, 3, 133885)), 3, 29).astype(np.int64)
    greedy = pkg.data.batch_boundaries(n, 100000)
    assert pkg.data.epoch_boundaries(n, 100000, 1, True) == greedy == pkg.data.epoch_boundaries(n, 100000, 8, False)
    nb = len(greedy) - 1
    assert nb % 8 != 0
    for world in (2, 4, 8):
        b = pkg.data.epoch_boundaries(n, 100000, world, True)
        k = len(b) - 1
        assert k == -(-nb // world) * world and b[0] == 0 and b[-1] == len(n) and (np.diff(b) > 0).all()
        sizes = np.add.reduceat(n, b[:-1])
        assert sizes.max() < 100000 and sizes.max() / sizes.min() < 1.02
        per_rank = np.array([sizes[r::world].sum() for r in range(world)])
        assert per_rank.max() / per_rank.min() < 1.02
        # epoch efficiency: work / (steps * the slowest rank's step)
        eff = sizes.sum() / (world * sizes.reshape(-1, world).max(1).sum())
        assert eff > 0.98
    # few graphs / tiny epochs fall back to the greedy cut instead of producing empty batches
    assert pkg.data.epoch_boundaries(np.array([5, 5, 5]), 8, 8, True) == pkg.data.batch_boundaries(np.array([5, 5, 5]), 8)


def test_checkpoint_roundtrip_reference_pickle_schema(pkg, tmp_path):
    """chem_tensorflow.py:309-359: pickle {params, weights{tf var name -> ndarray}, train_step, valid_step},
    restore by variable name incl. Adam slots; runs on CPU (weights only, no kernels)."""
    import pickle
    ms = pkg.synthetic_qm9(30, mean_nodes=8, seed=1)
    args = {"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms}
    m1 = pkg.SparseGGNNChemModel(dict(args))
    g = [torch.randn_like(v) for v in m1.trainable_variables.values()]
    m1.optimizer.apply_gradients(g)
    path = str(tmp_path / "model.pickle")
    m1.save_progress(path, 7, 3)
    blob = pickle.load(open(path, "rb"))
    assert set(blob) == {"params", "weights", "train_step", "valid_step"} and blob["train_step"] == 7
    names = set(blob["weights"])
    assert "graph_model/gnn_layer_0/gnn_edge_weights_0:0" in names
    assert "graph_model/gnn_layer_4/timestep_0/gru_cell/gates/kernel:0" in names
    assert "out_layer_task0/regression_gate/MLP_W_layer0:0" in names
    assert "graph_model/gnn_layer_0/gnn_edge_weights_0/Adam:0" in names and "beta1_power:0" in names
    assert blob["weights"]["graph_model/gnn_layer_0/gnn_edge_weights_0:0"].shape == (400, 100)
    assert blob["weights"]["graph_model/gnn_layer_4/timestep_0/gru_cell/gates/kernel:0"].shape == (400, 200)
    a2 = dict(args); a2["--restore"] = path
    m2 = pkg.SparseGGNNChemModel(a2)
    assert (m2.train_step_id, m2.valid_step_id) == (7, 3)
    for (n1, v1), (n2, v2) in zip(m1.named_variables().items(), m2.named_variables().items()):
        assert n1 == n2 and torch.equal(v1, v2)
    assert m2.optimizer.t == 1 and all(torch.equal(a, b) for a, b in zip(m1.optimizer.m, m2.optimizer.m))
    # frozen graph model: only the readout MLPs stay trainable (chem_tensorflow.py:174-182)
    a3 = dict(args); a3["--freeze-graph-model"] = True
    m3 = pkg.SparseGGNNChemModel(a3)
    assert all(k.startswith("out_layer_task") for k in m3.trainable_variables) and len(m3.trainable_variables) == 4


def test_adam_step_restored_from_long_reference_checkpoint(pkg):
    """A checkpoint written by the reference has no step counter, only TF's float32 beta powers.  0.9^(t+1) is zero in
    float32 after ~1000 steps (a few dozen QM9 epochs); the step must then come from beta2_power (round-1 advisor finding:
    math.log(0.0) crashed --restore)."""
    v = torch.zeros(3)
    for t in (0, 1, 7, 250, 900, 1500, 5000, 40000):
        b1p, b2p = np.float32(1.0), np.float32(1.0)
        for _ in range(t + 1):                                   # TF: beta_power *= beta after every step, in float32
            b1p = np.float32(b1p * np.float32(0.9)); b2p = np.float32(b2p * np.float32(0.999))
        opt = pkg.train.TFAdam([v.clone()])
        opt.load_state_variables({"w:0": v}, {"beta1_power:0": b1p, "beta2_power:0": b2p})
        assert abs(opt.t - t) <= max(1, t // 2000), (t, opt.t, float(b1p), float(b2p))
    # both powers gone (beyond ~87k steps): a large step, no exception; the bias corrections are 1 there
    opt = pkg.train.TFAdam([v.clone()])
    opt.load_state_variables({"w:0": v}, {"beta1_power:0": np.float32(0.0), "beta2_power:0": np.float32(0.0)})
    assert opt.t >= 100000
    g = torch.ones(3)
    opt.apply_gradients([g])                                     # lr_t is finite
    assert torch.isfinite(opt.vars[0]).all()


def test_feed_drops_index_derived_from_previous_batch(pkg):
    """Advisor finding: a reference-style feed (adjacency_lists, no 'message_index') must not reuse the cached index of
    the previous batch."""
    ms = pkg.synthetic_qm9(12, mean_nodes=6, seed=2)
    m = pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cpu", "train_data": None, "valid_data": ms})
    adj1, adj2 = [torch.zeros((1, 2), dtype=torch.int32)], [torch.zeros((2, 2), dtype=torch.int32)]
    m.feed({"adjacency_lists": adj1, "message_index": "index-of-batch-1"})
    assert m.placeholders["message_index"] == "index-of-batch-1"
    m.feed({"adjacency_lists": adj1})                            # the same lists object: the cache stays valid
    assert m.placeholders["message_index"] == "index-of-batch-1"
    m.feed({"adjacency_lists": adj2})                            # another batch without an index of its own
    assert m.placeholders["message_index"] is None
    m.feed({"adjacency_lists": adj1, "message_index": "again"})
    assert m.placeholders["message_index"] == "again"


def test_any_hidden_size_and_residual_fan_in_are_accepted(pkg):
    """The reference takes any hidden_size and any number of residual inputs per layer (chem_tensorflow_sparse.py:46-50, 139-145,
    211-212).  Sizes the kernels do not take as they are run zero-padded to ops.kernel_width (variables keep the reference's
    shapes); up to 6 residual inputs per layer; what cannot run fails at construction, not in the first batch."""
    ms = pkg.synthetic_qm9(12, mean_nodes=6, seed=2)
    base = {"--quiet": True, "--device": "cpu", "train_data": None, "valid_data": ms}
    assert [pkg.ops.kernel_width(d) for d in (20, 30, 52, 84, 100, 116, 96, 200, 260)] == [32, 32, 64, 100, 100, 128, 96, 200, 288]
    m = pkg.SparseGGNNChemModel(dict(base, **{"--config": {"hidden_size": 30}}))
    assert m._kw == 32 and m._edge_weight_vars[0].shape == (m.num_edge_types * 30, 30)
    assert m.gnn_weights.rnn_cells[0].gates_kernel.shape == (60, 60)
    ew, eb, attn, cell = m._kernel_layer(4, False)                       # layer 4: residual inputs [0, 2] -> 3 x + h row blocks
    assert ew.shape == (m.num_edge_types, 32, 32) and cell.gates_kernel.shape == (4 * 32, 64) and cell.candidate_bias.shape == (32,)
    Wg = m.gnn_weights.rnn_cells[4].gates_kernel
    assert torch.equal(cell.gates_kernel[32:62, 32:62], Wg[30:60, 30:60]) and float(cell.gates_kernel[30:32].abs().sum()) == 0.0
    assert m._kernel_layer(4, False)[0] is ew                            # cached per weight version
    m6 = pkg.SparseGGNNChemModel(dict(base, **{"--config": {"layer_timesteps": [1] * 7, "residual_connections": {"6": [0, 1, 2, 3, 4, 5]}}}))
    assert m6.gnn_weights.rnn_cells[6].gates_kernel.shape == (8 * 100, 200)
    with pytest.raises(ValueError, match="residual"):
        pkg.SparseGGNNChemModel(dict(base, **{"--config": {"layer_timesteps": [1] * 8, "residual_connections": {"7": [0, 1, 2, 3, 4, 5, 6]}}}))
    with pytest.raises(ValueError, match="not computed yet"):
        pkg.SparseGGNNChemModel(dict(base, **{"--config": {"residual_connections": {"1": [2]}}}))


def test_dense_task_sample_ratios_mask_labels(pkg):
    """chem_tensorflow_dense.py:153-158,180-189: per bucket, the labels of the examples beyond the sampled share
    feed value 0 / mask 0 (advisor finding: the dense packer trained on every label)."""
    ms = pkg.synthetic_qm9(96, mean_nodes=7, seed=5)
    cfg = {"batch_size": 8, "task_sample_ratios": {"0": 0.25}}
    m = pkg.DenseGGNNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms, "--config": cfg})
    tr, va = m.train_data, m.valid_data
    assert va["label_mask"].min() == 1.0                         # validation data are never masked
    lm = tr["label_mask"]
    for bucket in tr["bucketed"].values():
        keep = int(len(bucket) * 0.25)
        assert lm[np.asarray(bucket), 0].sum() == keep
    total_masked = 0
    for feed in m.make_minibatch_iterator(tr, is_training=True):
        tm, tv = feed["target_mask"], feed["target_values"]
        assert tm.shape == tv.shape and set(np.unique(tm.numpy())) <= {0.0, 1.0}
        assert (tv[tm == 0] == 0).all()
        total_masked += int((tm == 0).sum())
    assert total_masked > 0


def test_device_dataset_rejects_bond_outside_its_graph(pkg):
    raw = [{"targets": [[0.0]], "graph": [[0, 1, 1]], "node_features": [[1, 0, 0, 0, 0]] * 2},
           {"targets": [[0.0]], "graph": [[0, 1, 2]], "node_features": [[1, 0, 0, 0, 0]] * 2}]     # node 2 of a 2-node graph
    ms = pkg.data.MoleculeSet.from_json(raw)
    with pytest.raises(IndexError, match="graph 1"):
        pkg.data_device.DeviceMoleculeSet(ms, "cpu")


def _epoch_stats_worker(rank, world, port, ret):
    import importlib
    import types
    pkg = importlib.import_module("gated-graph-neural-network-samples_amd")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    _host_rank()
    ctx = pkg.parallel.DataParallelContext.from_env(backend="gloo")
    stub = types.SimpleNamespace(params={"task_ids": [0, 1], "task_sample_ratios": {}}, dist=ctx)
    rng = np.random.default_rng(7)                                 # the same stream on both ranks: [step, rank, ...]
    steps = 3
    num = rng.uniform(1, 2, (steps, world, 2)); den = rng.integers(1, 9, (steps, world, 2)).astype(float)
    ab = rng.uniform(1, 2, (steps, world, 2)); graphs = rng.integers(1, 9, (steps, world)).astype(float)
    graphs[2, 1] = 0; num[2, 1] = 0; den[2, 1] = 0; ab[2, 1] = 0    # rank 1's last batch is an empty padding batch
    stats = [torch.tensor(np.concatenate([num[s, rank], den[s, rank], ab[s, rank]])) for s in range(steps)]
    loss, accs, total = pkg.chem_model.EpochStats.reduce_over_ranks(stub, stats, list(graphs[:, rank]))
    N, Dn, A, G = num.sum(1), den.sum(1), ab.sum(1), graphs.sum(1)
    want_loss = float(((N / (Dn + 1e-7)).sum(1) * G).sum() / G.sum())
    want_acc = ((A / (Dn + 1e-7)) * G[:, None]).sum(0) / G.sum()
    ret[rank] = (abs(loss - want_loss), float(np.abs(accs - want_acc).max()), total == int(G.sum()), loss)
    dist.destroy_process_group()


def test_epoch_statistics_are_identical_on_every_rank_gloo(pkg):
    """Advisor finding: under data parallelism every rank must derive the same epoch loss / MAE (they decide on the
    best epoch and on early stopping; ranks that disagree hang the next all-reduce)."""
    port = _free_port()
    mgr = mp.Manager(); ret = mgr.dict()
    mp.spawn(_epoch_stats_worker, args=(2, port, ret), nprocs=2, join=True)
    assert ret[0][0] < 1e-12 and ret[0][1] < 1e-12 and ret[0][2] and ret[1][2]
    assert ret[0][3] == ret[1][3]                                  # bit-identical on the two ranks


def test_threaded_iterator_mirrors_reference_prefetcher(pkg):
    """utils.ThreadedIterator (reference utils.py:16-36): same elements in the same order, producer at most max_queue_size
    ahead, a producer exception surfaces in the consumer, and a consumer that stops early does not leave the producer stuck."""
    import threading, time
    TI = pkg.utils.ThreadedIterator
    assert list(TI(iter(range(100)), max_queue_size=3)) == list(range(100))
    assert list(TI(iter(()), max_queue_size=1)) == []
    produced = []

    def gen(n):
        for i in range(n):
            produced.append(i)
            yield i

    it = iter(TI(gen(50), max_queue_size=2))
    assert next(it) == 0
    time.sleep(0.2)
    assert len(produced) <= 1 + 2 + 1                    # consumed + queue + the one the producer holds while the queue is full
    before = threading.active_count()
    it.close()                                           # early exit: the producer must be released
    time.sleep(0.3)
    assert threading.active_count() <= before - 1 and len(produced) < 50

    def bad():
        yield 1
        raise KeyError("boom")

    got = []
    with pytest.raises(KeyError):
        for x in TI(bad(), max_queue_size=2):
            got.append(x)
    assert got == [1]


def test_bench_spawns_its_own_ranks_dry_run():
    """Round-2 review item 1: `python bench.py --gpus 2` started WITHOUT a launcher must bring up its own two ranks (it used
    to die on an assert).  --dry-run keeps everything around the kernels: rendezvous on 127.0.0.1, the rank/world sharding
    of the host packer, the flat gradient all-reduce (gloo here, RCCL on GPUs), the barrier-bracketed timing."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GGNN_LOCAL_DEVICE="0", GGNN_DIST_BACKEND="gloo")           # (a box with fewer GPUs than ranks: all on device 0, gloo)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-run", "--steps", "3"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["dry_run"] is True
    assert line["sharded_graphs_total"] == line["dataset_graphs"]            # the two shards partition the dataset
    assert line["allreduce_us"] > 0 and line["allreduce_bytes"] == 591802 * 4  # 591,802 parameters
    # a wrong --gpus / WORLD_SIZE pairing is an error message, not an assert
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-run"], env=env2, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and "--gpus 2" in r.stderr


def test_bench_gpus_8_dry_run():
    """The driver's 8-GPU launch line (`python bench.py --gpus 8 ...`) up to the kernels: eight gloo ranks on this box."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GGNN_LOCAL_DEVICE="0", GGNN_DIST_BACKEND="gloo")           # (a box with fewer GPUs than ranks: all on device 0, gloo)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--dry-run", "--steps", "2", "--n1-value", "1.25e9"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 8 and line["ranks_seen"] == 8 and line["dry_run"] is True
    assert line["n1_value"] == 1.25e9                 # (the N = 1 value reaches every rank: the real line carries weak_scaling_efficiency)
    assert line["sharded_graphs_total"] == line["dataset_graphs"]
    assert line["allreduce_us"] > 0 and line["allreduce_bytes"] == 591802 * 4
    assert line["batches_total_incl_padding"] % 8 == 0 and line["rank_nodes_max_over_min"] < 1.05


def test_dropout_seed_is_a_pure_function_of_seed_step_site(pkg):
    ds = pkg.utils.dropout_seed
    a = ds(0, 3, "edge_weights", 2)
    assert a == ds(0, 3, "edge_weights", 2) and 0 <= a < 2 ** 64
    assert len({ds(0, 3, "edge_weights", 2), ds(1, 3, "edge_weights", 2), ds(0, 4, "edge_weights", 2), ds(0, 3, "edge_weights", 1),
                ds(0, 3, "state", 2, 0)}) == 5
    assert a == 0xeb003e833a661aac                                                         # platform-independent (blake2b of the repr)


def test_bench_prices_kernels_against_the_pipe_of_their_operand_format():
    """bench.py's per-kernel roofline records (round-3 review, weak #1: no `frac` above 1, `peak` = the pipe the kernel runs on): an
    f32-MFMA kernel against 157.3 TF, a six-product bf16 kernel against 2500 / 6, the fused GRU in the two-piece f16 format (round 4)
    against 2500 / 3 -- the same achieved rate, three different ceilings -- and `bound` = the roof the kernel's arithmetic intensity
    puts it under: the GRU's 74 flop/B lie above the ridge of the f32 MFMA (20) and of the six-product form (52), below the
    three-product form's (104), where the HBM roof is the nearer one."""
    import importlib.util, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    V, M, D, T, R = 100000, 200000, 100, 4, 120000
    res = {"gru_fused_gather[nx=1]": [0.070] * 6, "msg_transform_compact": [0.025] * 8}
    want = 6.0 * V * 2 * D * D / 70e-6 / 1e12                         # TF of f32-equivalent work
    gbytes = float(2 * V * D * 4 + M * D * 4 + M * 4 + V * 4 + V * T * 4)
    for split, fmt, peak, gbound in ((False, 0, 157.3, "mfma"), (True, 3, 2500.0 / 6, "mfma"), (True, 2, 2500.0 / 3, "hbm")):
        bench.SPLIT_ACTIVE, bench.GRU_FWD_FORMAT = split, fmt
        k, tot = bench.kernel_table(res, 1, V, M, D, T, R)
        g = k["gru_fused_gather[nx=1]"]
        assert abs(g["mfma_achieved"] - want) < 1e-6 * want and abs(g["mfma_peak"] - peak) < 1e-9 and abs(g["mfma_frac"] - want / peak) < 1e-9
        assert g["mfma_frac"] <= 1.0 or not split
        assert abs(g["arithmetic_intensity"] - 6.0 * V * 2 * D * D / gbytes) < 1e-9 and abs(g["ridge_point"] - peak * 1e12 / 8e12) < 1e-9
        assert g["bound"] == gbound
        if gbound == "hbm":
            assert g["unit"] == "GB/s" and g["peak"] == 8000.0 and abs(g["achieved"] - gbytes / 70e-6 / 1e9) < 1e-6 and g["frac"] == g["hbm_frac"] < 1.0
        else:
            assert g["unit"] == "TFLOP/s" and g["achieved"] == g["mfma_achieved"] and g["frac"] == g["mfma_frac"]
        t = k["msg_transform_compact"]                                 # the transform stays on the six-product form: 27 flop/B
        assert abs(t["mfma_peak"] - (2500.0 / 6 if split else 157.3)) < 1e-9 and t["bound"] == ("hbm" if split else "mfma")
        assert abs(tot - (6 * 0.070 + 8 * 0.025)) < 1e-12
    assert g["pipe"].startswith("f16 MFMA") and "f16x2" in g["matrix_path"]


def test_bench_exact_format_reference_leg_never_raises():
    """bench.py's `exact_bf16x3_gru_reference`: the child's JSON line is parsed into the record; a child that dies, hangs or prints
    nothing yields an error record, never an exception (the leg must not take the headline down)."""
    import importlib.util, json, os, subprocess, types
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module2", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    args = types.SimpleNamespace(steps=20, warmup=5, streams=2, batches=6, mean_nodes=18.0)
    seen = {}

    def ok_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        line = {"value": 9.5e8, "unit": "node-state updates/s", "ms_per_step": 0.84, "ms_per_step_one_stream": 0.97, "gru_forward_format": "bf16x3",
                "roofline": {"kernel": "gru_fused_gather[nx=1]", "bound": "mfma", "frac": 0.33}, "config": {"nodes_per_batch": 99990, "graphs_per_batch": 11000}}
        return types.SimpleNamespace(returncode=0, stdout="noise\n" + json.dumps(line) + "\n", stderr="")
    rec = bench.exact_format_reference(args, 1.2e9, run=ok_run)
    assert rec["value"] == 9.5e8 and rec["gru_forward_format"] == "bf16x3" and abs(rec["value_ratio_default_over_exact"] - 1.2e9 / 9.5e8) < 1e-12
    assert seen["env"]["GGNN_GRU_FMT"] == "3" and seen["env"]["GGNN_BENCH_CHILD"] == "1"          # (the child must not spawn a child)
    # (the exact leg times its kernels too: its own roofline rides on the line as `roofline_exact`)
    assert "--no-secondary" in seen["cmd"] and "--no-roofline" not in seen["cmd"] and "--no-cpu-baseline" in seen["cmd"]
    assert rec["roofline"]["frac"] == 0.33
    small = bench.small_molecule_reference(args, run=ok_run)        # BASELINE.json's "~9 nodes" wording, as a secondary leg
    assert small["value"] == 9.5e8 and small["mean_nodes_per_graph"] == 9.0 and small["graphs_per_batch"] == 11000
    assert seen["cmd"][seen["cmd"].index("--mean-nodes") + 1] == "9" and "--no-roofline" in seen["cmd"]
    assert "error" in bench.small_molecule_reference(args, run=lambda cmd, **kw: types.SimpleNamespace(returncode=1, stdout="", stderr="x"))

    def dead_run(cmd, **kw):
        return types.SimpleNamespace(returncode=1, stdout="", stderr="boom")

    def hung_run(cmd, **kw):
        raise subprocess.TimeoutExpired(cmd, 120)
    assert "error" in bench.exact_format_reference(args, 1.2e9, run=dead_run)
    assert "error" in bench.exact_format_reference(args, 1.2e9, run=hung_run)


def test_bench_compact_line_fits_a_captured_tail():
    """bench.py prints ONE JSON line on stdout, last: the contract's fields plus roofline / cpu_baseline and the headline figures of
    the other legs -- short enough that a driver's captured tail keeps `train`, `end_to_end_fresh_batch` and `allreduce_us` (round 4's
    15 KB line lost them); the per-kernel tables go to gpurun_out/bench_detail.json and stderr."""
    import importlib.util, json, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module3", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    blob = "x" * 4000
    out = {"metric": "node-state updates/sec on QM9-shaped graphs, h=100, 4 edge types", "value": 1.4e9, "unit": "node-state updates/s",
           "n_gpus": 1, "steps": 96, "warmup": 12, "ms_per_step": 0.57, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32", "data": "synthetic", "matrix_path": blob,
           "config": {"workload": "sparse GGNN forward propagation, full-QM9-sized synthetic batches (configs[1])", "mode": "forward",
                      "hidden_size": 100, "layer_timesteps": [2, 2, 1, 2, 1], "parallelism": "dp1"},
           "operand_format": {"gru_forward": "f16x2", "gru_forward_per_layer": ["f16x2"] * 5, "policy": "auto", "selected_by": blob,
                              "bounds": {"proven": True, "h0_absmax": 1.0}, "every_other_kernel": "bf16x3 (exact)"},
           "exact_bf16x3_gru_reference": {"what": blob, "value": 1.1e9},
           "roofline": {"kernel": "gru_fused_gather[nx=1]", "bound": "hbm", "achieved": 2900.0, "peak": 8000.0, "unit": "GB/s", "frac": 0.36,
                        "traffic": 1.36e8, "matrix_path": blob, "pipe": blob, "sustained_mfma": {"a": blob}},
           "kernels": {"k%d" % i: {"what": blob} for i in range(8)},
           "cpu_baseline": {"value": 4.8e5, "unit": "node-state updates/s", "cores": 16, "kind": "port", "sample": blob,
                            "thread_sweep_node_updates_per_sec": {str(t): 1.0 for t in range(40)}},
           "train": {"what": blob, "ms_per_step": 3.4, "value": 2.3e8}, "end_to_end_fresh_batch": {"what": blob, "value": 1.0e9},
           "secondary": {"config3_dense_b256": {"kernels": blob, "ms_per_step": 0.05}, "config5_large_graph_h256": {"error": "boom"}},
           "allreduce_us": None, "ranks_seen": 1, "graphs_per_sec": 9.0e6}
    line = bench.compact_line(out, "gpurun_out/bench_detail.json")
    text = json.dumps(line)
    assert len(text) < 3500, len(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["roofline"]["frac"] == 0.36 and line["roofline"]["bound"] == "hbm" and "8 TB/s" in line["roofline"]["peak_is"]
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["cores"] == 16
    assert line["operand_format"]["gru_forward"] == "f16x2" and line["operand_format"]["proven"] is True
    assert line["exact_format_value"] == 1.1e9 and line["train"]["ms_per_step"] == 3.4 and line["end_to_end_fresh_batch"]["value"] == 1.0e9
    assert line["secondary"]["config5_large_graph_h256"] == {"error": "boom"} and line["detail_file"].endswith("bench_detail.json")
